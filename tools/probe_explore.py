"""What one --explore_bonus call costs: paac_explore_bonus timed by the context's timing hooks (the dispatch's own begin / end
stamps) at --rows rows of random stacks, beside its bounds: the bytes it must move (the observations once from HBM; the int8
sign operand once per 32 rows out of L2) and the int8 MFMA issue time.  One JSON line per row count; medians over --repeats calls
of THIS process."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops  # noqa: E402

HBM_BYTES_PER_US, CUS, CLOCK_MHZ, MFMA_CYCLES = 8e6, 256, 2400.0, 32      # v_mfma_i32_16x16x64_i8: 8 passes of 4 cycles

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[160, 2688])
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda")
    ctx = hip_ops.Context(_lib.ARCH_NIPS, 4, max_batch=8)          # (the timing hooks live on a context)
    for rows in a.rows:
        block = hip_ops.explore_block(dev, 3, 32, 20, rows)
        states = torch.randint(0, 256, (rows, _lib.EXPLORE_K), dtype=torch.uint8, device=dev)
        rewards, bonus = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
        call = lambda: hip_ops.explore_bonus(block, states, 0.1, rewards, bonus)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        for _ in range(a.repeats):
            call()
        torch.cuda.synchronize()
        us = np.array([m for _, _, m in ctx.prof_read()]) * 1e3
        ctx.prof_enable(False)
        groups = -(-rows // 32)
        obs_bytes, sign_bytes = rows * _lib.EXPLORE_K, groups * _lib.EXPLORE_SIGN_BYTES
        mfmas = groups * 2 * 4 * (_lib.EXPLORE_K // 64)
        print(json.dumps(dict(rows=rows, repeats=a.repeats, kernel_us_median=float(np.median(us)), kernel_us_min=float(us.min()),
                              kernel_us_p90=float(np.percentile(us, 90)), observation_bytes=obs_bytes, sign_bytes_l2=sign_bytes,
                              hbm_floor_us=obs_bytes / HBM_BYTES_PER_US, mfma_issue_us=mfmas * MFMA_CYCLES / (4 * CUS) / CLOCK_MHZ)))
    ctx.close()
