"""What one --redo_every recycle costs: the two recycle launches (mask + apply) timed by the context's timing hooks (the
dispatches' own begin / end stamps, first launch's begin to last launch's end), and the wall time of the whole entry (the
repack of the derived weight copies included, through a stream synchronisation).  A share --fraction of every layer's units is
made dormant.  Beside them the byte floor: the unit sums and mask words read, the touched 16-byte quads of the parameters and
both slots written, over 8 TB/s.  One JSON line; medians over --repeats calls of THIS process."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops, redo  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--arch", default="NATURE", choices=("NIPS", "NATURE"))
    ap.add_argument("--fraction", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    arch_id = {"NIPS": _lib.ARCH_NIPS, "NATURE": _lib.ARCH_NATURE}[a.arch]
    dev = torch.device("cuda")
    ctx = hip_ops.Context(arch_id, 4, max_batch=8)
    n = ctx.layout["total"]
    acc_f, _, lay = hip_ops.feature_block(dev, arch_id)
    rs = np.random.RandomState(0)
    sums = 1.0 + rs.rand(lay.U)
    for _, _, units, at in lay.layers():
        sums[at + rs.choice(units, max(1, int(round(a.fraction * units))), replace=False)] = 0.0
    acc_f[:lay.U] = torch.from_numpy(sums).to(dev)
    params, s0, s1 = (torch.randn(n, device=dev) for _ in range(3))
    mask, counts = torch.zeros(lay.U, dtype=torch.int32, device=dev), torch.zeros(12, dtype=torch.int32, device=dev)
    ctx.set_managed_weights(True)
    call = lambda: ctx.redo(params, s0, s1, redo.RMSPROP, lay, acc_f, 0.025, 3, 1, mask, counts)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    wall = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    kernels_us = np.array([m for _, _, m in ctx.prof_read()]) * 1e3
    # the quads a recycle must write, from the twin: elements that differ between two fills mark the touched ones
    host = [np.full(n, v, dtype=np.float32) for v in (2.0, 3.0, 4.0)]
    totals = redo.recycle(ctx.layout, host[0], host[1:], mask.cpu().numpy(), 3, 1, redo.RMSPROP)
    quads = int((host[1] != 3.0).reshape(-1, 4).any(axis=1).sum())
    floor_bytes = lay.U * (8 + 4) + lay.U * 4 + quads * 16 * 3
    print(json.dumps(dict(arch=a.arch, fraction=a.fraction, repeats=a.repeats, recycled=int(mask.sum().item()), units=lay.U,
                          touched_quads=quads, all_quads=n // 4, **totals, kernels_us_median=float(np.median(kernels_us)),
                          kernels_us_min=float(kernels_us.min()), entry_wall_us_median=float(np.median(wall)),
                          floor_bytes=floor_bytes, byte_floor_us=floor_bytes / 8e6)))
