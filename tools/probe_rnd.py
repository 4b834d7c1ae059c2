"""What one --explore_kind rnd call costs: the three launches of paac_rnd_bonus timed one by one by the context's timing hooks
(each dispatch's own begin / end stamps) at --rows rows of random stacks, beside their floors (bytes over HBM at 8 TB/s; fp32
MFMA issue spread over the workgroups the launch has); medians over --repeats calls of THIS process, one JSON line per row
count.  With --cycles N: what the flag adds to a cycle instead -- the device loop on catch at the default shape through the
captured graphs, off / simhash / rnd alternated twice in one process, three timed batches of N cycles each."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops, rnd, train  # noqa: E402

HBM_BYTES_PER_US, CUS, CLOCK_MHZ, MFMA_CYCLES = 8e6, 256, 2400.0, 32      # v_mfma_f32_16x16x4_f32: 8 passes of 4 cycles
KERNELS = ("rnd_hidden_kernel", "rnd_error_kernel", "rnd_step_kernel")


def floors(rows):
    """-> per launch (workgroups, HBM bytes, MFMAs of one wave's chain)."""
    tiles = -(-rows // 16)
    words = rows * 4
    return ((tiles * 4, rows * _lib.EXPLORE_K, 2 * 49),                                    # the stacks once; W1 out of L2
            (tiles, words * (256 + 272 + 64 + 256), 2 * 64 + 64),                           # HT, HP in; DO, DH out
            (276, words * (208 + 256 + 272 + 64) + 6 * 4 * rnd.NET, tiles))                 # U, DH, HP, DO in; w, m, v in and out


def calls(a):
    dev = torch.device("cuda")
    ctx = hip_ops.Context(_lib.ARCH_NIPS, 4, max_batch=8)          # (the timing hooks live on a context)
    for rows in a.rows:
        block = hip_ops.rnd_block(dev, 3, rows)
        states = torch.randint(0, 256, (rows, _lib.EXPLORE_K), dtype=torch.uint8, device=dev)
        rewards, bonus = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev)
        call = lambda: hip_ops.rnd_bonus(block, states, 0.1, 1e-4, rewards, bonus)
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        for _ in range(a.repeats):
            call()
        torch.cuda.synchronize()
        us = np.array([m for _, _, m in ctx.prof_read()]).reshape(-1, 3) * 1e3
        ctx.prof_enable(False)
        out = dict(rows=rows, repeats=a.repeats, call_us_median=float(np.median(us.sum(axis=1))))
        for k, (name, (wgs, hbm, chain)) in enumerate(zip(KERNELS, floors(rows))):
            out[name] = dict(us_median=float(np.median(us[:, k])), us_min=float(us[:, k].min()), us_p90=float(np.percentile(us[:, k], 90)),
                             workgroups=wgs, hbm_bytes=hbm, hbm_floor_us=hbm / HBM_BYTES_PER_US,
                             mfma_chain_us=chain * MFMA_CYCLES * max(1.0, wgs / CUS) / CLOCK_MHZ)
        print(json.dumps(out), flush=True)
    ctx.close()


def cycle(flags, cycles, warm):
    from paac_amd.paac import DeviceRollout, PAACLearner
    args = train.get_arg_parser().parse_args(["--emulator", "catch"] + flags)
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_rnd_")
    args.emulator_workers = 0
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    L = PAACLearner(network_creator, env_creator, args)
    L.network.initialize(np.random.RandomState(0))
    L.network.init = lambda folder, saver, session: 0
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=True)
    ro.run_cycles(warm)
    ro.synchronize()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        ro.run_cycles(cycles)
        ro.synchronize()
        out.append((time.perf_counter() - t0) / cycles * 1e6)
    ro.close()
    L.ctx.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[160, 2688])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--cycles", type=int, default=0)
    ap.add_argument("--warm", type=int, default=400)
    a = ap.parse_args()
    if a.cycles:
        for flags in 2 * ([], ["--explore_bonus", "0.1"], ["--explore_bonus", "0.1", "--explore_kind", "rnd"]):
            print(json.dumps(dict(flags=flags, us_per_cycle=cycle(flags, a.cycles, a.warm))), flush=True)
    else:
        calls(a)
