"""What --feature_stats costs.  Two modes, one JSON line each:

  --mode launches --arch NIPS|NATURE --rows R   the three launches of one fold (Gram, unit statistics, reduce) and the finish
      launch on random post-ReLU activations of the architecture's layer shapes, timed by the context's timing hooks (the
      dispatches' own begin / end stamps); medians over --repeats folds of THIS process -- run it in fresh processes and take
      the median of those.  Beside each: the bytes it must read over 8 TB/s and, for the Gram, the upper triangle's fp32
      MFMA work over the --peak_tflops given.
  --mode cycle   the replayed device cycle at the headline shape (T 5, N 32, NATURE) with the flag on against off, alternated
      window by window like tools/probe_window_stats.py, and the wall time of one record with and without the Gram's
      download and eigenvalues (--feature_rank_every)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, feature_stats, hip_ops  # noqa: E402
from probe_window_stats import stats, timed  # noqa: E402

PLANES = {"NIPS": (400, 81), "NATURE": (400, 81, 49)}


def launches(a):
    arch_id = {"NIPS": _lib.ARCH_NIPS, "NATURE": _lib.ARCH_NATURE}[a.arch]
    dev = torch.device("cuda")
    ctx = hip_ops.Context(arch_id, 4, max_batch=8)
    acc_f, acc_i, lay = hip_ops.feature_block(dev, arch_id)
    acts = [torch.relu(torch.randn(a.rows, p, c, device=dev)) for p, c in zip(PLANES[a.arch], lay.units)]
    acts += [None] * (3 - len(acts)) + [torch.relu(torch.randn(a.rows, lay.H, device=dev))]
    scalars = torch.zeros(feature_stats.FINISH_SCALARS, dtype=torch.float64, device=dev)
    for _ in range(5):
        hip_ops.feature_fold(lay, acc_f, acc_i, acts)
        hip_ops.feature_finish(lay, acc_f, acc_i, 0.025, scalars)
    torch.cuda.synchronize()
    ctx.prof_enable(True)
    for _ in range(a.repeats):
        hip_ops.feature_fold(lay, acc_f, acc_i, acts)
        hip_ops.feature_finish(lay, acc_f, acc_i, 0.025, scalars)
    torch.cuda.synchronize()
    ms = np.array([m for _, _, m in ctx.prof_read()]).reshape(a.repeats, 4) * 1e3
    med = np.median(ms, axis=0)
    conv_bytes = sum(t.numel() * 4 for t in acts[:3] if t is not None)
    h_bytes = acts[3].numel() * 4
    n32 = lay.H // 32
    gram_flop = 2.0 * a.rows * (n32 * (n32 + 1) // 2) * 1024
    print(json.dumps(dict(mode="launches", arch=a.arch, rows=a.rows, repeats=a.repeats,
                          us=dict(gram=float(med[0]), unit_stats=float(med[1]), reduce=float(med[2]), finish=float(med[3])),
                          floor_us=dict(gram_bytes=h_bytes / 8e6, gram_mfma=gram_flop / (a.peak_tflops * 1e6),
                                        unit_stats_bytes=(conv_bytes + h_bytes) / 8e6))))


def cycle(a):
    import tempfile
    from paac_amd import train
    from paac_amd.paac import DeviceRollout, PAACLearner

    def rollout(on):
        args = train.get_arg_parser().parse_args(["--feature_stats", "true" if on else "false"])
        args.game, args.arch = "breakout", "NATURE"
        args.emulator_counts, args.max_local_steps, args.emulator_workers = 32, 5, 0
        args.max_global_steps = 1 << 40
        args.debugging_folder = tempfile.mkdtemp(prefix="paac_probe_")
        nc, ec = train.get_network_and_environment_creator(args)
        L = PAACLearner(nc, ec, args)
        L.global_step = L.init_network()
        return L, DeviceRollout(L, ec.device_env_spec, sampler="numpy", use_graph=True)

    pair = {on: rollout(on) for on in (False, True)}
    cyc = {False: [], True: []}
    for w in range(a.windows + 1):
        for on in (False, True):
            ro = pair[on][1]
            with torch.cuda.stream(ro.stream):
                us = timed(lambda c: (ro.run_cycles(c), ro.synchronize()), a.cycles)
            if w:                                     # (window 0: capture and warm-up)
                cyc[on].append(us)
    res = dict(mode="cycle", cycle_off=stats(cyc[False]), cycle_feature_stats=stats(cyc[True]))
    res["added_us_median"] = res["cycle_feature_stats"]["median"] - res["cycle_off"]["median"]
    L, ro = pair[True]
    for every, name in ((0, "record_ms"), (1, "record_with_rank_ms")):
        L.feature_rank_every, took = every, []
        for _ in range(5):
            with torch.cuda.stream(ro.stream):
                ro.run_cycles(16)
                ro.synchronize()
                t0 = time.perf_counter()
                L._feature_read(ro.features)
                ro.synchronize()
                took.append((time.perf_counter() - t0) * 1e3)
        res[name] = float(np.median(took))
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--mode", choices=("launches", "cycle"), default="launches")
    ap.add_argument("--arch", default="NATURE")
    ap.add_argument("--rows", type=int, default=160)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--cycles", type=int, default=400)
    ap.add_argument("--peak_tflops", type=float, default=157.3)
    a = ap.parse_args()
    launches(a) if a.mode == "launches" else cycle(a)
