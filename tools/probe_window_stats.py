"""What --window_stats costs per cycle, at the headline shape (T 5, N 32, 4 actions) and at the Seaquest shard (T 20, N 128, 18
actions): the replayed device cycle with the flag on against off -- the flag adds one launch of one workgroup behind the
update (paac_window_fold) -- and the fold on its own, back to back.  The two settings alternate window by window; every
window is printed, then median, minimum and spread ((max - min) / median) per setting.  Prints one JSON line.

  python tools/probe_window_stats.py [--windows 9] [--cycles 400] [--repeats 400]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import train, window_stats  # noqa: E402
from paac_amd.paac import DeviceRollout, PAACLearner  # noqa: E402


def stats(us):
    us = np.asarray(us, dtype=np.float64)
    return dict(median=float(np.median(us)), min=float(us.min()), spread=float((us.max() - us.min()) / np.median(us)),
                windows=[round(float(u), 3) for u in us])


def timed(fn, count):
    """us per call of fn(count) between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(count)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


def rollout(T, N, game, on):
    args = train.get_arg_parser().parse_args(["--window_stats", "true" if on else "false"])
    args.game, args.arch = game, "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = N, T, 0
    args.max_global_steps = 1 << 40
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_probe_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    L.global_step = L.init_network()
    return L, DeviceRollout(L, ec.device_env_spec, sampler="numpy", use_graph=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--cycles", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=400)
    a = ap.parse_args()
    out = dict(windows=a.windows, cycles=a.cycles, repeats=a.repeats, us={})
    for T, N, A, game in ((5, 32, 4, "breakout"), (20, 128, 18, "seaquest")):
        res = {}
        pair = {on: rollout(T, N, game, on) for on in (False, True)}
        assert pair[True][0].num_actions == A and pair[True][1].window_f is not None and pair[False][1].window_f is None
        cyc = {False: [], True: []}
        for w in range(a.windows + 1):
            for on in (False, True):
                ro = pair[on][1]
                with torch.cuda.stream(ro.stream):
                    us = timed(lambda c: (ro.run_cycles(c), ro.synchronize()), a.cycles)
                if w:                                     # (window 0: capture and warm-up)
                    cyc[on].append(us)
        res["cycle_off"], res["cycle_window_stats"] = stats(cyc[False]), stats(cyc[True])
        res["added_us_median"] = res["cycle_window_stats"]["median"] - res["cycle_off"]["median"]
        # -- the fold on its own, on the tensors the last cycle left.  Back-to-back launches: the per-launch figure includes
        # the launch gap, so it bounds the kernel from above
        L, ro = pair[True]
        one = lambda c: [L.window_fold(ro.window_f, ro.window_i, ro.values, ro.rewards, ro.masks, ro.actions, ro.y, ro.adv,
                                       truncs=ro.truncs, finished=ro.finished) for _ in range(c)]
        with torch.cuda.stream(ro.stream):
            one(20)
            res["fold_back_to_back"] = stats([timed(one, a.repeats) for _ in range(a.windows)])
        block = window_stats.Block(ro.window_f.cpu().numpy(), ro.window_i.cpu().numpy())
        res["rows_folded"] = int(block.get("rows"))
        assert np.isfinite(block.f).all()
        for on in (False, True):
            pair[on][1].close()
        del pair
        out["us"]["T%d_N%d_A%d" % (T, N, A)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
