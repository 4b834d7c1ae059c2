"""--bootstrap_truncated on bricks and rally (32 environments, t_max 5, philox sampler, graph replay): what the flag costs per
cycle, and what it does to a run.

  python tools/probe_truncation.py time  [--blocks 5] [--cycles 400] [--warmup 100]
      cycle time of the same run with the flag off and on, bricks on the NATURE trunk (the headline shape's network and
      batch) and on the NIPS trunk, n-step and GAE(0.95): `blocks` blocks of `cycles` replayed cycles each between two events
      on the rollout's stream, microseconds per cycle, every block and the median.
  python tools/probe_truncation.py learn [--steps 4096000]
      the default flags (NIPS trunk, RMSProp, lr 0.0224: the settings of the games' own learning tests) on bricks and on
      rally, with and without the flag: per tenth of the run the mean return and mean length of the episodes finished in it
      (the last 4096 of them at most: the device ring's size) and the fraction of them that ended at the step cap.

Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import train  # noqa: E402
from paac_amd.paac import STATEFUL_KINDS, DeviceRollout, PAACLearner  # noqa: E402

N, T = 32, 5


def rollout(emulator, flags):
    args = train.get_arg_parser().parse_args(["--emulator", emulator] + flags)
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_probe_")
    args.emulator_workers, args.max_global_steps = 0, 1 << 40
    args.emulator_counts, args.max_local_steps = N, T
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    L = PAACLearner(network_creator, env_creator, args)
    L.network.initialize(np.random.RandomState(0))
    L.network.init = lambda folder, saver, session: 0
    L.global_step = L.init_network()
    return L, DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=True)


def time_cycles(a):
    out = {}
    for arch in ("NATURE", "NIPS"):
        for est, est_flags in (("nstep", []), ("gae", ["--gae_lambda", "0.95"])):
            for name in ("off", "on"):
                L, ro = rollout("bricks", ["--arch", arch, "--bootstrap_truncated", "true" if name == "on" else "false"] + est_flags)
                assert (ro.truncs is not None) == (name == "on")
                ro.run_cycles(a.warmup)
                ro.synchronize()
                us = []
                for _ in range(a.blocks):
                    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    start.record(ro.stream)
                    ro.run_cycles(a.cycles)
                    stop.record(ro.stream)
                    ro.synchronize()
                    us.append(start.elapsed_time(stop) * 1e3 / a.cycles)
                out["bricks/%s/%s/%s" % (arch, est, name)] = dict(us_per_cycle=[round(u, 2) for u in us],
                                                                  median=round(float(np.median(us)), 2))
                ro.close()
    return out


def learn(a):
    out = {}
    cycles = a.steps // (N * T)
    for emulator in ("bricks", "rally"):
        cap = STATEFUL_KINDS[emulator]["max_episode_steps"]
        for name in ("without", "with"):
            L, ro = rollout(emulator, ["--bootstrap_truncated", "true" if name == "with" else "false"])
            returns, lengths, capped, seen = [], [], [], 0
            for tenth in range(10):
                ro.run_cycles(cycles // 10)
                ro.synchronize()
                count, episodes = ro.finished_episodes()
                new = episodes[max(0, len(episodes) - (count - seen)):]
                seen = count
                returns.append(round(float(np.mean([r for r, _ in new])), 3) if new else None)
                lengths.append(round(float(np.mean([l for _, l in new])), 1) if new else None)
                capped.append(round(float(np.mean([l == cap for _, l in new])), 3) if new else None)
            out["%s/%s" % (emulator, name)] = dict(returns_by_tenth=returns, mean_length_by_tenth=lengths,
                                                   capped_fraction_by_tenth=capped, episodes=seen)
            ro.close()
    return dict(steps=cycles // 10 * 10 * N * T, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("what", choices=["time", "learn"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=4096000)
    a = ap.parse_args()
    print(json.dumps({a.what: time_cycles(a) if a.what == "time" else learn(a)}))


if __name__ == "__main__":
    main()
