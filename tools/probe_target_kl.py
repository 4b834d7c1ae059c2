"""--ppo_target_kl on catch (NIPS trunk, 32 environments, t_max 5, philox sampler, graph replay): what the flag costs per
cycle, and what it does to a run that needs it.

  python tools/probe_target_kl.py time  [--blocks 5] [--cycles 400] [--warmup 100]
      cycle time of the same --ppo_epochs 4 run with the flag off, with a D that never stops (1e30) and with a D that stops
      (0.001): `blocks` blocks of `cycles` replayed cycles each between two events on the rollout's stream, microseconds per
      cycle, every block and the median; the fraction of optimizer steps the stopping run applied (sampled after each block).
  python tools/probe_target_kl.py learn [--steps 1536000] [--target_kl 0.02]
      --optimizer adam -lr 0.001 --e 1e-5 --ppo_epochs 8 with and without --ppo_target_kl: the mean return of the episodes
      finished in each tenth of the run (the last 4096 of them at most: the device ring's size), and the mean
      ppo_steps_applied (sampled every 16 cycles).

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
from paac_amd.paac import DeviceRollout, PAACLearner  # noqa: E402

N, T = 32, 5


def rollout(flags):
    args = train.get_arg_parser().parse_args(["--emulator", "catch"] + flags)
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
    for name, flags in (("off", []), ("never", ["--ppo_target_kl", "1e30"]), ("stopping", ["--ppo_target_kl", "0.001"])):
        L, ro = rollout(["--ppo_epochs", "4"] + flags)
        ro.run_cycles(a.warmup)
        ro.synchronize()
        us, applied = [], []
        for _ in range(a.blocks):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(ro.stream)
            ro.run_cycles(a.cycles)
            stop.record(ro.stream)
            ro.synchronize()
            us.append(start.elapsed_time(stop) * 1e3 / a.cycles)
            if L.target_kl_on:
                applied.append(float(L.ppo_applied.sum().item()) / L.ppo_steps)
        out[name] = dict(us_per_cycle=[round(u, 2) for u in us], median=round(float(np.median(us)), 2),
                         **(dict(applied_fraction=round(float(np.mean(applied)), 3)) if applied else {}))
        ro.close()
    return out


def learn(a):
    out = {}
    cycles = a.steps // (N * T)
    for name, flags in (("without", []), ("with", ["--ppo_target_kl", str(a.target_kl)])):
        L, ro = rollout(["--optimizer", "adam", "-lr", "0.001", "--e", "1e-5", "--ppo_epochs", "8"] + flags)
        curve, applied, seen = [], [], 0
        for tenth in range(10):
            for _ in range(cycles // 10 // 16):
                ro.run_cycles(16)
                if L.target_kl_on:
                    ro.synchronize()
                    applied.append(int(L.ppo_applied.sum().item()))
            ro.synchronize()
            count, episodes = ro.finished_episodes()
            new = episodes[max(0, len(episodes) - (count - seen)):]
            seen = count
            curve.append(round(float(np.mean([r for r, _ in new])), 3) if new else None)
        out[name] = dict(returns_by_tenth=curve, episodes=seen,
                         **(dict(mean_ppo_steps_applied=round(float(np.mean(applied)), 2)) if applied else {}))
        ro.close()
    return dict(steps=cycles // 160 * 160 * N * T, target_kl=a.target_kl, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("what", choices=["time", "learn"])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--steps", type=int, default=1536000)
    ap.add_argument("--target_kl", type=float, default=0.02)
    a = ap.parse_args()
    print(json.dumps({a.what: time_cycles(a) if a.what == "time" else learn(a)}))


if __name__ == "__main__":
    main()
