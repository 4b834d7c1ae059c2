"""What --explore_bonus adds to a cycle: the device loop on catch at the default shape (32 environments, T = 5, NIPS) through
the captured graphs, the flag off / on / off / on in one process; per run three timed batches of --cycles cycles behind --warm
warm-up cycles, each ended by a synchronisation.  One JSON line per run: microseconds per cycle of each batch."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import train  # noqa: E402
from paac_amd.paac import DeviceRollout, PAACLearner  # noqa: E402


def run(beta, cycles, warm):
    args = train.get_arg_parser().parse_args(["--emulator", "catch", "--explore_bonus", beta])
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_explore_")
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
    ap.add_argument("--cycles", type=int, default=3000)
    ap.add_argument("--warm", type=int, default=400)
    a = ap.parse_args()
    for beta in ("0", "0.1", "0", "0.1"):
        print(json.dumps(dict(explore_bonus=beta, us_per_cycle=run(beta, a.cycles, a.warm))), flush=True)
