"""-m gpu: --optimizer adam under data parallelism.  Two gloo ranks on one GPU (the pattern of test_dp_gpu.py) keep
bit-identical replicas -- weights, moments and bias-correction powers -- and a world of one under RCCL with the all-reduce
captured into the cycle graph passes the replay-vs-eager check, which must restore the powers it advanced."""
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _chain(beta, length):
    p = np.float32(beta)
    for _ in range(length - 1):
        p = np.float32(p * np.float32(beta))
    return p


def _run(rank, world, port, out_dir, n_per_rank, cycles):
    os.environ["PAAC_ALLREDUCE"] = "single"
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import DeviceRollout, PAACLearner
    args = train.get_arg_parser().parse_args(["--optimizer", "adam", "--beta1", "0.8", "--beta2", "0.99"])
    args.game, args.arch = "breakout", "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = n_per_rank, 3, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_adam_dp_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    L.network.set_parameters(onet.init_params("NATURE", args.num_actions, np.random.RandomState(0), dtype=np.float32))
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * n_per_rank, use_graph=True)
    assert ro.phased
    ro.run_cycle()
    ro.run_cycles(cycles - 1)       # back to back: the optimizer step rides in front of the next cycle
    ro.synchronize()
    assert ro.check_replicas("grad") and ro.check_replicas("weights")
    names = [n for n, _ in L.update_state]
    assert names == ["params", "m", "v", "beta_powers"], names
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **{n: t.cpu().numpy() for n, t in L.update_state})
    ro.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_identical_adam_replicas(tmp_path):
    import torch.multiprocessing as mp
    cycles = 5
    mp.spawn(_run, args=(2, _free_port(), str(tmp_path), 4, cycles), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k]), k
    assert np.array_equal(r0["beta_powers"], np.array([_chain(0.8, cycles + 1), _chain(0.99, cycles + 1)]))
    assert np.any(r0["m"]) and np.all(np.isfinite(r0["params"]))


_GRAPH_EXCHANGE = r"""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, %(root)r)
from paac_amd import parallel, train
args = train.get_arg_parser().parse_args(["--optimizer", "adam", "--beta1", "0.8", "--beta2", "0.99", "--e", "1e-3"])
assert parallel.init_from_env(args) == 1
import torch
from paac_amd.paac import DeviceRollout, PAACLearner
args.game, args.arch = "breakout", "NATURE"
args.emulator_counts, args.max_local_steps, args.emulator_workers = 8, 5, 0
args.max_global_steps = 1 << 40
args.synthetic_terminal_p = 0.1
out = {}
for mode in ("plain", "graph"):
    os.environ["PAAC_FORCE_COLLECTIVES"] = "0" if mode == "plain" else "1"
    os.environ["PAAC_ALLREDUCE"] = "graph" if mode == "graph" else "single"
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_adam_graph_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    L.network.initialize(np.random.RandomState(0))
    np.random.seed(4)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="numpy", use_graph=True)
    checked = []
    if mode == "graph":
        inner = ro._replay_matches_eager
        ro._replay_matches_eager = lambda: checked.append(inner()) or checked[-1]
    ro.run_cycles(7)
    ro.synchronize()
    out[mode] = [t.cpu().numpy().copy() for _, t in L.update_state]
    if mode == "graph":
        assert ro.graph_exchange and checked == [True] and ro.exchange_fallback is None, (checked, ro.exchange_fallback)
        assert ro.check_replicas("weights")
    ro.close()
p = out["graph"][3]
c1, c2 = np.float32(0.8), np.float32(0.99)
w1, w2 = c1, c2
for _ in range(7):
    w1, w2 = np.float32(w1 * c1), np.float32(w2 * c2)
assert p[0] == w1 and p[1] == w2, (p, w1, w2)        # 7 real updates: the two checked cycles left no trace
for a, b in zip(out["graph"], out["plain"]):
    assert np.array_equal(a, b)
parallel.shutdown()
print("ADAM_GRAPH_EXCHANGE_OK")
"""


def test_graph_exchange_replay_check_restores_the_powers():
    """PAAC_ALLREDUCE=graph under RCCL, a world of one with the collectives forced on: the replay-vs-eager check runs a
    cycle eagerly and replayed from one snapshot (DeviceRollout._cycle_state); afterwards the powers must be the chain of
    the real updates only, and everything equal the unphased run bit for bit."""
    env = dict(os.environ, PAAC_DIST_FORCE="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(_free_port()))
    res = subprocess.run([sys.executable, "-c", _GRAPH_EXCHANGE % dict(root=ROOT)], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and "ADAM_GRAPH_EXCHANGE_OK" in res.stdout, (res.stdout[-1500:], res.stderr[-3000:])
