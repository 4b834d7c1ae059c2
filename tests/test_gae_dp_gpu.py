"""-m gpu: --gae_lambda under data parallelism.  Two gloo ranks on one GPU (the pattern of test_adam_dp_gpu.py) run the
split cycle -- returns + heads / fc backward (phase 1), then the conv backward re-reading y / adv (phase 2): the replicas stay
bit-identical, and each rank's y / adv equal the single-process restatement (tests/test_gae.py) of that rank's own records.
Each rank is a child process of the spawn; the first failure ends the test."""
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDA = 0.9


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(rank, world, port, out_dir, n_per_rank, T, cycles):
    os.environ["PAAC_ALLREDUCE"] = "split"      # phase 1 computes the returns, the conv backward (phase 2) re-reads y / adv
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import DeviceRollout, PAACLearner
    args = train.get_arg_parser().parse_args(["--gae_lambda", str(LAMBDA)])
    args.game, args.arch = "breakout", "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = n_per_rank, T, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_gae_dp_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    assert L.gae_lambda == LAMBDA
    L.network.set_parameters(onet.init_params("NATURE", args.num_actions, np.random.RandomState(0), dtype=np.float32))
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * n_per_rank, use_graph=True)
    assert ro.phased
    rec = {}
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        B = T * n_per_rank
        rec.update({"v_boot%d" % c: L.ctx.debug_activation(25, B + n_per_rank)[B:].cpu().numpy(),
                    "rewards%d" % c: ro.rewards.cpu().numpy(), "masks%d" % c: ro.masks.cpu().numpy(),
                    "values%d" % c: ro.values.cpu().numpy(), "y%d" % c: ro.y.cpu().numpy(), "adv%d" % c: ro.adv.cpu().numpy()})
    assert ro.check_replicas("grad") and ro.check_replicas("weights")
    rec.update({"state_" + n: t.cpu().numpy() for n, t in L.update_state})
    rec["gamma"] = np.float64(L.gamma)
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **rec)
    ro.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_identical_replicas_with_gae(tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gae import gae_restated
    cycles, N, T = 3, 4, 7
    procs = mp.spawn(_run, args=(2, _free_port(), str(tmp_path), N, T, cycles), nprocs=2, join=False)
    deadline = time.time() + 600
    try:
        while not procs.join(timeout=5):         # raises as soon as one rank has failed (and ends the other)
            assert time.time() < deadline, "the ranks did not finish within 600 s"
    finally:
        for proc in procs.processes:
            if proc.is_alive():
                proc.kill()
    r = [np.load(tmp_path / ("r%d.npz" % k)) for k in (0, 1)]
    for k in r[0].files:
        if k.startswith("state_"):
            assert np.array_equal(r[0][k], r[1][k]), k
    assert np.all(np.isfinite(r[0]["state_params"]))
    for rank in (0, 1):
        for c in range(cycles):
            g = lambda name: r[rank]["%s%d" % (name, c)]
            ye, ae = gae_restated(g("v_boot"), g("rewards"), g("masks"), g("values"), float(r[rank]["gamma"]), LAMBDA)
            assert np.array_equal(g("y"), ye.reshape(-1)), (rank, c)
            assert np.array_equal(g("adv"), ae.reshape(-1)), (rank, c)
    assert not np.array_equal(r[0]["rewards0"], r[1]["rewards0"]) or not np.array_equal(r[0]["values0"], r[1]["values0"])
