"""-m gpu: --ppo_epochs under data parallelism, one all-reduce per epoch.  Two gloo ranks on one GPU (the pattern of
test_gae_dp_gpu.py) run K = 3 with the exchange issued eagerly between graph launches (the pending-update arrangement): the
replicas stay bit-identical and finite.  An RCCL world of one runs the exchange captured into the cycle's graph (which first
passes the loop's own replayed-against-eager check) and, with one rank, must equal the single-process run bit for bit.
PAAC_ALLREDUCE=split is refused at construction.  Each rank is a child process of the spawn; the first failure ends the test."""
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
K = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _learner(n_per_rank, T, optimizer="rmsprop"):
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    args = train.get_arg_parser().parse_args(["--ppo_epochs", str(K), "--ppo_clip", "0.1", "--gae_lambda", "0.95",
                                              "--optimizer", optimizer])
    args.game, args.arch = "breakout", "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = n_per_rank, T, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_ppo_dp_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    assert L.ppo_epochs == K
    L.network.set_parameters(onet.init_params("NATURE", args.num_actions, np.random.RandomState(0), dtype=np.float32))
    return L, ec


def _run(rank, world, port, out_dir, backend, mode, n_per_rank, T, cycles, use_graph):
    os.environ["PAAC_ALLREDUCE"] = mode
    if world == 1:
        os.environ["PAAC_FORCE_COLLECTIVES"] = "1"       # a world of one still issues the stream-ordered all-reduce calls
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "nccl":
        torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    from paac_amd.paac import DeviceRollout
    L, ec = _learner(n_per_rank, T)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * n_per_rank,
                       use_graph=use_graph)
    assert ro.phased
    for c in range(cycles):
        ro.run_cycle()
    ro.synchronize()
    assert ro.check_replicas("grad") and ro.check_replicas("weights")
    rec = {"state_" + n: t.cpu().numpy() for n, t in L.update_state}
    rec["stats"] = L.ppo_stats.cpu().numpy()
    rec["global_step"] = np.int64(ro.global_step_dev.item())
    rec["exchange_mode"] = np.array(ro.exchange_mode)
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **rec)
    ro.close()
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, *args):
    import torch.multiprocessing as mp
    procs = mp.spawn(_run, args=(world, _free_port()) + args, nprocs=world, join=False)
    deadline = time.time() + 600
    try:
        while not procs.join(timeout=5):         # raises as soon as one rank has failed (and ends the other)
            assert time.time() < deadline, "the ranks did not finish within 600 s"
    finally:
        for proc in procs.processes:
            if proc.is_alive():
                proc.kill()


@pytest.mark.parametrize("use_graph", [True, False])
def test_two_gloo_ranks_keep_identical_replicas_over_three_epochs(tmp_path, use_graph):
    cycles, N, T = 3, 4, 7
    _spawn(2, str(tmp_path), "gloo", "single", N, T, cycles, use_graph)
    r = [np.load(tmp_path / ("r%d.npz" % k)) for k in (0, 1)]
    for k in r[0].files:
        if k.startswith("state_"):
            assert np.array_equal(r[0][k], r[1][k]), k
    assert np.all(np.isfinite(r[0]["state_params"]))
    assert int(r[0]["global_step"]) == cycles * 2 * N * T                # once per cycle, all ranks' environments
    assert str(r[0]["exchange_mode"]) == "single"
    for k in (0, 1):                                                     # each rank's own rows: epochs 2, 3 moved the policy
        assert (r[k]["stats"][0] == 0).all() and np.abs(r[k]["stats"][1:, 1]).max() > 0


def _single_process(_, out_dir, N, T, cycles):
    sys.path.insert(0, ROOT)
    from paac_amd.paac import DeviceRollout
    L, ec = _learner(N, T)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=0, use_graph=True)
    assert not ro.phased
    for c in range(cycles):
        ro.run_cycle()
    ro.synchronize()
    np.savez(os.path.join(out_dir, "single.npz"), **{"state_" + n: t.cpu().numpy() for n, t in L.update_state})
    ro.close()


@pytest.mark.parametrize("mode", ["graph", "single"])
def test_rccl_world_of_one_equals_the_single_process_run(tmp_path, mode):
    """The captured exchange (graph) and the eager one between graph launches (single), one rank: the sum over one rank is the
    gradient itself and grad_scale is 1, so weights and optimizer slots equal the run without collectives bit for bit -- except
    that run's phase-3 backward, whose slab reduction the optimizer step performs in the same order (include/paac_hip.h)."""
    import torch.multiprocessing as mp
    cycles, N, T = 3, 8, 5
    _spawn(1, str(tmp_path), "nccl", mode, N, T, cycles, True)
    mp.spawn(_single_process, args=(str(tmp_path), N, T, cycles), nprocs=1, join=True)
    dp, one = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "single.npz")
    assert str(dp["exchange_mode"]) == mode
    for k in one.files:
        assert np.array_equal(dp[k], one[k]), k


def test_split_exchange_is_refused_at_construction(monkeypatch):
    import torch.multiprocessing as mp
    with pytest.raises(Exception, match="ppo_epochs above 1 is not built for PAAC_ALLREDUCE=split"):
        mp.spawn(_run, args=(1, _free_port(), tempfile.mkdtemp(), "gloo", "split", 4, 5, 1, True), nprocs=1, join=True)
