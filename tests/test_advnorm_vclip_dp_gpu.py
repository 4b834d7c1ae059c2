"""-m gpu: --adv_norm and --ppo_vclip under data parallelism (the pattern of test_ppo_dp_gpu.py).  Two gloo ranks on one GPU
run K = 3 with both flags: the replicas stay bit-identical and finite, and each rank's adv_n is the normalisation of ITS OWN
shard's advantages (no collective is added: the statistics differ between the ranks).  An RCCL world of one runs the exchange
captured into the cycle's graph -- which first passes the loop's replayed-against-eager check, with the new tensors in its
snapshot -- and must equal the single-process run bit for bit.  --adv_norm alone at K = 1 runs in the split exchange too."""
import os
import sys
import tempfile
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _learner(n_per_rank, T, K):
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    args = train.get_arg_parser().parse_args(["--ppo_epochs", str(K), "--ppo_clip", "0.1", "--gae_lambda", "0.95",
                                              "--adv_norm", "true", "--ppo_vclip", "0.05"])
    args.game, args.arch = "breakout", "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = n_per_rank, T, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_advnorm_dp_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    assert L.adv_norm and L.vclip_on == (K > 1)
    L.network.set_parameters(onet.init_params("NATURE", args.num_actions, np.random.RandomState(0), dtype=np.float32))
    return L, ec


def _record(L, ro):
    rec = {"state_" + n: t.cpu().numpy() for n, t in L.update_state}
    rec["adv"], rec["adv_n"], rec["adv_stats"] = ro.adv.cpu().numpy(), L.adv_n.cpu().numpy(), L.adv_stats.cpu().numpy()
    if L.ppo_stats is not None:
        rec["stats"] = L.ppo_stats.cpu().numpy()
    rec["global_step"] = np.int64(ro.global_step_dev.item())
    rec["exchange_mode"] = np.array(ro.exchange_mode)
    return rec


def _run(rank, world, port, out_dir, backend, mode, n_per_rank, T, cycles, use_graph, K):
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
    L, ec = _learner(n_per_rank, T, K)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * n_per_rank,
                       use_graph=use_graph)
    assert ro.phased
    for c in range(cycles):
        ro.run_cycle()
    ro.synchronize()
    assert ro.check_replicas("grad") and ro.check_replicas("weights")
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **_record(L, ro))
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


def _own_shard(r):
    from test_adv_norm import adv_norm_restated, ulps
    want, mean, std = adv_norm_restated(r["adv"])
    assert ulps(r["adv_n"], want).max() <= 1.0
    assert abs(r["adv_stats"][0] - mean) <= 1e-12 * abs(mean) and abs(r["adv_stats"][1] - std) <= 1e-12 * abs(std) and std > 0


@pytest.mark.parametrize("use_graph", [True, False])
def test_two_gloo_ranks_keep_identical_replicas_and_normalise_their_own_shards(tmp_path, use_graph):
    cycles, N, T, K = 3, 4, 7, 3
    _spawn(2, str(tmp_path), "gloo", "single", N, T, cycles, use_graph, K)
    r = [np.load(tmp_path / ("r%d.npz" % k)) for k in (0, 1)]
    for k in r[0].files:
        if k.startswith("state_"):
            assert np.array_equal(r[0][k], r[1][k]), k
    assert np.all(np.isfinite(r[0]["state_params"]))
    assert int(r[0]["global_step"]) == cycles * 2 * N * T                # once per cycle, all ranks' environments
    assert str(r[0]["exchange_mode"]) == "single"
    for k in (0, 1):
        _own_shard(r[k])
        assert r[k]["stats"].shape == (K, 3) and (r[k]["stats"][0] == 0).all() and np.abs(r[k]["stats"][1:, 1]).max() > 0
    assert not np.array_equal(r[0]["adv_stats"], r[1]["adv_stats"])      # per rank: no collective on the statistics


def _single_process(_, out_dir, N, T, cycles, K):
    sys.path.insert(0, ROOT)
    from paac_amd.paac import DeviceRollout
    L, ec = _learner(N, T, K)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=0, use_graph=True)
    assert not ro.phased
    for c in range(cycles):
        ro.run_cycle()
    ro.synchronize()
    np.savez(os.path.join(out_dir, "single.npz"), **_record(L, ro))
    ro.close()


@pytest.mark.parametrize("mode,K", [("graph", 3), ("single", 3), ("split", 1)])
def test_rccl_world_of_one_equals_the_single_process_run(tmp_path, mode, K):
    """The captured exchange (graph: it has passed the replayed-against-eager check, or exchange_mode would say single), the
    eager one between graph launches (single), and --adv_norm alone in the two-piece exchange (split, K = 1): one rank's sum
    is the gradient itself, so everything equals the run without collectives bit for bit."""
    import torch.multiprocessing as mp
    cycles, N, T = 3, 8, 5
    _spawn(1, str(tmp_path), "nccl", mode, N, T, cycles, True, K)
    mp.spawn(_single_process, args=(str(tmp_path), N, T, cycles, K), nprocs=1, join=True)
    dp, one = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "single.npz")
    assert str(dp["exchange_mode"]) == mode
    for k in one.files:
        if k != "exchange_mode":
            assert np.array_equal(dp[k], one[k]), k
    _own_shard(dp)
