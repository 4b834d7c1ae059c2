"""-m gpu: --ppo_minibatches under data parallelism, one all-reduce per optimizer step (K * M per cycle).  Two gloo ranks on one
GPU (the pattern of test_ppo_dp_gpu.py) run K = 2, M = 2 with the exchange issued eagerly between graph launches: every rank
draws the same permutation (nothing rank-specific enters the counter) and applies it to its own shard, the replicas stay
bit-identical and finite.  An RCCL world of one runs the exchange captured into the cycle's graph, which first passes the loop's
own replayed-against-eager check.  PAAC_ALLREDUCE=split is refused at construction with a message naming the flag.  Each rank is
a child process of the spawn; the first failure ends the test."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
K, M = 2, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _learner(n_per_rank, T):
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    args = train.get_arg_parser().parse_args(["--ppo_epochs", str(K), "--ppo_minibatches", str(M), "--ppo_clip", "0.1",
                                              "--gae_lambda", "0.95"])
    args.game, args.arch = "breakout", "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = n_per_rank, T, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_mb_dp_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    assert L.minibatch_on and L.ppo_steps == K * M
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
    from paac_amd import parallel
    from paac_amd.paac import DeviceRollout
    L, ec = _learner(n_per_rank, T)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * n_per_rank,
                       use_graph=use_graph)
    assert ro.phased
    exchanges = [0]
    plain = parallel.allreduce_sum_

    def counted(t, *a, **kw):
        if t.data_ptr() == L.grad.data_ptr():
            exchanges[0] += 1
        return plain(t, *a, **kw)

    for c in range(cycles):
        if c == cycles - 1 and not ro.graph_exchange:    # the eager exchange: count one cycle's all-reduces of the gradient
            ro.synchronize()
            parallel.allreduce_sum_ = counted
        ro.run_cycle()
    parallel.allreduce_sum_ = plain
    ro.synchronize()
    assert ro.check_replicas("grad") and ro.check_replicas("weights")
    rec = {"state_" + n: t.cpu().numpy() for n, t in L.update_state}
    rec["stats"] = L.ppo_stats.cpu().numpy()
    rec["perms"] = L.mb["perms"].cpu().numpy()
    rec["actions"] = ro.actions.cpu().numpy()
    rec["exchanges"] = np.int64(exchanges[0])
    rec["global_step"] = np.int64(ro.global_step_dev.item())
    rec["exchange_mode"] = np.array(ro.exchange_mode)
    rec["fallback"] = np.array(str(ro.exchange_fallback))
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
def test_two_gloo_ranks_keep_identical_replicas(tmp_path, use_graph):
    from test_ppo_minibatch import FIRST_STEP_KL, perms_restated
    cycles, N, T = 3, 4, 6
    _spawn(2, str(tmp_path), "gloo", "single", N, T, cycles, use_graph)
    r = [np.load(tmp_path / ("r%d.npz" % k)) for k in (0, 1)]
    for k in r[0].files:
        if k.startswith("state_"):
            assert np.array_equal(r[0][k], r[1][k]), k
    assert np.all(np.isfinite(r[0]["state_params"]))
    assert int(r[0]["global_step"]) == cycles * 2 * N * T                # once per cycle, all ranks' environments
    assert str(r[0]["exchange_mode"]) == "single"
    # the same permutation on every rank (the restatement's for the last cycle's frame counter), applied to different shards
    assert np.array_equal(r[0]["perms"], r[1]["perms"])
    assert np.array_equal(r[0]["perms"], perms_restated(N * T, K, 9, cycles * T))
    assert not np.array_equal(r[0]["actions"], r[1]["actions"])
    for k in (0, 1):
        assert int(r[k]["exchanges"]) == K * M                           # one all-reduce per optimizer step
        assert r[k]["stats"].shape == (K * M, 2) and np.abs(r[k]["stats"][1:, 1]).max() > 0
        assert r[k]["stats"][0, 0] == 0 and abs(r[k]["stats"][0, 1]) < FIRST_STEP_KL       # (kept acting rows: test_ppo_minibatch.py)


def test_rccl_world_of_one_replays_the_captured_exchange(tmp_path):
    """PAAC_ALLREDUCE=graph: the K * M all-reduces are captured into the cycle's graph, and the loop's own check -- the same
    cycle once with the eager exchange and once replayed, the last step's exchanged gradients bit for bit -- has passed
    (a failed check falls back to `single` and names the reason)."""
    cycles, N, T = 3, 8, 5
    _spawn(1, str(tmp_path), "nccl", "graph", N, T, cycles, True)
    dp = np.load(tmp_path / "r0.npz")
    assert str(dp["exchange_mode"]) == "graph", str(dp["fallback"])
    assert np.all(np.isfinite(dp["state_params"])) and np.abs(dp["stats"][1:, 1]).max() > 0


def test_split_exchange_is_refused_naming_the_flag():
    import torch.multiprocessing as mp
    with pytest.raises(Exception, match="ppo_minibatches above 1 is not built for PAAC_ALLREDUCE=split"):
        mp.spawn(_run, args=(1, _free_port(), tempfile.mkdtemp(), "gloo", "split", 4, 5, 1, True), nprocs=1, join=True)
