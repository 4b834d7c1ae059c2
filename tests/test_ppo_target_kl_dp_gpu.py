"""-m gpu: --ppo_target_kl under data parallelism.  The value the gate compares is the mean of the ranks' approx_kl; it
travels behind the gradient through the step's one all-reduce, so every rank takes the same decision from the same bits.
Two gloo ranks on one GPU (the form of test_ppo_dp_gpu.py, no more processes than it uses): the gated run stops where
(a + b) * 0.5f says, on both ranks, the replicas stay identical and the weights are the two-rank --ppo_epochs j run's.  An
RCCL world of one runs the gate inside the captured exchange, behind the loop's own replayed-against-eager check."""
import os
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, N, T = 4, 8, 5
# approx_kl over 40 rows is a noisy estimate of either sign; at the default learning rate (0.0224) the first cycle's values
# from this start are all negative, and a negative value never stops a cycle.  At 0.3 the policy moves far enough that
# the mean of the two shards rises above zero inside the cycle.
LR = 0.3


def _learner(**flags):
    from oracle import network as onet
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    args = train.get_arg_parser().parse_args(["--ppo_clip", "0.2", "-lr", str(LR)])
    args.game, args.arch = "pong", "NIPS"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = N, T, 0
    args.max_global_steps = 1 << 40
    args.synthetic_terminal_p = 0.1
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_target_kl_dp_")
    for k, v in flags.items():
        setattr(args, k, v)
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    L.network.set_parameters(onet.init_params("NIPS", args.num_actions, np.random.RandomState(0), dtype=np.float32))
    return L, ec


def _cycles(rank, use_graph, cycles, **flags):
    """Fresh learner and rollout from the fixed start, `cycles` cycles -> (state arrays, stats, applied, checked, rollout facts)."""
    from paac_amd.paac import DeviceRollout
    L, ec = _learner(**flags)
    ro = DeviceRollout(L, ec.device_env_spec, sampler="philox", sampler_seed=9, env_offset=rank * N, use_graph=use_graph)
    assert ro.phased and L.kl_in_store == L.target_kl_on
    assert L.grad_store.numel() == L.grad.numel() + (4 if L.target_kl_on else 0) and L.grad.data_ptr() == L.grad_store.data_ptr()
    out = []
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        assert ro.check_replicas("grad") and ro.check_replicas("weights")
        out.append(dict(state=[t.cpu().numpy().copy() for _, t in L.update_state], stats=L.ppo_stats.cpu().numpy().copy()
                        if L.ppo_stats is not None else None,
                        applied=L.ppo_applied.cpu().numpy().copy() if L.target_kl_on else None,
                        checked=L.ppo_kl_checked.cpu().numpy().copy() if L.target_kl_on else None))
    facts = dict(mode=ro.exchange_mode, fallback=ro.exchange_fallback)
    ro.close()
    return out, facts


def _run(rank, world, port, out_dir, backend, use_graph):
    os.environ["PAAC_ALLREDUCE"] = "graph" if backend == "nccl" else "single"
    if world == 1:
        os.environ["PAAC_DIST_FORCE"] = "1"
        os.environ["PAAC_FORCE_COLLECTIVES"] = "1"       # a world of one still issues the stream-ordered all-reduce calls
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from test_ppo_target_kl_gpu import stop_positions
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if backend == "nccl":
        torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    # the ranks' KL rows from an ungated cycle
    free, facts = _cycles(rank, use_graph, 1, ppo_epochs=K)
    own = torch.from_numpy(free[0]["stats"][:, 1].copy())
    rows = [torch.zeros_like(own) for _ in range(world)]
    if backend == "nccl":
        rows = [own]
    else:
        dist.all_gather(rows, own)
    rows = [r.numpy() for r in rows]
    mean = rows[0] if world == 1 else (rows[0] + rows[1]) * np.float32(0.5)
    assert mean.dtype == np.float32
    if world == 2:
        assert not np.array_equal(rows[0][1:], rows[1][1:])          # the shards differ: neither rank's own value decides
    positions = stop_positions(mean, 1)
    print("rank %d: approx_kl rows %s, mean %s, stop positions %s" % (rank, [r.tolist() for r in rows], mean.tolist(), positions),
          flush=True)
    assert positions, mean
    j, D = positions[-1]
    gated, gfacts = _cycles(rank, use_graph, 2, ppo_epochs=K, ppo_target_kl=D)
    short, _ = _cycles(rank, use_graph, 1, ppo_epochs=j)
    rec = {"gated_%d" % i: a for i, a in enumerate(gated[0]["state"])}
    rec.update({"short_%d" % i: a for i, a in enumerate(short[0]["state"])})
    rec.update({"free_%d" % i: a for i, a in enumerate(free[0]["state"])})
    rec.update(mean=mean, j=np.int64(j), applied=gated[0]["applied"], checked=gated[0]["checked"], applied2=gated[1]["applied"],
               mode=np.array(gfacts["mode"]), fallback=np.array(str(gfacts["fallback"])), free_mode=np.array(facts["mode"]))
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **rec)
    dist.barrier()
    dist.destroy_process_group()


def _check_rank(r):
    j = int(r["j"])
    assert 1 <= j < K
    assert r["applied"].tolist() == [1] * j + [0] * (K - j), (j, r["applied"], r["mean"])
    assert np.array_equal(r["checked"][1:j + 1], r["mean"][1:j + 1])
    n = len([k for k in r.files if k.startswith("gated_")])
    assert n >= 3
    for i in range(n):
        assert np.array_equal(r["gated_%d" % i], r["short_%d" % i]), i
    assert not np.array_equal(r["gated_0"], r["free_0"]) and np.isfinite(r["gated_0"]).all()
    a2 = r["applied2"]
    assert a2[0] == 1 and (np.diff(a2) <= 0).all()       # the next cycle cleared the flag (step 0 is never gated)


@pytest.mark.parametrize("use_graph", [True, False])
def test_two_gloo_ranks_stop_where_the_mean_says(tmp_path, use_graph):
    _spawn(2, str(tmp_path), "gloo", use_graph)
    r = [np.load(tmp_path / ("r%d.npz" % k)) for k in (0, 1)]
    assert np.array_equal(r[0]["mean"], r[1]["mean"]) and int(r[0]["j"]) == int(r[1]["j"])
    for k in (0, 1):
        _check_rank(r[k])
        assert str(r[k]["mode"]) == "single"
    for key in r[0].files:
        if key.startswith("gated_"):
            assert np.array_equal(r[0][key], r[1][key]), key
    assert np.array_equal(r[0]["applied"], r[1]["applied"]) and np.array_equal(r[0]["checked"], r[1]["checked"])
    assert np.array_equal(r[0]["applied2"], r[1]["applied2"])


def test_rccl_world_of_one_gates_inside_the_captured_exchange(tmp_path):
    _spawn(1, str(tmp_path), "nccl", True)
    r = np.load(tmp_path / "r0.npz")
    assert str(r["mode"]) == "graph" and str(r["fallback"]) == "None", (r["mode"], r["fallback"])
    assert str(r["free_mode"]) == "graph"
    _check_rank(r)


def _spawn(world, *args):
    """test_ppo_dp_gpu._spawn around this module's _run: the first failure ends the test, nothing is left running."""
    import time
    import torch.multiprocessing as mp
    from test_ppo_dp_gpu import _free_port
    procs = mp.spawn(_run, args=(world, _free_port()) + args, nprocs=world, join=False)
    deadline = time.time() + 600
    try:
        while not procs.join(timeout=5):
            assert time.time() < deadline, "the ranks did not finish within 600 s"
    finally:
        for proc in procs.processes:
            if proc.is_alive():
                proc.kill()
