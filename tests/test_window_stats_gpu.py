"""-m gpu: --window_stats (spec and twin: paac_amd/window_stats.py; contract: include/paac_hip.h, paac_window_fold).  The entry
against the twin, its refusals, the device loop's block (eager, captured), training with the flag on against off, a real
run's records, the host loop.

Acceptance of a block against the twin's (`assert_block`): integer fields and the min / max fields bit for bit; every float64
sum within n * 2^-52 * sum|term|, n the number of terms folded so far -- float64 rounding alone (the twin states the kernel's
order, so the two normally agree to the bit; a fused multiply-add on an inexact square is the one difference that bound
allows)."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from paac_amd import window_stats as ws
from test_window_stats import RING_WORDS, make_cycle

EXACT_F = ("max_abs_adv", "max_grad_norm", "ep_return_min", "ep_return_max", "ep_length_min", "ep_length_max")


class Bounds(object):
    """Per float64 sum of the block: the number of terms folded so far and the sum of their magnitudes."""

    def __init__(self):
        self.n = np.zeros(ws.N_F)
        self.mag = np.zeros(ws.N_F)

    def bump(self, name, terms, column=0):
        at = ws.FIELDS_F[name][0] + column
        terms = np.asarray(terms, dtype=np.float64).reshape(-1)
        self.n[at] += terms.size
        self.mag[at] += np.abs(terms).sum()

    def cycle(self, cycle, cursor):
        f64 = lambda k: np.asarray(cycle[k], dtype=np.float32).astype(np.float64).reshape(-1)
        v, y, adv, r = f64("values"), f64("y"), f64("adv"), f64("rewards")
        d = y - v
        for name, terms in zip(ws.ROW_SUMS, (v, v * v, y, y * y, d, d * d, adv, adv * adv, r)):
            self.bump(name, terms)
        loss = np.array(cycle["loss"], dtype=np.float32).reshape(-1, 4)
        if cycle.get("loss0") is not None:
            loss[0] = cycle["loss0"]
        for c in range(4):
            self.bump("sum_loss", loss[:, c], c)
        if cycle.get("ppo_stats") is not None:
            stats = np.asarray(cycle["ppo_stats"])
            for c in range(stats.shape[1]):
                self.bump("sum_stats", stats[cycle.get("stats_first", 0):, c], c)
        self.bump("sum_grad_norm", cycle["gnorm"])
        if cycle.get("ring") is not None:
            _, _, returns, lengths = ws.ring_entries(cycle["ring"], cursor)
            self.episodes(returns, lengths)

    def episodes(self, returns, lengths):
        r, n = np.asarray(returns, dtype=np.float64), np.asarray(lengths, dtype=np.float64)
        for name, terms in zip(ws.EPISODE_SUMS, (r, r * r, n, n * n)):
            self.bump(name, terms)


def assert_block(acc_f, acc_i, twin, bounds, what=""):
    got_f = acc_f.cpu().numpy() if isinstance(acc_f, torch.Tensor) else np.asarray(acc_f)
    got_i = acc_i.cpu().numpy() if isinstance(acc_i, torch.Tensor) else np.asarray(acc_i)
    assert got_f.shape == (ws.N_F,) and got_i.shape == (ws.N_I,)
    assert np.array_equal(got_i, twin.i), (what, got_i, twin.i)
    exact = np.zeros(ws.N_F, dtype=bool)
    for name in EXACT_F:
        exact[ws.FIELDS_F[name][0]] = True
    assert np.array_equal(got_f[exact], twin.f[exact]), (what, got_f[exact], twin.f[exact])
    delta, allowed = np.abs(got_f - twin.f)[~exact], (bounds.n * 2.0 ** -52 * bounds.mag)[~exact]
    print(what, "largest |delta| / allowed:", float(np.max(delta / np.maximum(allowed, 1e-300))), "largest |delta|:", float(delta.max()))
    assert (delta <= allowed).all(), (what, delta, allowed)


def to_device(cycle):
    dev = {}
    for k, v in cycle.items():
        dev[k] = torch.from_numpy(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v
    return dev


def device_fold(acc_f, acc_i, dev):
    from paac_amd import hip_ops
    hip_ops.window_fold(acc_f, acc_i, dev["values"], dev["rewards"], dev["masks"], dev["actions"], dev["y"], dev["adv"], dev["A"],
                        loss=dev["loss"], gnorm=dev["gnorm"], truncs=dev["truncs"], loss0=dev["loss0"], ppo_stats=dev["ppo_stats"],
                        stats_first=dev["stats_first"], applied=dev["applied"], finished=dev["ring"])
    torch.cuda.synchronize()


def random_ring(rs, count):
    ring = np.zeros(RING_WORDS, dtype=np.int32)
    ring[0] = count
    ring[2:2 + ws.RING].view(np.float32)[:] = (rs.randn(ws.RING) * 5).astype(np.float32)
    ring[2 + ws.RING:] = rs.randint(1, 1000, ws.RING)
    return ring


def advance_ring(rs, ring, new):
    ring = ring.copy()
    count = int(ring[0])
    slots = (count + np.arange(new)) & (ws.RING - 1)
    ring[2:2 + ws.RING].view(np.float32)[slots] = (rs.randn(new) * 5).astype(np.float32)
    ring[2 + ws.RING:][slots] = rs.randint(1, 1000, new)
    ring[0] = count + new
    return ring


# (N, T, A, truncs, steps, stats_cols, stats_first, loss0, ring: None or (cursor, count, new entries before folds 2 and 3))
ENTRY_CASES = {
    "6rows_A3_plain": (3, 2, 3, False, 1, 0, 0, False, None),
    "6rows_A18_truncs_wrap": (3, 2, 18, True, 1, 0, 0, False, (4090, 4100, (7, 0))),
    "260rows_A18_truncs_6steps_gated_wrap": (52, 5, 18, True, 6, 3, 0, False, (4090, 4100, (7, 0))),
    "260rows_A3_6steps_fullbatch_dropped": (52, 5, 3, False, 6, 2, 1, True, (1000, 6000, (5, ws.RING + 3))),
}


@pytest.mark.parametrize("case", sorted(ENTRY_CASES))
def test_entry_equals_the_twin_over_three_folds(case):
    from paac_amd import hip_ops
    N, T, A, truncs, steps, cols, first, loss0, ring_plan = ENTRY_CASES[case]
    rs = np.random.RandomState(len(case))
    assert hip_ops.window_fields() == (ws.N_F, ws.N_I)
    acc_f, acc_i = hip_ops.window_block("cuda")
    twin, bounds = ws.Block(), Bounds()
    ring = None
    if ring_plan is not None:
        cursor, count, later = ring_plan
        ring = random_ring(rs, count)
        twin.set("ring_cursor", cursor)
        acc_i[ws.FIELDS_I["ring_cursor"][0]] = cursor
    applied = np.array([1, 1, 0, 0, 0, 0], dtype=np.int32) if (steps == 6 and cols == 3) else None
    for k in range(3):
        if ring is not None and k > 0:
            ring = advance_ring(rs, ring, later[k - 1])
        cycle = make_cycle(rs, T, N, A, steps=steps, truncs=truncs, stats_cols=cols, stats_first=first, applied=applied, ring=ring,
                           loss0=loss0)
        bounds.cycle(cycle, twin.get("ring_cursor"))
        ws.fold(twin, cycle)
        device_fold(acc_f, acc_i, to_device(cycle))
        assert_block(acc_f, acc_i, twin, bounds, "%s fold %d" % (case, k + 1))
    assert twin.get("cycles") == 3 and twin.get("rows") == 3 * N * T
    if case.endswith("dropped"):
        assert twin.get("episodes_dropped") == (5000 - ws.RING) + 3 and twin.get("episodes") == 2 * ws.RING + 5
    if case.endswith("wrap"):
        assert twin.get("episodes") == 17 and twin.get("ring_cursor") == 4107


def test_every_refusal_names_its_argument_and_launches_nothing():
    from paac_amd import _lib, hip_ops
    lib = _lib.load()
    rs = np.random.RandomState(1)
    dev = to_device(make_cycle(rs, 2, 3, 3, steps=2, stats_cols=2))
    acc_f, acc_i = hip_ops.window_block("cuda")
    device_fold(acc_f, acc_i, dev)                         # a block that is not all zeros
    before = (acc_f.clone(), acc_i.clone())
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def inputs(**changes):
        fields = dict(T=2, N=3, A=3, values=p(dev["values"]), rewards=p(dev["rewards"]), masks=p(dev["masks"]),
                      actions=p(dev["actions"]), y=p(dev["y"]), adv=p(dev["adv"]), truncs=None, loss=p(dev["loss"]), loss0=None,
                      steps=2, ppo_stats=p(dev["ppo_stats"]), stats_cols=2, stats_first=0, applied=None, gnorm=p(dev["gnorm"]),
                      finished=None)
        fields.update(changes)
        return _lib.WindowInputs(**fields)

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(block, f=acc_f, i=acc_i):
        rc = lib.paac_window_fold(ctypes.byref(block) if block is not None else None, p(f) if f is not None else None,
                                  p(i) if i is not None else None, stream)
        torch.cuda.synchronize()
        assert rc < 0
        assert torch.equal(acc_f, before[0]) and torch.equal(acc_i, before[1])
        return lib.paac_last_error().decode()

    assert lib.paac_window_fold(ctypes.byref(inputs()), p(acc_f), p(acc_i), stream) == 0      # the unchanged block is accepted
    torch.cuda.synchronize()
    before = (acc_f.clone(), acc_i.clone())
    assert "in is null" in refused(None)
    assert "acc_f is null" in refused(inputs(), f=None)
    assert "acc_i is null" in refused(inputs(), i=None)
    for name in ("values", "rewards", "masks", "actions", "y", "adv", "loss", "gnorm"):
        assert "%s is null" % name in refused(inputs(**{name: None})), name
    assert "T=0" in refused(inputs(T=0)) and "N=-1" in refused(inputs(N=-1))
    assert "A=1 " in refused(inputs(A=1)) and "A=33 " in refused(inputs(A=33))
    assert "steps=0 " in refused(inputs(steps=0)) and "steps=65 " in refused(inputs(steps=65))
    assert "stats_cols=4" in refused(inputs(stats_cols=4)) and "stats_first=3" in refused(inputs(stats_first=3))
    # ... and the wrapper's own checks come before the library's
    bad = dict(dev, rewards=dev["rewards"][:1])
    with pytest.raises(ValueError, match="rewards must be"):
        device_fold(acc_f, acc_i, bad)
    with pytest.raises(ValueError, match="dtype"):
        device_fold(acc_f, acc_i, dict(dev, actions=dev["actions"].to(torch.int64)))
    with pytest.raises(ValueError, match="loss must be"):
        device_fold(acc_f, acc_i, dict(dev, loss=dev["loss"].view(-1)))
    assert torch.equal(acc_f, before[0]) and torch.equal(acc_i, before[1])


# -- the device loop -----------------------------------------------------------------------------------------------------

N, T = 4, 5


def catch_args(argv=(), **kw):
    import tempfile
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "catch", "--arch", "NIPS"] + list(argv))
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_windowtest_")
    args.emulator_workers = 0
    for k, v in dict(dict(emulator_counts=N, max_local_steps=T, max_global_steps=1 << 40), **kw).items():
        setattr(args, k, v)
    return args


def seeded_learner(args):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(0))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner, env_creator


def read_cycle(L, ro):
    """What the fold of the cycle that has just run read, copied to the host."""
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    ppo = L.ppo_epochs > 1
    return dict(T=ro.T, N=ro.N, A=ro.A, values=host(ro.values), rewards=host(ro.rewards), masks=host(ro.masks),
                actions=host(ro.actions), y=host(ro.y), adv=host(ro.adv), truncs=host(ro.truncs),
                loss=host(L.ppo_loss) if ppo else host(L.loss_dev).reshape(1, 4),
                loss0=host(L.loss_dev) if ppo and not L.minibatch_on else None, ppo_stats=host(L.ppo_stats) if ppo else None,
                stats_first=0 if L.minibatch_on else 1, applied=host(L.ppo_applied), gnorm=host(L.gnorm_dev), ring=host(ro.finished))


def device_blocks(sampler, cycles=6, **flags):
    """`cycles` cycles of the device loop on catch with the flag on, eagerly (the twin folded over each cycle's own tensors,
    read back) and captured -> (eager block, twin, bounds, captured block, the eager run's cycles)."""
    from paac_amd.paac import DeviceRollout
    out = []
    for use_graph in (False, True):
        L, env_creator = seeded_learner(catch_args(["--window_stats", "true"], sampler=sampler, **flags))
        np.random.seed(11)
        L.global_step = L.init_network()
        ro = DeviceRollout(L, env_creator.device_env_spec, sampler=sampler, sampler_seed=42, use_graph=use_graph)
        assert ro.window_f is not None
        if use_graph:
            ro.run_cycles(cycles)
            ro.synchronize()
        else:
            twin, bounds, seen = ws.Block(), Bounds(), []
            for c in range(cycles):
                ro.run_cycle()
                ro.synchronize()
                seen.append(read_cycle(L, ro))
                bounds.cycle(seen[-1], twin.get("ring_cursor"))
                ws.fold(twin, seen[-1])
            out += [twin, bounds, seen]
        out.append((ro.window_f.cpu().numpy().copy(), ro.window_i.cpu().numpy().copy()))
        ro.close()
        L.ctx.close()
    twin, bounds, seen, eager, captured = out
    return eager, twin, bounds, captured, seen


@pytest.mark.parametrize("sampler", ["philox", "numpy"])
def test_device_loop_block_eager_captured_and_twin_agree(sampler):
    eager, twin, bounds, captured, _ = device_blocks(sampler)
    assert_block(eager[0], eager[1], twin, bounds, "eager " + sampler)
    assert np.array_equal(eager[0], captured[0]) and np.array_equal(eager[1], captured[1])
    assert twin.get("cycles") == 6 and twin.get("rows") == 120
    assert twin.get("opt_steps") == twin.get("opt_steps_applied") == 6 and twin.get("action_count").sum() == 120
    assert twin.get("episodes") > 0 and twin.get("episodes") == twin.get("ring_cursor") == twin.get("terminals")
    out = ws.summary(twin, num_actions=3)
    assert out["episode_length_max"] <= 13 and -1.0 <= out["episode_return_min"] <= out["episode_return_max"] <= 1.0
    assert out["explained_variance"] is not None and np.isfinite(out["explained_variance"])


def test_device_loop_block_with_skipped_minibatch_steps():
    # approx_kl over 10 rows is a noisy estimate of either sign and a negative value never stops a cycle; under a threshold of
    # float32(1.5e-12) any positive one of the 36 does
    eager, twin, bounds, captured, seen = device_blocks("philox", ppo_epochs=3, ppo_minibatches=2, ppo_target_kl=1e-12)
    assert_block(eager[0], eager[1], twin, bounds, "minibatch ppo")
    assert np.array_equal(eager[0], captured[0]) and np.array_equal(eager[1], captured[1])
    applied = sum(int((c["applied"] != 0).sum()) for c in seen)
    assert twin.get("cycles") == 6 and twin.get("opt_steps") == 36 and twin.get("stat_steps") == 36
    assert twin.get("opt_steps_applied") == applied and applied < 36
    out = ws.summary(twin, num_actions=3, ppo=True)
    assert out["opt_steps"] == 36 and out["opt_steps_applied"] == applied and out["approx_kl"] is not None


def test_device_loop_block_with_adv_norm():
    eager, twin, bounds, captured, _ = device_blocks("philox", adv_norm=True)
    assert_block(eager[0], eager[1], twin, bounds, "adv_norm")
    assert np.array_equal(eager[0], captured[0]) and np.array_equal(eager[1], captured[1])
    assert twin.get("cycles") == 6 and twin.get("rows") == 120


def test_training_is_bit_identical_with_the_flag_on():
    """Weights, optimizer slots and the rollout planes after 6 replayed cycles, flag on against off.  (Without the feature the
    flag does not parse.)"""
    from paac_amd.paac import DeviceRollout
    runs = []
    for flag in ("true", "false"):
        L, env_creator = seeded_learner(catch_args(["--window_stats", flag]))
        L.global_step = L.init_network()
        ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=True)
        assert (ro.window_f is not None) == (flag == "true")
        ro.run_cycles(6)
        ro.synchronize()
        runs.append([t.cpu().numpy().copy() for _, t in L.update_state] +
                    [t.cpu().numpy().copy() for t in (ro.actions, ro.values, ro.rewards, ro.masks, ro.y, ro.adv, ro.tick, L.loss_dev,
                                                      L.gnorm_dev)])
        ro.close()
        L.ctx.close()
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(a, b) for a, b in zip(*runs))
    assert np.isfinite(runs[0][0]).all()


def _records(folder):
    return [json.loads(line) for line in open(os.path.join(folder, "metrics.jsonl"))]


def test_a_real_run_writes_a_window_record_behind_every_progress_record():
    """paac_amd.train's loop on catch, 128 environments: a log window is 16 cycles, three windows are trained."""
    cycles, folders = 48, []
    for flag in ("true", "false"):
        args = catch_args(["--window_stats", flag], emulator_counts=128, max_global_steps=cycles * 128 * T)
        learner, _ = seeded_learner(args)
        np.random.seed(9)
        learner.train()
        folders.append(args.debugging_folder)
    on, off = _records(folders[0]), _records(folders[1])
    kinds = [r["kind"] for r in on]
    progress = [i for i, k in enumerate(kinds) if k == "progress"]
    assert len(progress) == 3 and all(kinds[i + 1] == "window" for i in progress) and kinds.count("window") == 3
    windows = [r for r in on if r["kind"] == "window"]
    assert [w["global_step"] for w in windows] == [on[i]["global_step"] for i in progress]
    assert sum(w["cycles"] for w in windows) == cycles and sum(w["rows"] for w in windows) == cycles * 128 * T
    assert sum(w["episodes"] for w in windows) == kinds.count("episode") > 0
    assert all(w["episodes_dropped"] == 0 and len(w["action_freq"]) == 3 and abs(sum(w["action_freq"]) - 1.0) < 1e-12 for w in windows)
    assert all(w["explained_variance"] is not None and w["episode_return_mean"] is not None for w in windows)
    # every record from before the flag is what it is without it, wall-clock fields aside.  Episodes that end on the same step
    # take their ring slots in the order their workgroups arrive (an atomic counter): two runs of one command already order
    # them differently (tests/test_evaluation_gpu.py says so too), so the episode records are compared as what each drain
    # wrote, sorted, and last_10_rewards_avg -- the mean of whichever ten entries that order puts last; with 128 environments
    # a step finishes several episodes -- is left out like the wall-clock fields
    def rest(records):
        out = []
        for r in records:
            if r["kind"] == "window":
                continue
            out.append(json.dumps({k: v for k, v in r.items() if k not in ("steps_per_s", "steps_per_s_avg", "seconds", "time",
                                                                               "last_10_rewards_avg")},
                                  sort_keys=True))
        return out
    a, b = rest(on), rest(off)
    assert len(a) == len(b)
    ordered = lambda lines: [l for l in lines if '"kind": "episode"' not in l]
    assert ordered(a) == ordered(b)
    assert sorted(l for l in a if '"kind": "episode"' in l) == sorted(l for l in b if '"kind": "episode"' in l)
    assert [json.loads(l)["kind"] for l in a] == [json.loads(l)["kind"] for l in b]


def test_host_loop_block_equals_the_twin():
    """--host_environments true on catch, N = 4, T = 5, four cycles: the block the eager folds left on the device against the
    twin folded over the feeds of the same cycles; the episodes come from the loop's own bookkeeping."""
    feeds = []
    args = catch_args(["--window_stats", "true", "--host_environments", "true"], max_global_steps=4 * N * T, record_feeds=True,
                      feed_callback=lambda feed: feeds.append(feed))
    learner, _ = seeded_learner(args)
    np.random.seed(9)
    learner.train()
    assert len(feeds) == 4 and learner.host_window is not None
    twin, bounds = ws.Block(), Bounds()
    for feed in feeds:
        cycle = dict(T=T, N=N, A=3, values=feed["values"], rewards=feed["rewards"], masks=feed["masks"],
                     actions=feed["actions"], y=feed["y"], adv=feed["adv"], truncs=None, loss=feed["window_loss"],
                     gnorm=feed["window_gnorm"], ring=None)
        bounds.cycle(cycle, 0)
        ws.fold(twin, cycle)
    assert_block(learner.host_window[0], learner.host_window[1], twin, bounds, "host loop")
    assert twin.get("cycles") == 4 and twin.get("rows") == 80 and twin.get("episodes") == 0
    returns, lengths = learner.host_window_episodes
    assert len(returns) == int(twin.get("terminals")) == len(lengths)
    ws.fold_episodes(twin, returns, lengths)
    assert ws.summary(twin, num_actions=3)["episodes"] == len(returns)
