"""-m gpu: --ppo_target_kl D (include/paac_hip.h has the contract).  Everything here is bit for bit: the gated entries
against their ungated twins and against the state before the call; a stopped cycle against the shorter run; graph replay
against eager execution.  NIPS, N = 8, T = 5 (40 rows) unless said otherwise."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 8, 5


# -- (1) the entries ---------------------------------------------------------------------------------------------------

def _entry_case(optimizer):
    """-> (ctx, pre-state tensors [params, slot1, slot2(, powers)], grad, states, lr_dev)."""
    from paac_amd import hip_ops
    from test_adam import ARCH_ID, gradient, make_case, upload
    params, states, _, _, _ = make_case("NIPS", 4, N * T, seed=5)
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=N * T)
    ctx.set_managed_weights(True)
    n = ctx.layout["total"]
    p = upload(ctx, params)
    rs = np.random.RandomState(17)
    if optimizer == "adam":
        pre = [p, torch.from_numpy(rs.randn(n).astype(np.float32) * 1e-3).cuda(),
               torch.from_numpy((rs.rand(n) * 1e-4).astype(np.float32)).cuda(),
               torch.tensor([0.9 ** 3, 0.999 ** 3], dtype=torch.float32, device="cuda")]
    else:
        # (rmsprop_mom: momentum 0.9 on a momentum slot that already holds something -- the update rule the learner never
        # selects but the entry serves)
        mom = rs.randn(n).astype(np.float32) * 1e-3 if optimizer == "rmsprop_mom" else np.zeros(n, dtype=np.float32)
        pre = [p, torch.from_numpy((1.0 + rs.rand(n)).astype(np.float32)).cuda(), torch.from_numpy(mom).cuda()]
    grad = torch.from_numpy(gradient(ctx.layout, 0.5, 1.0, seed=4)).cuda()
    return ctx, pre, grad, torch.from_numpy(states).cuda(), torch.tensor([0.0224], device="cuda")


def _step(ctx, optimizer, state, grad, lr_dev, mode, gnorm, gate=None):
    if optimizer == "adam":
        a = (state[0], grad, state[1], state[2], state[3], lr_dev, 0.9, 0.999, 1e-5, 0.5, mode, 1.0, gnorm)
        return ctx.clip_adam(*a) if gate is None else ctx.clip_adam_gated(*a, **gate)
    a = (state[0], grad, state[1], state[2], lr_dev, 0.99, 0.9 if optimizer == "rmsprop_mom" else 0.0, 0.1, 0.5, mode, 1.0, gnorm)
    return ctx.clip_rmsprop(*a) if gate is None else ctx.clip_rmsprop_gated(*a, **gate)


@pytest.mark.parametrize("mode", ["global", "local", "ignore"])
@pytest.mark.parametrize("optimizer", ["rmsprop", "rmsprop_mom", "adam"])
def test_gated_entry_applies_or_leaves_everything(optimizer, mode):
    from paac_amd import _lib
    code = {"ignore": _lib.CLIP_IGNORE, "global": _lib.CLIP_GLOBAL, "local": _lib.CLIP_LOCAL}[mode]
    ctx, pre, grad, states, lr_dev = _entry_case(optimizer)
    thr = float(np.float32(0.03))
    SENTINEL = -7.0

    def logits(p):
        out = torch.zeros((N * T, 4), device="cuda")
        ctx.forward(p, states, logits=out)
        return out

    def fresh():
        state = [t.clone() for t in pre]
        ctx.pack_weights(state[0])
        return state

    def gate_of(kl, first, stop, scale=1.0):
        g = dict(kl=torch.tensor([kl], dtype=torch.float32, device="cuda"), kl_scale=scale, thr=thr, first=first, stop=stop,
                 applied=torch.full((1,), -1, dtype=torch.int32, device="cuda"),
                 checked=torch.full((1,), -1.0, dtype=torch.float32, device="cuda"))
        return g

    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    # the ungated twin
    twin, gn_twin = fresh(), torch.full((1,), SENTINEL, device="cuda")
    logits_pre = logits(twin[0])
    _step(ctx, optimizer, twin, grad, lr_dev, code, gn_twin)
    logits_twin = logits(twin[0])
    assert not same(twin[:3], pre[:3]) and not torch.equal(logits_twin, logits_pre) and gn_twin.item() != SENTINEL
    # kl under thr (exactly at it: the rule is !(k <= thr)), a stale stop flag cleared by first: the twin's step
    for kl, scale in ((0.01, 1.0), (thr, 1.0), (2 * thr, 0.5)):
        st, gn, stop = fresh(), torch.full((1,), SENTINEL, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
        g = gate_of(kl, 1, stop, scale)
        _step(ctx, optimizer, st, grad, lr_dev, code, gn, g)
        assert same(st, twin) and torch.equal(gn, gn_twin) and torch.equal(logits(st[0]), logits_twin), (kl, scale)
        assert stop.item() == 0 and g["applied"].item() == 1
        assert g["checked"].item() == float(np.float32(kl) * np.float32(scale))
    # kl over thr, and NaN: nothing moves; then sticky; then a new cycle's first step applies
    for kl in (float(np.nextafter(np.float32(thr), np.float32(1))), 0.5, float("nan")):
        st, gn, stop = fresh(), torch.full((1,), SENTINEL, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        g = gate_of(kl, 1, stop)
        _step(ctx, optimizer, st, grad, lr_dev, code, gn, g)
        assert same(st, pre) and gn.item() == SENTINEL and torch.equal(logits(st[0]), logits_pre), kl
        assert stop.item() == 1 and g["applied"].item() == 0
        got = g["checked"].item()
        assert (got != got) if kl != kl else got == float(np.float32(kl))
        g2 = gate_of(1e-6, 0, stop)                      # sticky: not the first gated step, a tiny kl, still skipped
        _step(ctx, optimizer, st, grad, lr_dev, code, gn, g2)
        assert same(st, pre) and gn.item() == SENTINEL and stop.item() == 1 and g2["applied"].item() == 0
        assert g2["checked"].item() == float(np.float32(1e-6))
        g3 = gate_of(1e-6, 1, stop)                      # the next cycle's first gated step
        _step(ctx, optimizer, st, grad, lr_dev, code, gn, g3)
        assert same(st, twin) and torch.equal(gn, gn_twin) and stop.item() == 0 and g3["applied"].item() == 1
        assert torch.equal(logits(st[0]), logits_twin)
    # applied / checked are nullable
    st, stop = fresh(), torch.zeros(1, dtype=torch.int32, device="cuda")
    g = gate_of(0.5, 1, stop)
    g.update(applied=None, checked=None)
    _step(ctx, optimizer, st, grad, lr_dev, code, None, g)
    assert same(st, pre) and stop.item() == 1
    ctx.close()


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_a_skipped_step_completes_the_pending_slab_reduction(optimizer):
    """A phase-3 backward leaves the conv part of `grad` to the next optimizer step's norm pass; a skipped step still does
    that work: grad equals the phase-0 gradient bit for bit, and the ctx takes the next backward."""
    from paac_amd import _lib
    from test_adam import make_case
    ctx, pre, _, states, lr_dev = _entry_case(optimizer)
    _, _, idx, y, adv = make_case("NIPS", 4, N * T, seed=5)
    dev = [torch.from_numpy(a).cuda() for a in (idx, y, adv)]
    n = ctx.layout["total"]
    ctx.pack_weights(pre[0])
    g0, g3 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    ctx.loss_backward(pre[0], states, *dev, 0.02, g0, phase=0)
    ctx.loss_backward(pre[0], states, *dev, 0.02, g3, phase=3)
    torch.cuda.synchronize()
    assert not torch.equal(g0, g3)                       # the conv weight gradients are still split-K slabs
    st, stop = [t.clone() for t in pre], torch.zeros(1, dtype=torch.int32, device="cuda")
    gate = dict(kl=torch.tensor([1.0], device="cuda"), thr=0.03, first=1, stop=stop)
    _step(ctx, optimizer, st, g3, lr_dev, _lib.CLIP_GLOBAL, None, gate)
    torch.cuda.synchronize()
    assert stop.item() == 1 and all(torch.equal(a, b) for a, b in zip(st, pre))
    assert torch.equal(g0, g3)
    g0b = torch.zeros(n, device="cuda")
    ctx.loss_backward(pre[0], states, *dev, 0.02, g0b, phase=0)       # nothing is left pending in the ctx
    assert torch.equal(g0b, g0)
    ctx.close()


def test_gated_entries_refuse_bad_gates():
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(0, 4, max_batch=8)
    n = ctx.layout["total"]
    z = lambda k=n: torch.zeros(k, device="cuda")
    stop, kl = torch.zeros(1, dtype=torch.int32, device="cuda"), z(1)
    good = dict(kl=kl, thr=0.03, first=1, stop=stop)
    bad = [dict(good, kl=None), dict(good, stop=None), dict(good, thr=float("nan")), dict(good, thr=-0.01),
           dict(good, kl_scale=0.0), dict(good, kl_scale=-1.0), dict(good, kl_scale=float("inf")),
           dict(good, kl_scale=float("nan"))]
    p = z() + 1.0
    for gate in bad:
        with pytest.raises(_lib.PaacHipError, match="paac_clip_rmsprop_gated"):
            ctx.clip_rmsprop_gated(p, z(), z() + 1, z(), z(1), 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL, **gate)
        with pytest.raises(_lib.PaacHipError, match="paac_clip_adam_gated"):
            ctx.clip_adam_gated(p, z(), z(), z(), z(2) + 0.9, z(1), 0.9, 0.999, 1e-5, 3.0, _lib.CLIP_GLOBAL, **gate)
    # a NULL gate (the wrappers always build one: straight through the library)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    a, b, c, d, lr = p, z(), z() + 1, z(), z(1)
    rc = ctx.lib.paac_clip_rmsprop_gated(ctx.handle, vp(a), vp(b), vp(c), vp(d), n, vp(lr), 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL,
                                         1.0, None, None, None)
    assert rc < 0 and b"null gate" in ctx.lib.paac_last_error()
    pw = z(2) + 0.9
    rc = ctx.lib.paac_clip_adam_gated(ctx.handle, vp(a), vp(b), vp(c), vp(d), vp(pw), n, vp(lr), 0.9, 0.999, 1e-5, 3.0,
                                      _lib.CLIP_GLOBAL, 1.0, None, None, None)
    assert rc < 0 and b"null gate" in ctx.lib.paac_last_error()
    torch.cuda.synchronize()
    assert float(p.min()) == 1.0 and float(p.max()) == 1.0 and stop.item() == 0     # nothing ran
    ctx.close()


# -- the loops ---------------------------------------------------------------------------------------------------------

def _args(drop=False, **flags):
    from test_gae import loop_args
    flags.setdefault("sampler", "philox")
    args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, test_seed=11, ppo_clip=0.2, **flags)
    if drop:
        del args.ppo_target_kl                            # a Namespace from before the flag
    return args


def _record(L):
    torch.cuda.synchronize()
    rec = dict(state=[t.cpu().numpy().copy() for _, t in L.update_state],
               stats=L.ppo_stats.cpu().numpy().copy() if L.ppo_stats is not None else None)      # (--ppo_epochs 1 has none)
    if L.target_kl_on:
        rec.update(applied=L.ppo_applied.cpu().numpy().copy(), checked=L.ppo_kl_checked.cpu().numpy().copy())
    return rec


def device_run(cycles, use_graph=False, drop=False, each=None, **flags):
    """`cycles` cycles of the device loop from the fixed start (weights of seed 0, the environments' seeds) -> _record."""
    from test_learner_gpu import build_learner
    from paac_amd.paac import DeviceRollout
    args = _args(drop, **flags)
    L, _, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler=args.sampler, sampler_seed=42, use_graph=use_graph)
    for c in range(cycles):
        ro.run_cycle()
        if each is not None:
            ro.synchronize()
            each(L, c)
    ro.synchronize()
    rec = _record(L)
    ro.close()
    return rec


def host_run(cycles, drop=False, **flags):
    from test_learner_gpu import build_learner
    args = _args(drop, host_environments=True, **flags)
    args.max_global_steps = cycles * N * T
    L, _, _ = build_learner(args)
    np.random.seed(args.test_seed)
    L.train()
    return _record(L)


def same_state(a, b):
    return len(a["state"]) == len(b["state"]) and all(np.array_equal(x, y) for x, y in zip(a["state"], b["state"]))


# -- (2) D = 0 and a D that can never trigger ---------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("loop", ["device", "host"])
def test_off_and_never_triggering_equal_the_run_without_the_flag(loop, M):
    run = (lambda **kw: device_run(4, use_graph=True, **kw)) if loop == "device" else (lambda **kw: host_run(4, **kw))
    flags = dict(ppo_epochs=4, ppo_minibatches=M)
    base = run(drop=True, **flags)
    off = run(ppo_target_kl=0.0, **flags)
    never = run(ppo_target_kl=1e30, **flags)
    assert "applied" not in off and same_state(base, off) and np.array_equal(base["stats"], off["stats"])
    assert same_state(base, never) and np.array_equal(base["stats"], never["stats"])
    assert never["applied"].shape == (4 * M,) and (never["applied"] == 1).all()
    gated = slice(0 if M > 1 else 1, None)
    assert np.array_equal(never["checked"][gated], base["stats"][gated, 1])
    assert np.isfinite(base["state"][0]).all() and np.abs(base["stats"][1:, 1]).max() > 0


# -- (3), (4) stopping equals a shorter run ----------------------------------------------------------------------------

def stop_positions(kl, first_gated):
    """-> [(j, D)]: the gated steps where kl is a new running maximum above 0, each with a D whose float32(1.5 * D) lies
    strictly between the previous maximum and kl[j]."""
    out, best = [], np.float32(0.0)
    for j in range(first_gated, len(kl)):
        if kl[j] > best:
            D = (float(best) + float(kl[j])) / 2 / 1.5
            thr = np.float32(1.5 * D)
            if best < thr < kl[j]:                        # (two adjacent floats leave no room: not a position)
                out.append((j, D))
            best = kl[j]
    return out


# approx_kl over 40 rows is a noisy estimate of either sign: at the default learning rate (0.0224, and Adam's usual 1e-4) every
# value of the first cycle from this start is negative, and a negative value never stops a cycle.  The learning rates below
# were found by running the ungated cycle over a grid of them (RMSProp 0.02 .. 3, Adam 1e-4 .. 2e-2) and taking one whose
# cycle has at least two stop positions; the tests assert that it has.
STOP_LR = {"rmsprop": 0.3, "adam": 0.005}                 # M = 1, K = 6: positions 3, 5 and 1, 3
STOP_LR_MINIBATCH = 0.2                                   # M = 2, K = 3, RMSProp: positions 1, 4


@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_a_stopped_cycle_equals_the_shorter_run(optimizer):
    """M = 1, K = 6, one cycle from the fixed start, -lr raised (STOP_LR above says why)."""
    K = 6
    flags = dict(optimizer=optimizer, initial_lr=STOP_LR[optimizer])
    if optimizer == "adam":
        flags.update(e=1e-5)
    free = device_run(1, ppo_epochs=K, **flags)
    kl = free["stats"][:, 1]
    print("approx_kl of the ungated cycle (%s):" % optimizer, kl.tolist())
    assert free["stats"][0, 1] == 0
    positions = stop_positions(kl, 1)
    print("stop positions:", positions)
    assert len(positions) >= 2, kl
    for j, D in positions:
        gated = device_run(1, ppo_epochs=K, ppo_target_kl=D, **flags)
        short = device_run(1, ppo_epochs=j, **flags)
        assert gated["applied"].tolist() == [1] * j + [0] * (K - j), (j, gated["applied"])
        assert same_state(gated, short), j               # weights, slots and (Adam) the powers
        assert np.array_equal(gated["checked"][1:j + 1], kl[1:j + 1]), j
        assert np.array_equal(gated["stats"][:j + 1], free["stats"][:j + 1])
    assert not same_state(free, short)


# RMSProp at STOP_LR_MINIBATCH carries the case as it is set: at least two positions, one of them no multiple of M.  No Adam
# learning rate of the grid gave a second position at this shape; the Adam case is there beside it for what RMSProp cannot
# show -- the powers of a cycle that stops inside an epoch -- with the one position its rate gives, step 1.
@pytest.mark.parametrize("optimizer,lr,need", [("rmsprop", STOP_LR_MINIBATCH, 2), ("adam", 0.005, 1)])
def test_a_stopped_minibatch_cycle_equals_the_hand_driven_steps(monkeypatch, optimizer, lr, need):
    """M = 2, K = 3: the expected weights come from the learner's own ungated pieces, minibatch_step_backward(s) and
    apply_gradients(), for the first j steps behind the loop's own rollout, record pass and shuffles.  (Recomputed-trunk
    route, so that step 0's approx_kl is exactly 0 and j = 0 is no stop position.)"""
    from test_learner_gpu import build_learner
    from paac_amd.paac import DeviceRollout
    monkeypatch.setenv("PAAC_REUSE_ACTING", "0")
    K, M = 3, 2
    flags = dict(ppo_epochs=K, ppo_minibatches=M, optimizer=optimizer, initial_lr=lr)
    if optimizer == "adam":
        flags.update(e=1e-5)
    free = device_run(1, **flags)
    kl = free["stats"][:, 1]
    print("approx_kl of the ungated cycle (%s):" % optimizer, kl.tolist())
    assert kl[0] == 0
    positions = stop_positions(kl, 0)
    print("stop positions:", positions)
    assert len(positions) >= need and any(j % M for j, _ in positions), kl
    for j, D in positions:
        gated = device_run(1, ppo_target_kl=D, **flags)
        assert gated["applied"].tolist() == [1] * j + [0] * (K * M - j), (j, gated["applied"])
        assert np.array_equal(gated["checked"][:j + 1], kl[:j + 1]), j
        # by hand
        args = _args(**flags)
        L, _, env_creator = build_learner(args)
        L.global_step = L.init_network()
        ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=False)
        with torch.cuda.stream(ro.stream):
            ro._rollout_and_backward(0)                   # rollout, record, returns, shuffles, step 0's backward
            for s in range(j):
                if s > 0:
                    L.minibatch_step_backward(s, ro.rollout_states(0), ro.actions.view(-1), ro.y, ro.actor_adv, phase=3)
                L.apply_gradients()
        ro.synchronize()
        assert same_state(gated, _record(L)), j
        ro.close()


# -- (5) graph replay equals eager -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampler", ["philox", "numpy"])
def test_graph_replay_equals_eager(sampler):
    """6 cycles, K = 4, -lr 0.3 (STOP_LR above), thr = the largest approx_kl of cycle 1 (taken from an ungated cycle: the
    gated run's first cycle is that cycle until it stops, and it never does): cycle 1 applies every step, and the policy
    moves further than that in some step of a later cycle."""
    K, cycles = 4, 6
    flags = dict(ppo_epochs=K, sampler=sampler, initial_lr=STOP_LR["rmsprop"])
    kl = device_run(1, **flags)["stats"][1:, 1]
    thr = np.float32(kl.max())
    D = float(thr) / 1.5
    if np.float32(1.5 * D) < thr:
        D = float(np.nextafter(thr, np.float32(1))) / 1.5
    assert np.float32(1.5 * D) >= thr > 0
    hist = {True: [], False: []}
    out = {g: device_run(cycles, use_graph=g, ppo_target_kl=D,
                         each=lambda L, c, g=g: hist[g].append(L.ppo_applied.cpu().numpy().copy()), **flags)
           for g in (True, False)}
    print("applied per cycle:", [h.tolist() for h in hist[True]])
    assert same_state(out[True], out[False])
    assert len(hist[True]) == cycles and all(np.array_equal(a, b) for a, b in zip(hist[True], hist[False]))
    assert hist[True][0].tolist() == [1] * K
    assert any(h.sum() < K for h in hist[True]) and any(h.sum() == K for h in hist[True])
    for h in hist[True]:                                  # sticky inside a cycle, cleared by the next one
        assert h[0] == 1 and (np.diff(h) <= 0).all()


# -- (6) metrics ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2])
def test_metrics_carry_the_gates_decisions(tmp_path, M):
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    K, n = 3, 32
    recs = {}
    for name, extra in (("off", {}), ("on", dict(ppo_target_kl=1e-4))):
        folder = tmp_path / name
        args = loop_args(game="pong", arch="NIPS", emulator_counts=n, emulator_workers=0, max_local_steps=T,
                         max_global_steps=64 * n * T, synthetic_terminal_p=0.1, sampler="philox", ppo_epochs=K,
                         ppo_minibatches=M, debugging_folder=str(folder), **extra)
        L, _, _ = build_learner(args)
        L.train()
        recs[name] = [json.loads(l) for l in open(folder / "metrics.jsonl")]
    steps = {k: [r for r in v if r["kind"] == "ppo_epoch"] for k, v in recs.items()}
    progress = {k: [r for r in v if r["kind"] == "progress"] for k, v in recs.items()}
    assert len(steps["off"]) == len(steps["on"]) == K * M and len(progress["off"]) == len(progress["on"]) == 1
    # without the flag: the keys from before it
    base = {"kind", "time", "global_step", "epoch", "loss", "actor_loss", "critic_loss", "entropy", "clip_fraction", "approx_kl"}
    if M > 1:
        base |= {"minibatch"}
    assert all(set(r) == base for r in steps["off"])
    assert set(progress["off"][0]) == {"kind", "time", "global_step", "steps_per_s", "steps_per_s_avg", "last_10_rewards_avg", "lr",
                                       "grad_norm", "loss", "actor_loss", "critic_loss", "entropy"}
    # with it: applied and kl_checked on every gated step's record, ppo_steps_applied on the progress record
    for s, r in enumerate(steps["on"]):
        if M == 1 and s == 0:
            assert set(r) == base
            continue
        assert set(r) == base | {"applied", "kl_checked"} and isinstance(r["applied"], bool)
        assert r["kl_checked"] == r["approx_kl"]
    assert set(progress["on"][0]) == set(progress["off"][0]) | {"ppo_steps_applied"}
    applied = [r.get("applied", True) for r in steps["on"]]
    assert progress["on"][0]["ppo_steps_applied"] == sum(applied) and applied == sorted(applied, reverse=True)
