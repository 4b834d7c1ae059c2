"""--gae_lambda: generalized advantage estimation (Schulman et al., arXiv 1506.02438) beside the reference's n-step return
(paac.py:144-149).  The reference has no GAE, so the checker is this file's own restatement of the contract in
include/paac_hip.h: float32 inputs promoted to float64, every operation a separate IEEE float64 operation in a fixed order.
numpy float64 arithmetic performs the same operations, so y and adv are compared BIT FOR BIT -- the bar
test_nstep_returns_bit_exact holds the n-step scan to."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH_ID = {"NIPS": 0, "NATURE": 1}


# -- the restatement ---------------------------------------------------------------------------------------------------

def gae_restated(v_boot, rewards, masks, values, gamma, lam):
    """-> (y, adv) float32 [T, N].  V_T = v_boot; gl = gamma * lambda, one Python-float product."""
    T = rewards.shape[0]
    gamma, gl = np.float64(gamma), np.float64(float(gamma) * float(lam))
    r, m, V = rewards.astype(np.float64), masks.astype(np.float64), values.astype(np.float64)
    y, adv = np.zeros(rewards.shape, np.float32), np.zeros(rewards.shape, np.float32)
    A = np.zeros(rewards.shape[1], np.float64)
    Vn = v_boot.astype(np.float64)
    for t in reversed(range(T)):
        delta = (r[t] + (gamma * Vn) * m[t]) - V[t]
        A = delta + (gl * A) * m[t]
        adv[t] = A.astype(np.float32)
        y[t] = (A + V[t]).astype(np.float32)
        Vn = V[t]
    return y, adv


def records(T, N, seed):
    """Rollout records as the issue sets them: rewards in {-1, 0, 1}, about 10 % terminals, environment 0 terminal at every
    step and environment 1 never, values at trained magnitude (a few units)."""
    rs = np.random.RandomState(seed)
    v_boot = (3.0 * rs.randn(N)).astype(np.float32)
    rewards = rs.choice([-1.0, 0.0, 1.0], size=(T, N)).astype(np.float32)
    masks = (rs.rand(T, N) > 0.1).astype(np.float32)
    masks[:, 0] = 0.0
    if N > 1:
        masks[:, 1] = 1.0
    values = (3.0 * rs.randn(T, N)).astype(np.float32)
    return v_boot, rewards, masks, values


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_flag_default_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    assert p.parse_args([]).gae_lambda == 1.0
    a = p.parse_args(["--gae_lambda", "0.95"])
    assert a.gae_lambda == 0.95
    text = [t for o, _, _, _, t in train.BUILD_FLAGS if o == ("--gae_lambda",)][0]
    assert "1.0" in text and "n-step" in text
    logger_utils.save_args(a, str(tmp_path / "with"))
    assert logger_utils.load_args(str(tmp_path / "with" / "args.json"))["gae_lambda"] == 0.95
    # an args.json from before the flag: evaluation (paac_amd/test.py: restore_settings) keeps the parser's default
    b = p.parse_args([])
    del b.gae_lambda
    logger_utils.save_args(b, str(tmp_path / "without"))
    assert "gae_lambda" not in logger_utils.load_args(str(tmp_path / "without" / "args.json"))
    from paac_amd import test as evaluation
    for folder, want in (("with", 0.95), ("without", None)):
        cli = argparse.Namespace(folder=str(tmp_path / folder), device="/gpu:0", gif_name=None)
        settings = evaluation.restore_settings(cli)
        assert getattr(settings, "gae_lambda", None) == want and settings.max_global_steps == 0


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")])
def test_actor_learner_rejects_lambda_outside_the_unit_interval(bad):
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    args.gae_lambda = bad
    args.num_actions = 4
    with pytest.raises(ValueError, match="gae_lambda"):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_routing_rule():
    from paac_amd import hip_ops
    assert not hip_ops.uses_gae(None) and not hip_ops.uses_gae(1.0) and not hip_ops.uses_gae(1)
    assert hip_ops.uses_gae(0.0) and hip_ops.uses_gae(0.95) and hip_ops.uses_gae(float(np.nextafter(1.0, 0.0)))


def test_returns_tick_follows_the_routing_rule(monkeypatch):
    """hip_ops.returns_tick: None and 1.0 reach the n-step entry, 0.95 the GAE entry with its lambda; the records and the
    bookkeeping keyword arguments arrive as given."""
    from paac_amd import hip_ops
    calls = []
    monkeypatch.setattr(hip_ops, "nstep_returns_tick", lambda *a, **k: calls.append(("nstep", a, k)))
    monkeypatch.setattr(hip_ops, "gae_returns_tick", lambda *a, **k: calls.append(("gae", a, k)))
    tick = dict(global_step_dev="gs", increment=160, initial_lr=0.0224, lr_annealing_steps=80000000, lr_out_dev="lr",
                tick_dev="tick", tick_inc=5)
    hip_ops.returns_tick("vb", "r", "m", "V", 0.99, "y", "adv", **tick)
    hip_ops.returns_tick("vb", "r", "m", "V", 0.99, "y", "adv", 1.0, **tick)
    hip_ops.returns_tick("vb", "r", "m", "V", 0.99, "y", "adv", gae_lambda=0.95, **tick)
    assert calls == [("nstep", ("vb", "r", "m", "V", 0.99, "y", "adv"), tick)] * 2 + \
        [("gae", ("vb", "r", "m", "V", 0.99, 0.95, "y", "adv"), tick)]


def test_header_declares_the_entries_and_the_enum():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, nargs in (("paac_gae_returns", 11), ("paac_gae_returns_tick", 18)):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name + " missing from the header"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs
        assert "double gae_lambda" in m.group(1) and name in _lib.EXPORTED_SYMBOLS
    # the n-step entries keep their signatures
    assert len(_lib._SIGNATURES["paac_nstep_returns"][1]) == 10 and len(_lib._SIGNATURES["paac_nstep_returns_tick"][1]) == 17
    assert re.search(r"PAAC_RETURNS_NSTEP\s*=\s*0\s*,\s*PAAC_RETURNS_GAE\s*=\s*1", hdr)
    assert (_lib.RETURNS_NSTEP, _lib.RETURNS_GAE) == (0, 1)
    struct = re.search(r"typedef struct \{([^}]*)\} paac_returns;", hdr).group(1)
    fields = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    assert fields[-2:] == ["estimator", "gae_lambda"]                  # trailing: a zero-filled tail is the n-step path
    assert [f for f, _ in _lib.Returns._fields_][-2:] == ["estimator", "gae_lambda"]
    assert len(_lib.Returns._fields_) == len(fields) + 1               # (T, N share a declaration)


def test_restatement_equals_the_closed_form():
    """A_t = sum_k (gamma lambda)^k (prod_{j<k} m_{t+j}) delta_{t+k}, float64; both are float64 sums of at most 20 terms:
    relative 1e-12 of the case's largest |A|."""
    T, N, gamma = 20, 128, 0.99
    for seed, lam in ((0, 0.0), (1, 0.5), (2, 0.95), (3, 1.0)):
        v_boot, r, m, V = records(T, N, seed)
        _, adv = gae_restated(v_boot, r, m, V, gamma, lam)
        r64, m64 = r.astype(np.float64), m.astype(np.float64)
        Vx = np.concatenate([V.astype(np.float64), v_boot.astype(np.float64)[None]])
        delta = r64 + gamma * Vx[1:] * m64 - Vx[:-1]
        closed = np.zeros((T, N))
        for t in range(T):
            w = np.ones(N)
            for k in range(T - t):
                closed[t] += w * delta[t + k]
                w = w * (gamma * lam) * m64[t + k]
        # (adv is the float32 rounding of the float64 A: compare at float64 through a second, unrounded scan)
        A = np.zeros(N)
        Vn = v_boot.astype(np.float64)
        got = np.zeros((T, N))
        for t in reversed(range(T)):
            A = ((r64[t] + (gamma * Vn) * m64[t]) - Vx[t]) + ((gamma * lam) * A) * m64[t]
            got[t] = A
            Vn = Vx[t]
        assert np.array_equal(got.astype(np.float32), adv)
        assert np.abs(got - closed).max() <= 1e-12 * np.abs(closed).max(), (lam, np.abs(got - closed).max())
    # lambda = 0 is the one-step TD error
    v_boot, r, m, V = records(5, 8, 9)
    _, adv = gae_restated(v_boot, r, m, V, gamma, 0.0)
    Vx = np.concatenate([V, v_boot[None]]).astype(np.float64)
    td = (r.astype(np.float64) + (gamma * Vx[1:]) * m.astype(np.float64)) - Vx[:-1]
    assert np.array_equal(adv, td.astype(np.float32))


def test_restatement_at_lambda_one_is_the_n_step_return_up_to_rounding():
    """GAE(1) against oracle.rollout.nstep_returns (float64 rewards / masks, as the reference's buffers are).  Not bitwise;
    the bound is derived: the n-step scan's float32 first product contributes at most 2^-24 |gamma v_boot|, the final float32
    rounding at most 2^-24 |result|, the float64 steps nothing visible: |difference| <= 2^-23 M with
    M = max(|v_boot|, |y|, |adv|) over the case."""
    from oracle import rollout as oroll
    T, N, gamma = 20, 128, 0.99
    worst = 0.0
    for seed in range(200):
        v_boot, r, m, V = records(T, N, 1000 + seed)
        y, adv = gae_restated(v_boot, r, m, V, gamma, 1.0)
        ye, ae = oroll.nstep_returns(v_boot, r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), gamma)
        ye, ae = ye.astype(np.float32), ae.astype(np.float32)
        M = max(np.abs(v_boot).max(), np.abs(ye).max(), np.abs(ae).max())
        dy, da = np.abs(y.astype(np.float64) - ye).max(), np.abs(adv.astype(np.float64) - ae).max()
        worst = max(worst, dy / (2.0 ** -23 * M), da / (2.0 ** -23 * M))
        assert dy <= 2.0 ** -23 * M and da <= 2.0 ** -23 * M, (seed, dy, da, M)
    print("largest |difference| / (2^-23 M) over 200 seeds: %.3f" % worst)


def test_estimators_differ_on_the_cpu():
    """At T = 20 and lambda = 0.95 the two estimators are different quantities, far beyond float32 rounding."""
    from oracle import rollout as oroll
    v_boot, r, m, V = records(20, 128, 5)
    _, adv = gae_restated(v_boot, r, m, V, 0.99, 0.95)
    _, ae = oroll.nstep_returns(v_boot, r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), 0.99)
    M = max(np.abs(adv).max(), np.abs(ae).max())
    assert np.abs(adv - ae).max() > 2.0 ** -10 * M


# -- GPU: the standalone entries ---------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# T = 8: the 8-step chunk / preload filled; T = 9, 17, 20: crossed; N = 65, 256: across the scan's 64-environment workgroup
SHAPES = [(1, 1), (5, 8), (5, 32), (5, 65), (8, 64), (9, 32), (17, 65), (20, 128), (20, 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_gae_returns_bit_exact(T, N):
    import torch
    from paac_amd import hip_ops
    v_boot, r, m, V = records(T, N, T * 1000 + N)
    for lam in (0.0, 0.5, 0.95):
        for gamma in (0.99, 1.0):
            y, adv = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
            hip_ops.gae_returns(dev(v_boot), dev(r), dev(m), dev(V), gamma, lam, y, adv)
            ye, ae = gae_restated(v_boot, r, m, V, gamma, lam)
            assert np.array_equal(y.cpu().numpy(), ye.reshape(-1)), (lam, gamma)
            assert np.array_equal(adv.cpu().numpy(), ae.reshape(-1)), (lam, gamma)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_gae_returns_tick_bit_exact_with_bookkeeping(T, N):
    import torch
    from oracle import rollout as oroll
    from paac_amd import hip_ops
    v_boot, r, m, V = records(T, N, T * 1000 + N + 1)
    gs = torch.tensor([0], dtype=torch.int64, device="cuda")
    tick = torch.tensor([7], dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, device="cuda")
    step = 0
    for inc, lam, gamma in ((160, 0.0, 0.99), (160, 0.5, 1.0), (79999680, 0.95, 0.99), (5, 0.95, 1.0)):
        y, adv = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
        hip_ops.gae_returns_tick(dev(v_boot), dev(r), dev(m), dev(V), gamma, lam, y, adv, gs, inc, 0.0224, 80000000, lr,
                                 tick, T)
        step += inc
        ye, ae = gae_restated(v_boot, r, m, V, gamma, lam)
        assert np.array_equal(y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(adv.cpu().numpy(), ae.reshape(-1))
        assert int(gs.item()) == step
        assert lr.item() == np.float32(oroll.get_lr(step, 0.0224, 80000000))
    assert int(tick.item()) == 7 + 4 * T
    # without a frame counter
    hip_ops.gae_returns_tick(dev(v_boot), dev(r), dev(m), dev(V), 0.99, 0.5, y, adv, gs, 1, 0.0224, 80000000, lr)
    assert int(gs.item()) == step + 1 and int(tick.item()) == 7 + 4 * T


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", SHAPES)
def test_nstep_returns_tick_bit_exact_with_bookkeeping(T, N):
    """The n-step twin: y / adv against oracle.rollout.nstep_returns, the bookkeeping against oracle.rollout.get_lr."""
    import torch
    from oracle import rollout as oroll
    from paac_amd import hip_ops
    v_boot, r, m, V = records(T, N, T * 1000 + N + 2)
    gs = torch.tensor([0], dtype=torch.int64, device="cuda")
    tick = torch.tensor([7], dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, device="cuda")
    step = 0
    for inc, gamma in ((160, 0.99), (160, 1.0), (79999680, 0.99), (5, 1.0)):
        y, adv = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
        hip_ops.nstep_returns_tick(dev(v_boot), dev(r), dev(m), dev(V), gamma, y, adv, gs, inc, 0.0224, 80000000, lr, tick, T)
        step += inc
        ye, ae = oroll.nstep_returns(v_boot, r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), gamma)
        assert np.array_equal(y.cpu().numpy(), ye.reshape(-1).astype(np.float32))
        assert np.array_equal(adv.cpu().numpy(), ae.reshape(-1).astype(np.float32))
        assert int(gs.item()) == step
        assert lr.item() == np.float32(oroll.get_lr(step, 0.0224, 80000000))
    assert int(tick.item()) == 7 + 4 * T
    # without a frame counter
    hip_ops.nstep_returns_tick(dev(v_boot), dev(r), dev(m), dev(V), 0.99, y, adv, gs, 1, 0.0224, 80000000, lr)
    assert int(gs.item()) == step + 1 and int(tick.item()) == 7 + 4 * T
    assert lr.item() == np.float32(oroll.get_lr(step + 1, 0.0224, 80000000))


@pytest.mark.gpu
def test_entries_refuse_bad_lambda_and_unknown_estimators():
    import ctypes
    import torch
    from paac_amd import _lib, hip_ops
    v_boot, r, m, V = records(5, 8, 3)
    y, adv = torch.zeros(40, device="cuda"), torch.zeros(40, device="cuda")
    gs, lr = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.PaacHipError, match="paac_gae_returns: gae_lambda"):
            hip_ops.gae_returns(dev(v_boot), dev(r), dev(m), dev(V), 0.99, bad, y, adv)
        with pytest.raises(_lib.PaacHipError, match="paac_gae_returns_tick: gae_lambda"):
            hip_ops.gae_returns_tick(dev(v_boot), dev(r), dev(m), dev(V), 0.99, bad, y, adv, gs, 1, 0.0224, 100, lr)
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=40)
    n = ctx.layout["total"]
    p, grad = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    s = torch.zeros((40, 84, 84, 4), dtype=torch.uint8, device="cuda")
    acts = torch.zeros(40, dtype=torch.int32, device="cuda")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.PaacHipError, match="paac_loss_backward_returns: gae_lambda"):
            ctx.loss_backward_returns(p, s, acts, dev(v_boot), dev(r), dev(m), dev(V), 0.99, y, adv, 0.02, grad, gae_lambda=bad)
    keep = [dev(v_boot), dev(r), dev(m), dev(V)]
    ret = _lib.Returns(v_boot=keep[0].data_ptr(), rewards=keep[1].data_ptr(), masks=keep[2].data_ptr(),
                       values=keep[3].data_ptr(), T=5, N=8, gamma=0.99, y_out=y.data_ptr(), adv_out=adv.data_ptr(),
                       estimator=2, gae_lambda=0.5)
    rc = ctx.lib.paac_loss_backward_returns(ctx.handle, p.data_ptr(), s.data_ptr(), acts.data_ptr(), ctypes.byref(ret), 40,
                                            0.02, grad.data_ptr(), None, 0, 0, None)
    assert rc < 0 and b"estimator 2" in ctx.lib.paac_last_error()
    ctx.close()


@pytest.mark.gpu
def test_estimators_differ_on_the_gpu():
    """The same records through both entries at T = 20, lambda = 0.95: a build that ignores the flag fails here."""
    import torch
    from paac_amd import hip_ops
    T, N = 20, 128
    v_boot, r, m, V = records(T, N, 5)
    out = []
    for lam in (None, 0.95):
        y, adv = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
        hip_ops.returns(dev(v_boot), dev(r), dev(m), dev(V), 0.99, y, adv, lam)
        out.append(adv.cpu().numpy())
    M = max(np.abs(out[0]).max(), np.abs(out[1]).max())
    assert np.abs(out[0] - out[1]).max() > 2.0 ** -10 * M


# -- GPU: the returns inside the backward's first launch ---------------------------------------------------------------

def upload(ctx, params):
    import torch
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return torch.from_numpy(flat).cuda()


def check_fused_gae(arch_id, arch, A, T, N, lam=0.95, gamma=0.99, routes=("given", "trunk", "kept")):
    """paac_loss_backward_returns with the GAE fields on three routes -- v_boot given after a whole training forward
    (heads_bwd_kernel), v_boot = NULL after a trunk-only training forward over T*N + N rows (heads_train_kernel where the
    geometry has it), and the same with the acting rows kept -- in phases 0, 3 and 1 + 2: y_out / adv_out equal the
    standalone entry's and the restatement's, gradient and loss equal paac_loss_backward fed those y / adv; all bit for bit."""
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    B = T * N
    rs = np.random.RandomState(17 + A + T)
    params = onet.init_params(arch, A, rs, dtype=np.float32)
    states = dev(rs.randint(0, 256, (B + N, 84, 84, 4)).astype(np.uint8))
    acts = dev(rs.randint(0, A, B).astype(np.int32))
    _, r, m, _ = records(T, N, 23 + A)
    r, m = dev(r), dev(m)
    ctx = hip_ops.Context(arch_id, A, max_batch=B + N)
    p = upload(ctx, params)
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    n = ctx.layout["total"]
    values = torch.zeros((T, N), device="cuda")
    probs = torch.zeros((N, A), device="cuda")

    def prepare(route):
        """-> v_boot to pass (None: taken from the forward)"""
        if route == "given":
            vt = torch.zeros(B + N, device="cuda")
            ctx.train_forward(p, states, values=vt)
            return vt[B:].clone()
        for t in range(T):                      # the acting forwards produce values[t] on every route
            if route == "kept":
                ctx.keep_next_forward(t * N)
            ctx.forward(p, states[t * N:(t + 1) * N], probs=probs, values=values[t])
        if route == "kept":
            ctx.bootstrap_forward_trunk(p, states[B:], B)
        else:
            ctx.train_forward_trunk(p, states)
        return None

    prepare("trunk")                            # (fills `values` for the route that does not run acting forwards)
    ctx.loss_backward(p, states[:B], acts, torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), 0.02,
                      torch.zeros(n, device="cuda"), forward_done=True)
    for route in routes:
        for phase in (0, 3, 12):
            y, adv = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
            grad, loss = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            gs = torch.tensor([1000], dtype=torch.int64, device="cuda")
            tick = torch.tensor([7], dtype=torch.int64, device="cuda")
            lr = torch.zeros(1, device="cuda")
            vb = prepare(route)
            ctx.loss_backward_returns(p, states[:B], acts, vb, r, m, values, gamma, y, adv, 0.02, grad, loss, forward_done=True,
                                      phase=1 if phase == 12 else phase, global_step_dev=gs, increment=B, initial_lr=0.0224,
                                      lr_annealing_steps=80000000, lr_out_dev=lr, tick_dev=tick, tick_inc=T, gae_lambda=lam)
            if phase == 12:
                ctx.loss_backward(p, states[:B], acts, y, adv, 0.02, grad, loss, forward_done=True, phase=2)
            torch.cuda.synchronize()
            if vb is None:                      # the bootstrap values the launch computed: rows [B, B + N) of the training set
                vb = ctx.debug_activation(25, B + N)[B:].clone()
            y2, adv2 = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
            gs2 = torch.tensor([1000], dtype=torch.int64, device="cuda")
            tick2 = torch.tensor([7], dtype=torch.int64, device="cuda")
            lr2 = torch.zeros(1, device="cuda")
            hip_ops.gae_returns_tick(vb, r, m, values, gamma, lam, y2, adv2, gs2, B, 0.0224, 80000000, lr2, tick2, T)
            what = (arch, A, route, phase)
            assert torch.equal(y, y2) and torch.equal(adv, adv2), what
            assert torch.equal(gs, gs2) and torch.equal(tick, tick2) and torch.equal(lr, lr2), what
            ye, ae = gae_restated(vb.cpu().numpy(), r.cpu().numpy(), m.cpu().numpy(), values.cpu().numpy(), gamma, lam)
            assert np.array_equal(y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(adv.cpu().numpy(), ae.reshape(-1)), what
            grad2, loss2 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            prepare(route)
            if phase == 12:
                ctx.loss_backward(p, states[:B], acts, y2, adv2, 0.02, grad2, loss2, forward_done=True, phase=1)
                ctx.loss_backward(p, states[:B], acts, y2, adv2, 0.02, grad2, loss2, forward_done=True, phase=2)
            else:
                ctx.loss_backward(p, states[:B], acts, y2, adv2, 0.02, grad2, loss2, forward_done=True, phase=phase)
            torch.cuda.synchronize()
            if phase == 3:                      # (the conv part of a phase-3 gradient stays in slabs until the optimizer step)
                off = [t for t in ctx.layout["tensors"] if t["name"].startswith("fc")][0]["offset"]
                assert torch.equal(grad[off:], grad2[off:]), what
            else:
                assert torch.equal(grad, grad2), what
            assert torch.equal(loss, loss2), what
            assert np.isfinite(grad.cpu().numpy()).all() and float(grad.abs().max()) > 0
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,T,N", [("NATURE", 4, 5, 32), ("NATURE", 18, 20, 8), ("NIPS", 4, 9, 8), ("NIPS", 18, 5, 32)])
def test_fused_gae_returns_equal_the_standalone_entry_and_the_split_backward(arch, A, T, N):
    check_fused_gae(ARCH_ID[arch], arch, A, T, N)


_USER_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from oracle import network as onet
from paac_amd import _lib, networks
CONVS, FC = [(16, 8, 4), (32, 4, 2), (32, 3, 1)], 256
onet.ARCHS["GAE_USER"] = (CONVS, FC)
networks.define_architecture("GAE_USER", CONVS, FC)
assert _lib.user_arch() == (CONVS, FC)
import test_gae
for A, T, N in ((4, 5, 32), (18, 20, 8)):
    test_gae.check_fused_gae(_lib.ARCH_USER, "GAE_USER", A, T, N, routes=("given", "trunk"))
print("GAE_USER_OK")
"""


@pytest.mark.gpu
def test_fused_gae_returns_on_a_user_architecture():
    """A process holds one user geometry: the same check in a child process, on the library build() makes for
    --user_arch 16,32,32,256.  (Kept acting rows need a stock trunk's conv tower -- paac_keep_next_forward refuses a user
    geometry and the device loop does not use them there -- so the two routes a user architecture has are checked.)"""
    res = subprocess.run([sys.executable, "-c", _USER_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "GAE_USER_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,T,N", [("NATURE", 4, 5, 8), ("NIPS", 6, 20, 3)])
def test_zero_filled_tail_and_lambda_one_are_the_n_step_path(arch, A, T, N):
    """paac_returns with estimator = 0, gae_lambda = 0 (a caller from before the fields), and the Python keyword at None /
    1.0: y, adv, bookkeeping, gradient and loss equal paac_nstep_returns_tick + paac_loss_backward bit for bit."""
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    B = T * N
    rs = np.random.RandomState(12)
    params = onet.init_params(arch, A, rs, dtype=np.float32)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    p = upload(ctx, params)
    s, acts = dev(rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)), dev(rs.randint(0, A, B).astype(np.int32))
    v_boot, r, m, V = [dev(a) for a in records(T, N, 4)]
    n = ctx.layout["total"]
    out = []
    for mode in ("separate", None, 1.0):
        y, adv = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        gs = torch.tensor([1000], dtype=torch.int64, device="cuda")
        tick = torch.tensor([7], dtype=torch.int64, device="cuda")
        lr = torch.zeros(1, device="cuda")
        grad, loss = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
        if mode == "separate":
            hip_ops.nstep_returns_tick(v_boot, r, m, V, 0.99, y, adv, gs, B, 0.0224, 80000000, lr, tick, T)
            ctx.loss_backward(p, s, acts, y, adv, 0.02, grad, loss)
        else:
            ctx.loss_backward_returns(p, s, acts, v_boot, r, m, V, 0.99, y, adv, 0.02, grad, loss, global_step_dev=gs,
                                      increment=B, initial_lr=0.0224, lr_annealing_steps=80000000, lr_out_dev=lr,
                                      tick_dev=tick, tick_inc=T, gae_lambda=mode)
        torch.cuda.synchronize()
        out.append((y, adv, gs, tick, lr, grad, loss))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert torch.equal(a, b)
    ctx.close()


# -- GPU: the loops ----------------------------------------------------------------------------------------------------

def loop_args(**kw):
    from test_learner_gpu import make_args
    return make_args(**kw)


def learner_state(learner):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for _, t in learner.update_state]


def run_device_loop(N, T, sampler, cycles, use_graph=True, check=None, **flags):
    from test_learner_gpu import build_learner
    from paac_amd.paac import DeviceRollout
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler=sampler, test_seed=11, **flags)
    if flags.get("gae_lambda", 1.0) is None:
        del args.gae_lambda                     # a Namespace from before the flag
    learner, _, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, env_creator.device_env_spec, sampler=sampler, use_graph=use_graph)
    ys = []
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        ys.append((ro.y.cpu().numpy().copy(), ro.adv.cpu().numpy().copy()))
        if check:
            check(learner, ro, c)
    out = dict(state=learner_state(learner), y=ys, global_step=int(ro.global_step_dev.item()), lr=float(learner.lr_dev.item()))
    ro.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(32, 5), (8, 20)])
@pytest.mark.parametrize("sampler", ["numpy", "philox"])
def test_device_loop_gae(N, T, sampler):
    """The device-resident cycle with --gae_lambda 0.95: after each cycle y and adv are the restatement of the loop's own
    rewards, masks, acting values and bootstrap values, bit for bit; graph replay and eager execution leave identical
    weights and optimizer slots; global_step and lr advance as without the flag."""
    from oracle import rollout as oroll
    cycles, lam = 3, 0.95

    def check(learner, ro, c):
        assert learner.gae_lambda == lam
        v_boot = learner.ctx.debug_activation(25, T * N + N)[T * N:].cpu().numpy()
        r, m, V = ro.rewards.cpu().numpy(), ro.masks.cpu().numpy(), ro.values.cpu().numpy()
        ye, ae = gae_restated(v_boot, r, m, V, learner.gamma, lam)
        assert np.array_equal(ro.y.cpu().numpy(), ye.reshape(-1)), "cycle %d" % c
        assert np.array_equal(ro.adv.cpu().numpy(), ae.reshape(-1)), "cycle %d" % c
        if T == 20:                             # and not the n-step return of the same records
            _, an = oroll.nstep_returns(v_boot, r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), learner.gamma)
            assert np.abs(ae - an).max() > 2.0 ** -10 * max(np.abs(ae).max(), np.abs(an).max())

    graph = run_device_loop(N, T, sampler, cycles, use_graph=True, check=check, gae_lambda=lam)
    eager = run_device_loop(N, T, sampler, cycles, use_graph=False, gae_lambda=lam)
    for a, b in zip(graph["state"], eager["state"]):
        assert np.array_equal(a, b)
    for (y0, a0), (y1, a1) in zip(graph["y"], eager["y"]):
        assert np.array_equal(y0, y1) and np.array_equal(a0, a1)
    step = cycles * N * T
    assert graph["global_step"] == eager["global_step"] == step
    assert graph["lr"] == eager["lr"] == float(np.float32(oroll.get_lr(step, 0.0224, 80000000)))
    assert all(np.isfinite(a).all() for a in graph["state"])


@pytest.mark.gpu
def test_default_is_unchanged_in_the_device_loop():
    """gae_lambda = 1.0 and a Namespace without the attribute: bit-identical weights, slots, y, adv after several cycles."""
    a = run_device_loop(8, 5, "numpy", 4, gae_lambda=1.0)
    b = run_device_loop(8, 5, "numpy", 4, gae_lambda=None)
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(x, y)
    for (y0, a0), (y1, a1) in zip(a["y"], b["y"]):
        assert np.array_equal(y0, y1) and np.array_equal(a0, a1)
    assert a["global_step"] == b["global_step"] and a["lr"] == b["lr"]
    c = run_device_loop(8, 5, "numpy", 4, gae_lambda=0.95)
    assert not np.array_equal(a["state"][0], c["state"][0])            # the flag reaches the update


def run_host_loop(cycles, **flags):
    from test_learner_gpu import build_learner
    N, T = 8, 5
    feeds = []
    args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=cycles * N * T, host_environments=True, record_feeds=True, feed_callback=feeds.append,
                     synthetic_terminal_p=0.1, test_seed=42, **flags)
    if flags.get("gae_lambda", 1.0) is None:
        del args.gae_lambda
    learner, _, _ = build_learner(args)
    np.random.seed(args.test_seed)
    learner.train()
    return learner, feeds, learner_state(learner)


@pytest.mark.gpu
def test_host_loop_gae():
    """The host-plugin loop (PAACLearner._train_host) with --gae_lambda 0.9: the feed's y / adv are the restatement of that
    cycle's records."""
    from oracle import rollout as oroll
    learner, feeds, _ = run_host_loop(3, gae_lambda=0.9)
    assert len(feeds) == 3
    differs = False
    for f in feeds:
        ye, ae = gae_restated(f["v_boot"], f["rewards"], f["masks"], f["values"], learner.gamma, 0.9)
        assert np.array_equal(f["y"], ye.reshape(f["y"].shape)) and np.array_equal(f["adv"], ae.reshape(f["adv"].shape))
        _, an = oroll.nstep_returns(f["v_boot"], f["rewards"].astype(np.float64), f["masks"].astype(np.float64),
                                    f["values"].astype(np.float64), learner.gamma)
        differs = differs or np.abs(ae - an).max() > 2.0 ** -10 * np.abs(an).max()
    assert differs


@pytest.mark.gpu
def test_default_is_unchanged_in_the_host_loop():
    _, fa, a = run_host_loop(3, gae_lambda=1.0)
    _, fb, b = run_host_loop(3, gae_lambda=None)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for f, g in zip(fa, fb):
        assert np.array_equal(f["y"], g["y"]) and np.array_equal(f["adv"], g["adv"])
