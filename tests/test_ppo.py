"""--ppo_epochs / --ppo_clip: PPO's clipped-surrogate epochs (Schulman et al., arXiv 1707.06347) on one rollout.  The reference
has no PPO, so the checker is this file's float64 restatement of the contract in include/paac_hip.h.  The surrogate's gradient
is the reference loss's gradient at the effective advantage adv * active * (p + eps) / (p_old + eps) (substitute it into
oracle/network.py:head_grads), so the gradients come from the unmodified oracle; the actor scalar, clip_fraction and approx_kl
are restated here.  Bars: the ones tests/test_hip_network.py holds the backward to -- 1e-4 of max(|want|.max(), 1e-3 * global
norm) per tensor, 1e-4 on the loss scalars; clip_fraction is a count over B and must be exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARCH_ID = {"NIPS": 0, "NATURE": 1}
EPS = 1e-30


# -- the restatement ---------------------------------------------------------------------------------------------------

def ppo_restated(pi, idx, adv, p_old, clip, beta):
    """float64 -> dict(active, adv_eff, actor, clip_fraction, approx_kl, ratio)."""
    pi, adv, p_old = pi.astype(np.float64), adv.astype(np.float64), p_old.astype(np.float64)
    p = pi[np.arange(len(idx)), idx]
    r = p * (1.0 / (p_old + EPS))
    clipped = ((adv > 0) & (r > 1.0 + clip)) | ((adv < 0) & (r < 1.0 - clip))
    ent = -(pi * np.log(pi + EPS)).sum(axis=1)
    surr = np.minimum(r * adv, np.clip(r, 1.0 - clip, 1.0 + clip) * adv)
    return dict(active=~clipped, adv_eff=adv * (~clipped) * ((p + EPS) / (p_old + EPS)), ratio=r,   # (x / x == 1 exactly)
                actor=np.mean(-(surr + beta * ent)), clip_fraction=np.mean(clipped),
                approx_kl=np.mean(np.log(p_old + EPS) - np.log(p + EPS)))


def restated_loss(logits, v, idx, y, adv, p_old, clip, beta):
    """The whole restated loss as a function of the heads' outputs (for the difference quotients)."""
    z = logits - logits.max(axis=1, keepdims=True)
    pi = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    return 5.0 * (ppo_restated(pi, idx, adv, p_old, clip, beta)["actor"] + np.mean(0.25 * (y - v) ** 2))


def restated_head_grads(logits, v, idx, y, adv, p_old, clip, beta):
    from oracle import network as onet
    z = logits - logits.max(axis=1, keepdims=True)
    pi = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    R = ppo_restated(pi, idx, adv, p_old, clip, beta)
    return onet.head_grads(pi, v, np.eye(pi.shape[1])[idx], y, R["adv_eff"], beta)


def heads_case(B, A, seed):
    rs = np.random.RandomState(seed)
    logits, v = rs.randn(B, A), rs.randn(B)
    z = logits - logits.max(axis=1, keepdims=True)
    pi = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    idx = rs.randint(0, A, B)
    return logits, v, pi, idx, rs.randn(B), rs.randn(B)


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_flag_defaults_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    d = p.parse_args([])
    assert d.ppo_epochs == 1 and d.ppo_clip == 0.2
    a = p.parse_args(["--ppo_epochs", "4", "--ppo_clip", "0.1"])
    assert a.ppo_epochs == 4 and a.ppo_clip == 0.1
    assert {("--ppo_epochs",), ("--ppo_clip",)} <= {o for o, _, _, _, _ in train.BUILD_FLAGS}
    logger_utils.save_args(a, str(tmp_path))
    back = logger_utils.load_args(str(tmp_path / "args.json"))
    assert back["ppo_epochs"] == 4 and back["ppo_clip"] == 0.1


@pytest.mark.parametrize("field,bad", [("ppo_epochs", 0), ("ppo_epochs", -3), ("ppo_epochs", 17), ("ppo_epochs", 2.5),
                                       ("ppo_clip", 0.0), ("ppo_clip", 1.0), ("ppo_clip", -0.2), ("ppo_clip", float("nan"))])
def test_actor_learner_refuses_bad_flags(field, bad):
    from paac_amd import _lib, train
    from paac_amd.actor_learner import ActorLearner
    assert _lib.PPO_EPOCHS_MAX == 16
    args = train.get_arg_parser().parse_args([])
    setattr(args, field, bad)
    args.num_actions = 4
    with pytest.raises(ValueError, match=field):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_header_declares_the_entries():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, nargs, must in (("paac_loss_backward_ppo", 16, ("const float* p_old", "float clip_eps", "float* ppo_stats_out",
                                                              "int forward_done", "int phase")),
                              ("paac_loss_backward_record", 14, ("float* p_old_out", "int forward_done", "int phase"))):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name + " missing from the header"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs
        assert all(t in m.group(1) for t in must) and name in _lib.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+PAAC_PPO_EPOCHS_MAX\s+16", hdr)
    m = re.search(r"int\s+paac_loss_backward_returns_record\s*\(([^;]*)\);", hdr)
    assert m and "const paac_returns* ret" in m.group(1) and "float* p_old_out" in m.group(1)
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["paac_loss_backward_returns_record"][1]) == 13
    assert _lib.Returns._fields_[-1][0] == "gae_lambda"                # paac_returns itself is unchanged
    for text in ("1 + EPS", "1 - EPS", "clip_fraction", "approx_kl", "p_old[i] = pi(a_i | s_i)"):
        assert text in hdr, text


def test_restatement_with_p_old_equal_p_is_the_reference_gradient():
    from oracle import network as onet
    logits, v, pi, idx, y, adv = heads_case(64, 6, 1)
    p_old = pi[np.arange(64), idx]
    R = ppo_restated(pi, idx, adv, p_old, 0.2, 0.02)
    assert R["active"].all() and R["clip_fraction"] == 0.0 and R["approx_kl"] == 0.0
    assert np.array_equal(R["adv_eff"], adv)
    got, want = restated_head_grads(logits, v, idx, y, adv, p_old, 0.2, 0.02), onet.head_grads(pi, v, np.eye(6)[idx], y, adv, 0.02)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... and the actor scalar is the reference's with log pi replaced by the ratio (= 1): -(adv + beta H)
    ent = -(pi * np.log(pi + EPS)).sum(axis=1)
    assert abs(R["actor"] - np.mean(-(adv + 0.02 * ent))) < 1e-15


def test_restated_gradient_is_the_derivative_of_the_restated_loss():
    """Central differences in float64 on rows away from the clip bounds (ratios designed at least 0.05 from 1 +- EPS; a step of
    1e-6 in a logit moves a ratio by at most 2e-6).  Truncation error of the quotient ~ h^2 = 1e-12, cancellation ~ 1e-16 / h =
    1e-10 of the loss: the bar is 1e-7 absolute on gradients of order 1e-2."""
    B, A, clip, beta, h = 48, 6, 0.2, 0.02, 1e-6
    logits, v, pi, idx, y, adv = heads_case(B, A, 2)
    ratios = np.array([0.5, 0.85, 0.95, 1.05, 1.15, 2.0])[np.arange(B) % 6]
    p_old = pi[np.arange(B), idx] / ratios
    dlogits, dv = restated_head_grads(logits, v, idx, y, adv, p_old, clip, beta)
    R = ppo_restated(pi, idx, adv, p_old, clip, beta)
    assert 0 < R["clip_fraction"] < 1
    for i in range(B):
        for a in range(A):
            lp, lm = logits.copy(), logits.copy()
            lp[i, a] += h
            lm[i, a] -= h
            q = (restated_loss(lp, v, idx, y, adv, p_old, clip, beta) - restated_loss(lm, v, idx, y, adv, p_old, clip, beta)) / (2 * h)
            assert abs(q - dlogits[i, a]) < 1e-7, (i, a, q, dlogits[i, a])
        vp, vm = v.copy(), v.copy()
        vp[i] += h
        vm[i] -= h
        q = (restated_loss(logits, vp, idx, y, adv, p_old, clip, beta) - restated_loss(logits, vm, idx, y, adv, p_old, clip, beta)) / (2 * h)
        assert abs(q - dv[i]) < 1e-7


def test_a_clipped_rows_gradient_is_entropy_and_critic_only():
    from oracle import network as onet
    B, A = 32, 4
    logits, v, pi, idx, y, adv = heads_case(B, A, 3)
    adv = np.abs(adv) + 0.1
    p_old = pi[np.arange(B), idx] / 2.0            # ratio 2 with adv > 0: every row clipped
    R = ppo_restated(pi, idx, adv, p_old, 0.2, 0.02)
    assert not R["active"].any() and R["clip_fraction"] == 1.0
    got = restated_head_grads(logits, v, idx, y, adv, p_old, 0.2, 0.02)
    want = onet.head_grads(pi, v, np.eye(A)[idx], y, np.zeros(B), 0.02)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the mirrored case: ratio 0.5 with adv < 0
    R = ppo_restated(pi, idx, -adv, pi[np.arange(B), idx] * 2.0, 0.2, 0.02)
    assert not R["active"].any()
    # ... and the same ratios with the other sign of adv are NOT clipped (the objective's pessimistic side)
    assert ppo_restated(pi, idx, -adv, p_old, 0.2, 0.02)["active"].all()


# -- GPU: kernel level -------------------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(ctx, params):
    import torch
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return torch.from_numpy(flat).cuda()


def unflatten(ctx, flat):
    host = flat.detach().cpu().numpy()
    return {t["name"]: host[t["offset"]:t["offset"] + t["size"]].reshape(t["shape"]) for t in ctx.layout["tensors"]}


RATIOS = np.array([0.5, 0.85, 0.95, 1.05, 1.15, 2.0])


def ppo_all_routes(ctx, p, s, acts, y, adv, p_old, clip, B):
    """paac_loss_backward_ppo on every route and phase -> (grad, loss, stats) of phase 0 after a whole forward; asserts the
    others equal it bit for bit: phases 1 + 2 and 3 (its fc / heads tail: the conv part stays in slabs until the optimizer
    step), and the trunk-only forward (heads_train_kernel on the three-conv tower, the deferred heads launch elsewhere)."""
    import torch
    n = ctx.layout["total"]
    off = [t for t in ctx.layout["tensors"] if t["name"].startswith("fc")][0]["offset"]
    out = {}
    for route in ("whole", "trunk"):
        for phase in (0, 12, 3):
            grad, loss, stats = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
            if route == "trunk":
                ctx.train_forward_trunk(p, s)
            else:
                ctx.train_forward(p, s)
            ctx.loss_backward_ppo(p, s, acts, y, adv, p_old, clip, 0.02, grad, loss, stats, forward_done=True,
                                  phase=1 if phase == 12 else phase)
            if phase == 12:
                ctx.loss_backward_ppo(p, s, acts, y, adv, p_old, clip, 0.02, grad, loss, None, forward_done=True, phase=2)
            torch.cuda.synchronize()
            out[(route, phase)] = (grad, loss, stats)
    g0, l0, s0 = out[("whole", 0)]
    for key, (g, l, st) in out.items():
        assert torch.equal(l, l0) and torch.equal(st, s0), key
        assert torch.equal(g[off:], g0[off:]) if key[1] == 3 else torch.equal(g, g0), key
    return g0, l0, s0


def check_designed_ratios(arch_id, arch, A, B, clip, seed=5):
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    from test_hip_network import make_case
    params, states, idx, y, adv = make_case(arch, A, B, seed=seed)
    ctx = hip_ops.Context(arch_id, A, max_batch=B)
    p, s, acts = upload(ctx, params), dev(states), dev(idx)
    probs = torch.zeros((B, A), device="cuda")
    ctx.forward(p, s, probs=probs)
    ratios = RATIOS[np.random.RandomState(seed + 1).randint(0, 6, B)]
    p_old = (probs.cpu().numpy()[np.arange(B), idx].astype(np.float64) / ratios).astype(np.float32)
    assert (adv > 0).any() and (adv < 0).any()
    grad, loss, stats = ppo_all_routes(ctx, p, s, acts, dev(y), dev(adv), dev(p_old), clip, B)
    nconv = len(onet.ARCHS[arch][0])
    masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(nconv)}
    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
    ref = onet.forward(params, states, arch, dtype=np.float64)
    R = ppo_restated(ref["pi"], idx, adv, p_old, clip, 0.02)
    margin = np.minimum(np.abs(R["ratio"] / (1 + clip) - 1), np.abs(R["ratio"] / (1 - clip) - 1)).min()
    assert margin > 1e-3, margin                 # designed: the nearest ratio is 0.05 from a bound
    L, g_ref = onet.loss_and_grads(params, states, np.eye(A)[idx], y, R["adv_eff"].astype(np.float64), 0.02, arch,
                                   dtype=np.float64, relu_masks=masks)
    lo, st = loss.cpu().numpy(), stats.cpu().numpy()
    want_loss = 5.0 * (R["actor"] + L["critic"])
    print("%s A=%d B=%d clip=%g: loss %g / %g actor %g / %g clip_fraction %g / %g approx_kl %g / %g" %
          (arch, A, B, clip, lo[0], want_loss, lo[1], R["actor"], st[0], R["clip_fraction"], st[1], R["approx_kl"]))
    assert abs(lo[0] - want_loss) < 1e-4 * max(1.0, abs(want_loss))
    assert abs(lo[1] - R["actor"]) < 1e-4 * max(1.0, abs(R["actor"])) and abs(lo[2] - L["critic"]) < 1e-4 * max(1.0, abs(L["critic"]))
    assert abs(lo[3] - L["entropy"].mean()) < 1e-4
    assert st[0] == np.float32(np.float32(np.sum(~R["active"])) / np.float32(B)) and 0 < st[0] < 1
    assert abs(st[1] - R["approx_kl"]) < 1e-4 * max(1.0, abs(R["approx_kl"]))
    got, gn = unflatten(ctx, grad), onet.global_norm(g_ref)
    for name, want in g_ref.items():
        err, scale = np.abs(got[name] - want).max(), max(np.abs(want).max(), 1e-3 * gn)
        print("  %s: err / scale %.3g" % (name, err / scale))
        assert err / scale < 1e-4, "%s: max abs err %g (scale %g)" % (name, err, scale)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B,clip", [("NATURE", 4, 160, 0.2), ("NATURE", 18, 1280, 0.1), ("NIPS", 6, 40, 0.1),
                                           ("NIPS", 18, 160, 0.2), ("NATURE", 6, 2560, 0.2)])
def test_designed_ratios_against_the_restatement(arch, A, B, clip):
    check_designed_ratios(ARCH_ID[arch], arch, A, B, clip)


_USER_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from oracle import network as onet
from paac_amd import _lib, networks
CONVS, FC = [(16, 8, 4), (32, 4, 2), (32, 3, 1)], 256
onet.ARCHS["PPO_USER"] = (CONVS, FC)
networks.define_architecture("PPO_USER", CONVS, FC)
assert _lib.user_arch() == (CONVS, FC)
import test_ppo
test_ppo.check_designed_ratios(_lib.ARCH_USER, "PPO_USER", 4, 160, 0.2)
test_ppo.check_record_and_identity(_lib.ARCH_USER, "PPO_USER", 6, 40)
print("PPO_USER_OK")
"""


@pytest.mark.gpu
def test_designed_ratios_on_a_user_architecture():
    """A process holds one user geometry: the same checks in a child process, on the library built for 16,32,32,256."""
    res = subprocess.run([sys.executable, "-c", _USER_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "PPO_USER_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


def check_record_and_identity(arch_id, arch, A, B):
    """(2) the recording calls give paac_loss_backward's gradient and loss bit for bit and p_old == the training set's
    probability of the action taken; (3) the surrogate fed that p_old is the plain loss's gradient bit for bit, clips nothing,
    and measures a KL of exactly zero."""
    import torch
    from paac_amd import hip_ops
    from test_gae import records
    from test_hip_network import make_case
    T, N = 5, B // 5
    params, states, idx, y, adv = make_case(arch, A, B, seed=8)
    ctx = hip_ops.Context(arch_id, A, max_batch=B)
    p, s, acts, y, adv = upload(ctx, params), dev(states), dev(idx), dev(y), dev(adv)
    n = ctx.layout["total"]
    v_boot, r, m, V = [dev(a) for a in records(T, N, 4)]
    for route in ("whole", "trunk"):
        for phase in (0, 3):
            fwd = lambda: ctx.train_forward_trunk(p, s) if route == "trunk" else ctx.train_forward(p, s)
            g0, l0 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            fwd()
            ctx.loss_backward(p, s, acts, y, adv, 0.02, g0, l0, forward_done=True, phase=phase)
            g1, l1, p_old = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(B, device="cuda")
            fwd()
            ctx.loss_backward_record(p, s, acts, y, adv, p_old, 0.02, g1, l1, forward_done=True, phase=phase)
            torch.cuda.synchronize()
            probs = ctx.debug_activation(26, B).view(B, A)
            what = (arch, route, phase)
            assert torch.equal(g0, g1) and torch.equal(l0, l1), what
            assert torch.equal(p_old, probs[torch.arange(B), acts.long()]) and float(p_old.min()) > 0, what
            g2, l2, st = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.ones(2, device="cuda")
            fwd()
            ctx.loss_backward_ppo(p, s, acts, y, adv, p_old, 0.2, 0.02, g2, l2, st, forward_done=True, phase=phase)
            torch.cuda.synchronize()
            assert torch.equal(g0, g2), what
            assert torch.equal(l0[2:], l2[2:]) and st.cpu().tolist() == [0.0, 0.0], what
            # both estimators of the fused-returns entry with p_old_out set
            for lam in (None, 0.9):
                out = []
                for rec in (None, torch.zeros(B, device="cuda")):
                    yo, ao = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
                    g, l = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
                    fwd()
                    ctx.loss_backward_returns(p, s, acts, v_boot, r, m, V, 0.99, yo, ao, 0.02, g, l, forward_done=True,
                                              phase=phase, gae_lambda=lam, p_old_out=rec)
                    torch.cuda.synchronize()
                    out.append((g, l, yo, ao))
                assert all(torch.equal(a, b) for a, b in zip(*out)), (what, lam)
                assert torch.equal(rec, p_old), (what, lam)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B", [("NATURE", 4, 160), ("NATURE", 18, 40), ("NIPS", 6, 40), ("NATURE", 6, 1280)])
def test_recording_is_free_and_the_surrogate_at_ratio_one_is_the_plain_loss(arch, A, B):
    check_record_and_identity(ARCH_ID[arch], arch, A, B)


@pytest.mark.gpu
def test_entry_refuses_bad_clip_and_null_p_old():
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=8)
    n = ctx.layout["total"]
    p, g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    s = torch.zeros((8, 84, 84, 4), dtype=torch.uint8, device="cuda")
    a, z = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, device="cuda")
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(_lib.PaacHipError, match="paac_loss_backward_ppo: clip_eps"):
            ctx.loss_backward_ppo(p, s, a, z, z, z, bad, 0.02, g)
    rc = ctx.lib.paac_loss_backward_ppo(ctx.handle, p.data_ptr(), s.data_ptr(), a.data_ptr(), z.data_ptr(), z.data_ptr(), None,
                                        0.2, 8, 0.02, g.data_ptr(), None, None, 0, 0, None)
    assert rc < 0 and b"null p_old" in ctx.lib.paac_last_error()
    rc = ctx.lib.paac_loss_backward_record(ctx.handle, p.data_ptr(), s.data_ptr(), a.data_ptr(), z.data_ptr(), z.data_ptr(), None,
                                           8, 0.02, g.data_ptr(), None, 0, 0, None)
    assert rc < 0 and b"null p_old_out" in ctx.lib.paac_last_error()
    ctx.close()


# (4) natural ratios: params -> one real optimizer step -> the surrogate call.  A clip decision is discontinuous: a row whose
# float64 ratio lies within 1e-3 (relative) of 1 +- EPS could legitimately flip in float32 (the forward's 1e-5 bar is two
# decades below that margin).  The seeds below were chosen by running natural_case on the CPU: they produce no such row, the
# test asserts that and excludes nothing.
NATURAL = [("NIPS", 6, 40, 0.2, 3), ("NIPS", 4, 40, 0.1, 4)]


def natural_case(arch, A, B, clip, seed, lr=0.0224):
    """float64 oracle: (params, states, idx, y, adv, params after one clipped RMSProp step, pi before, pi after, restatement)."""
    from oracle import network as onet
    from test_hip_network import make_case
    params, states, idx, y, adv = make_case(arch, A, B, seed=seed, weight_scale=3.5)
    pi0 = onet.forward(params, states, arch, dtype=np.float64)["pi"]
    _, g = onet.loss_and_grads(params, states, np.eye(A)[idx], y, adv, 0.02, arch, dtype=np.float64)
    g, _ = onet.clip_by_global_norm(g, 3.0)
    ms, mom = onet.rmsprop_init(params)
    p1, _, _ = onet.rmsprop_step({k: v.astype(np.float64) for k, v in params.items()}, g, ms, mom, lr)
    p1 = {k: v.astype(np.float32) for k, v in p1.items()}
    pi1 = onet.forward(p1, states, arch, dtype=np.float64)["pi"]
    R = ppo_restated(pi1, idx, adv, pi0[np.arange(B), idx], clip, 0.02)
    margin = np.minimum(np.abs(R["ratio"] / (1 + clip) - 1), np.abs(R["ratio"] / (1 - clip) - 1))
    return params, states, idx, y, adv, p1, pi0, R, margin


@pytest.mark.parametrize("arch,A,B,clip,seed", NATURAL)
def test_natural_ratio_seeds_keep_every_row_away_from_the_clip_bounds(arch, A, B, clip, seed):
    R, margin = natural_case(arch, A, B, clip, seed)[-2:]
    assert (margin > 1e-3).all(), margin.min()
    assert 0 < R["clip_fraction"] < 1            # ... and the step really moved ratios across the bounds


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B,clip,seed", NATURAL)
def test_natural_ratios_after_one_real_step(arch, A, B, clip, seed):
    import torch
    from oracle import network as onet
    from paac_amd import _lib, hip_ops
    params, states, idx, y, adv, p1, pi0, R, margin = natural_case(arch, A, B, clip, seed)
    assert (margin > 1e-3).all(), margin.min()
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    p, s, acts, yd, ad = upload(ctx, params), dev(states), dev(idx), dev(y), dev(adv)
    n = ctx.layout["total"]
    grad, loss, p_old = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(B, device="cuda")
    ctx.loss_backward_record(p, s, acts, yd, ad, p_old, 0.02, grad, loss)
    ms, mom, lr = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), torch.tensor([0.0224], device="cuda")
    ctx.clip_rmsprop(p, grad, ms, mom, lr, 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)
    assert np.abs(p_old.cpu().numpy() - pi0[np.arange(B), idx]).max() < 1e-5
    stats = torch.zeros(2, device="cuda")
    ctx.train_forward_trunk(p, s)
    ctx.loss_backward_ppo(p, s, acts, yd, ad, p_old, clip, 0.02, grad, loss, stats, forward_done=True)
    torch.cuda.synchronize()
    stepped = unflatten(ctx, p)
    nconv = len(onet.ARCHS[arch][0])
    masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(nconv)}
    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
    # the restatement on the weights the device holds after its step, with the device's own p_old
    pi1 = onet.forward(stepped, states, arch, dtype=np.float64)["pi"]
    Rd = ppo_restated(pi1, idx, adv, p_old.cpu().numpy(), clip, 0.02)
    assert np.array_equal(Rd["active"], R["active"])
    L, g_ref = onet.loss_and_grads(stepped, states, np.eye(A)[idx], y, Rd["adv_eff"], 0.02, arch, dtype=np.float64,
                                   relu_masks=masks)
    lo, st = loss.cpu().numpy(), stats.cpu().numpy()
    print("natural %s A=%d: clip_fraction %g / %g approx_kl %g / %g actor %g / %g" %
          (arch, A, st[0], Rd["clip_fraction"], st[1], Rd["approx_kl"], lo[1], Rd["actor"]))
    assert st[0] == np.float32(np.float32(np.sum(~Rd["active"])) / np.float32(B))
    assert abs(st[1] - Rd["approx_kl"]) < 1e-4 * max(1.0, abs(Rd["approx_kl"]))
    assert abs(lo[1] - Rd["actor"]) < 1e-4 * max(1.0, abs(Rd["actor"])) and abs(lo[2] - L["critic"]) < 1e-4 * max(1.0, abs(L["critic"]))
    got, gn = unflatten(ctx, grad), onet.global_norm(g_ref)
    for name, want in g_ref.items():
        err, scale = np.abs(got[name] - want).max(), max(np.abs(want).max(), 1e-3 * gn)
        assert err / scale < 1e-4, "%s: max abs err %g (scale %g)" % (name, err, scale)
    ctx.close()


# -- GPU: the loops ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_one_epoch_is_the_default_in_both_loops():
    """--ppo_epochs 1 --ppo_clip 0.05 against the default run: weights and optimizer slots bit for bit after several cycles."""
    from test_gae import run_device_loop, run_host_loop
    a = run_device_loop(8, 5, "numpy", 4)
    b = run_device_loop(8, 5, "numpy", 4, ppo_epochs=1, ppo_clip=0.05)
    assert all(np.array_equal(x, y) for x, y in zip(a["state"], b["state"]))
    c = run_device_loop(8, 5, "numpy", 4, ppo_epochs=2)
    assert not np.array_equal(a["state"][0], c["state"][0])            # the flag reaches the update
    _, _, ha = run_host_loop(3)
    _, _, hb = run_host_loop(3, ppo_epochs=1, ppo_clip=0.05)
    assert all(np.array_equal(x, y) for x, y in zip(ha, hb))
    _, _, hc = run_host_loop(3, ppo_epochs=3)
    assert not np.array_equal(ha[0], hc[0]) and all(np.isfinite(x).all() for x in hc)


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(32, 5), (8, 20)])
@pytest.mark.parametrize("sampler", ["numpy", "philox"])
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_three_epochs_graph_replay_equals_eager(N, T, sampler, optimizer):
    from oracle import rollout as oroll
    from test_gae import run_device_loop
    cycles, K = 3, 3
    seen = []

    def check(learner, ro, c):
        seen.append((learner.ppo_stats.cpu().numpy().copy(), learner.ppo_loss.cpu().numpy().copy()))
        if optimizer == "adam":                  # Adam's powers advance K times per cycle
            want = np.float32(learner.beta1)
            for _ in range(K * (c + 1)):
                want = np.float32(want * np.float32(learner.beta1))
            assert learner.beta_powers.cpu().numpy()[0] == want

    flags = dict(ppo_epochs=K, optimizer=optimizer, gae_lambda=0.95)
    if optimizer == "adam":
        flags.update(e=1e-5, initial_lr=1e-4)
    graph = run_device_loop(N, T, sampler, cycles, use_graph=True, check=check, **flags)
    eager = run_device_loop(N, T, sampler, cycles, use_graph=False, **flags)
    assert all(np.array_equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    assert all(np.isfinite(a).all() for a in graph["state"])
    step = cycles * N * T                         # global_step, lr and the frame counter advance once per cycle
    assert graph["global_step"] == eager["global_step"] == step
    assert graph["lr"] == eager["lr"] == float(np.float32(oroll.get_lr(step, flags.get("initial_lr", 0.0224), 80000000)))
    for stats, losses in seen:
        assert (stats[0] == 0).all() and np.isfinite(stats).all() and np.isfinite(losses).all()
        assert (stats[1:, 0] >= 0).all() and (stats[1:, 0] <= 1).all() and (losses[1:, 3] > 0).all()


@pytest.mark.gpu
def test_device_cycle_equals_the_hand_composition(monkeypatch):
    """K = 3 in the device loop against the same cycle composed from the C entries on the loop's own rollout records: the
    recording paac_loss_backward_returns, the update, then K - 1 x (paac_train_forward_trunk + paac_loss_backward_ppo +
    update) -- y, adv, p_old, the per-epoch statistics, weights and optimizer slots bit for bit.  The composition's first
    forward is paac_train_forward_trunk, so the loop runs its recomputed-trunk route (PAAC_REUSE_ACTING=0; kept acting rows
    differ from a recomputed forward by the summation order, include/paac_hip.h -- that route is held to graph == eager)."""
    reuse = "0"
    import torch
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    from paac_amd.paac import DeviceRollout
    monkeypatch.setenv("PAAC_REUSE_ACTING", reuse)
    N, T, K = 32, 5, 3
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="philox", test_seed=11, ppo_epochs=K,
                     ppo_clip=0.1)
    L, _, env_creator = build_learner(args)
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", use_graph=True)
    ro.run_cycle()
    ro.synchronize()
    before = [t.clone() for _, t in L.update_state]
    ro.run_cycle()                                # parity 1: the cycle that is composed by hand below
    ro.synchronize()
    after = [t.clone() for _, t in L.update_state]
    stats, gs, lr = L.ppo_stats.clone(), int(ro.global_step_dev.item()), L.lr_dev.clone()
    assert gs == 2 * N * T and int(ro.tick.item()) == 2 * T
    # -- by hand, from the weights before that cycle and the records it left
    for (_, t), b in zip(L.update_state, before):
        t.copy_(b)
    L.ctx.pack_weights(L.network.params)
    p, B = L.network.params, T * N
    s_all = ro.states[T:2 * T + 1].view((T + 1) * N, 84, 84, 4)
    s, acts = s_all[:B], ro.actions.view(-1)
    y, adv, p_old = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    gstep, lr2 = torch.tensor([N * T], dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda")
    L.lr_dev.zero_()
    L.ctx.train_forward_trunk(p, s_all)
    L.ctx.loss_backward_returns(p, s, acts, None, ro.rewards, ro.masks, ro.values, L.gamma, y, adv, L.entropy_beta, L.grad,
                                L.loss_dev, forward_done=True, phase=3, global_step_dev=gstep, increment=N * T,
                                initial_lr=L.initial_lr, lr_annealing_steps=L.lr_annealing_steps, lr_out_dev=L.lr_dev,
                                p_old_out=p_old)
    L.apply_gradients()
    st = torch.zeros((K, 2), device="cuda")
    for k in range(1, K):
        L.ctx.train_forward_trunk(p, s)
        L.ctx.loss_backward_ppo(p, s, acts, y, adv, p_old, 0.1, L.entropy_beta, L.grad, L.loss_dev, st[k], forward_done=True,
                                phase=3)
        L.apply_gradients()
    torch.cuda.synchronize()
    assert torch.equal(L.lr_dev, lr) and int(gstep.item()) == gs
    assert torch.equal(y, ro.y) and torch.equal(adv, ro.adv) and torch.equal(p_old, L.p_old)
    assert torch.equal(st, stats)
    for (name, t), a in zip(L.update_state, after):
        assert torch.equal(t, a), name
    assert float(stats[1:, 1].abs().max()) > 0     # epochs 2 and 3 moved the policy
    ro.close()


@pytest.mark.gpu
def test_metrics_carry_one_record_per_epoch(tmp_path):
    import json
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    N, T, K = 32, 5, 3
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=64 * N * T, synthetic_terminal_p=0.1, sampler="philox", ppo_epochs=K,
                     debugging_folder=str(tmp_path))
    L, _, _ = build_learner(args)
    L.train()
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    epochs = [r for r in recs if r.get("ppo_epoch") is not None or r.get("kind") == "ppo_epoch" or "clip_fraction" in r]
    assert len(epochs) == K and sorted(r["epoch"] for r in epochs) == [1, 2, 3]
    first = [r for r in epochs if r["epoch"] == 1][0]
    assert first["clip_fraction"] == 0.0 and first["approx_kl"] == 0.0
    assert all(0.0 <= r["clip_fraction"] <= 1.0 and np.isfinite(r["approx_kl"]) and np.isfinite(r["loss"]) for r in epochs)
