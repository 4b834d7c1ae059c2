"""--ppo_vclip EPSV: the PPO2 critic term (value clipping) of epochs 2..K.  The reference has no PPO, so the checker is this
file's float64 restatement of the contract in include/paac_hip.h, on top of tests/test_ppo.py's restatement of the actor term.
A value-clipped row's critic gradient is zero, which is the reference loss's critic gradient at the target y = v, so the
gradients still come from the unmodified oracle; the critic scalar and value_clip_fraction are restated here.  Bars are
tests/test_ppo.py's for the same shapes: 1e-4 of max(|want|.max(), 1e-3 * global norm) per tensor, 1e-4 on the loss scalars;
the two clip fractions are counts over B and must be exact.

The designed rows (kind = row % 4), with d = v - v_old:
  0  unclipped: v_old = v * (1 - 2^-6), so |d| < EPSV for |v| < 12.8 and d is exact (v and v_old lie within a factor of two:
     Sterbenz), hence vc == v and l2 == l1 to the bit in fp32 and in fp64 alike -- the tie the contract resolves to "not clipped"
  1  clipped above: v_old = v - 2 EPSV, y = v + 1: vc = v - EPSV, l2 = (1 + EPSV)^2 > l1 = 1: no critic gradient
  2  clipped below: v_old = v + 2 EPSV, y = v - 1: the mirror image
  3  clamp active, l1 > l2: v_old = v - 2 EPSV, y = v - 1: l2 = (1 - EPSV)^2 < 1: the gradient still flows
Every decision but kind 0's has a margin of EPSV = 0.2, five decades above the forward's 1e-5 bar."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARCH_ID = {"NIPS": 0, "NATURE": 1}
EPSV = 0.2


# -- the restatement ---------------------------------------------------------------------------------------------------

def vclip_restated(v, v_old, y, epsv):
    """float64 -> dict(vclipped, clamped, critic (mean), value_clip_fraction)."""
    v, v_old, y = [np.asarray(a).astype(np.float64) for a in (v, v_old, y)]
    vc = v_old + np.clip(v - v_old, -epsv, epsv)
    l1, l2 = (y - v) ** 2, (y - vc) ** 2
    vclipped = l2 > l1
    return dict(vclipped=vclipped, clamped=np.abs(v - v_old) > epsv, critic=np.mean(0.25 * np.maximum(l1, l2)),
                value_clip_fraction=np.mean(vclipped))


def restated_loss(logits, v, idx, y, adv, p_old, v_old, clip, epsv, beta):
    from test_ppo import ppo_restated
    z = logits - logits.max(axis=1, keepdims=True)
    pi = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    return 5.0 * (ppo_restated(pi, idx, adv, p_old, clip, beta)["actor"] + vclip_restated(v, v_old, y, epsv)["critic"])


def restated_head_grads(logits, v, idx, y, adv, p_old, v_old, clip, epsv, beta):
    """The oracle's head gradients at the effective advantage (test_ppo) and, for a value-clipped row, at the target y = v."""
    import test_ppo
    y_eff = np.where(vclip_restated(v, v_old, y, epsv)["vclipped"], v, y)
    return test_ppo.restated_head_grads(logits, v, idx, y_eff, adv, p_old, clip, beta)


def design_rows(v, y, epsv):
    """(v_old fp32, y fp32, kind) of the designed rows for the values `v` (the module docstring has the table)."""
    v = np.asarray(v, dtype=np.float32)
    kind = np.arange(v.size) % 4
    e = np.float32(epsv)
    v_old = np.select([kind == 0, kind == 2], [v * np.float32(1.0 - 2.0 ** -6), v + 2 * e], v - 2 * e).astype(np.float32)
    y = np.select([kind == 0, kind == 1], [np.asarray(y, dtype=np.float32), v + 1], v - 1).astype(np.float32)
    return v_old, y, kind


def assert_designed(R, kind):
    """The restatement alone must see every kind where it was designed (a case it would leave without one is a bad case)."""
    assert all((kind == k).sum() >= 1 for k in range(4))
    assert np.array_equal(R["vclipped"], (kind == 1) | (kind == 2))
    assert np.array_equal(R["clamped"], kind != 0)


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_flag_defaults_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    assert p.parse_args([]).ppo_vclip == 0.0
    a = p.parse_args(["--ppo_vclip", "0.2", "--ppo_epochs", "4"])
    assert a.ppo_vclip == 0.2
    assert ("--ppo_vclip",) in {f[0] for f in train.BUILD_FLAGS}
    logger_utils.save_args(a, str(tmp_path))
    assert logger_utils.load_args(str(tmp_path / "args.json"))["ppo_vclip"] == 0.2


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf")])
def test_actor_learner_refuses_bad_values(bad):
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    args.ppo_vclip = bad
    args.num_actions = 4
    with pytest.raises(ValueError, match="ppo_vclip"):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_header_declares_the_entry():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    m = re.search(r"int\s+paac_loss_backward_ppo_vclip\s*\(([^;]*)\);", hdr)
    assert m, "paac_loss_backward_ppo_vclip missing from the header"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["paac_loss_backward_ppo_vclip"][1]) == 18
    for t in ("const float* p_old", "const float* v_old", "float clip_eps", "float vclip_eps", "float* ppo_stats_out",
              "int forward_done", "int phase"):
        assert t in m.group(1), t
    assert "paac_loss_backward_ppo_vclip" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGNATURES["paac_loss_backward_ppo"][1]) == 16          # the entry without the term is unchanged
    for text in ("vc = v_old + fminf(fmaxf(v - v_old, -EPSV), EPSV)", "vclipped = l2 > l1", "0.25 * fmaxf(l1, l2)",
                 "dv = vclipped ? 0 : s*0.5*(v - y)", "value_clip_fraction"):
        assert text in hdr, text


def designed_heads_case(B, A, seed):
    from test_ppo import RATIOS, heads_case
    logits, v, pi, idx, y, adv = heads_case(B, A, seed)
    v = v.astype(np.float32).astype(np.float64)
    v_old, y, kind = design_rows(v, y, EPSV)
    p_old = pi[np.arange(B), idx] / RATIOS[np.arange(B) % 6]
    return logits, v, pi, idx, y.astype(np.float64), adv, p_old, v_old.astype(np.float64), kind


def test_designed_rows_contain_every_kind():
    logits, v, pi, idx, y, adv, p_old, v_old, kind = designed_heads_case(48, 6, 2)
    R = vclip_restated(v, v_old, y, EPSV)
    assert_designed(R, kind)
    assert R["value_clip_fraction"] == 0.5
    # kind 0's tie is exact: vc == v to the bit, in fp64 and in fp32
    z = kind == 0
    assert np.array_equal((v_old + np.clip(v - v_old, -EPSV, EPSV))[z], v[z])
    v32, o32 = v.astype(np.float32), v_old.astype(np.float32)
    assert np.array_equal((o32 + np.clip(v32 - o32, np.float32(-EPSV), np.float32(EPSV)))[z], v32[z])


def test_restated_gradient_is_the_derivative_of_the_restated_loss():
    """Central differences in float64, step 1e-6: truncation ~ 1e-12, cancellation ~ 1e-10 of the loss; bar 1e-7 absolute
    (tests/test_ppo.py's reasoning).  Every designed decision has a margin far above the step; kind 0's tie stays a tie at
    v +- h (d stays exact)."""
    B, A, clip, beta, h = 48, 6, 0.2, 0.02, 1e-6
    logits, v, pi, idx, y, adv, p_old, v_old, kind = designed_heads_case(B, A, 2)
    assert_designed(vclip_restated(v, v_old, y, EPSV), kind)
    dlogits, dv = restated_head_grads(logits, v, idx, y, adv, p_old, v_old, clip, EPSV, beta)
    assert not dv[(kind == 1) | (kind == 2)].any() and (dv[(kind == 0) | (kind == 3)] != 0).all()
    f = lambda lg, vv: restated_loss(lg, vv, idx, y, adv, p_old, v_old, clip, EPSV, beta)
    for i in range(B):
        vp, vm = v.copy(), v.copy()
        vp[i] += h
        vm[i] -= h
        q = (f(logits, vp) - f(logits, vm)) / (2 * h)
        assert abs(q - dv[i]) < 1e-7, (i, kind[i], q, dv[i])
        for a in range(A):
            lp, lm = logits.copy(), logits.copy()
            lp[i, a] += h
            lm[i, a] -= h
            q = (f(lp, v) - f(lm, v)) / (2 * h)
            assert abs(q - dlogits[i, a]) < 1e-7, (i, a, q, dlogits[i, a])


def test_with_v_old_equal_v_the_restatement_is_test_ppos():
    import test_ppo
    B, A = 64, 6
    logits, v, pi, idx, y, adv, p_old, _, _ = designed_heads_case(B, A, 1)
    R = vclip_restated(v, v, y, EPSV)
    assert not R["vclipped"].any() and not R["clamped"].any() and R["value_clip_fraction"] == 0.0
    assert R["critic"] == np.mean(0.25 * (y - v) ** 2)
    got = restated_head_grads(logits, v, idx, y, adv, p_old, v, 0.2, EPSV, 0.02)
    want = test_ppo.restated_head_grads(logits, v, idx, y, adv, p_old, 0.2, 0.02)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert restated_loss(logits, v, idx, y, adv, p_old, v, 0.2, EPSV, 0.02) == test_ppo.restated_loss(logits, v, idx, y, adv, p_old, 0.2, 0.02)


# -- GPU: kernel level -------------------------------------------------------------------------------------------------

def vclip_all_routes(ctx, p, s, acts, y, adv, p_old, v_old, clip, epsv):
    """paac_loss_backward_ppo_vclip on every route and phase tests/test_ppo.py:ppo_all_routes covers -> (grad, loss, stats) of
    phase 0 after a whole forward; asserts the others equal it bit for bit."""
    import torch
    n = ctx.layout["total"]
    off = [t for t in ctx.layout["tensors"] if t["name"].startswith("fc")][0]["offset"]
    out = {}
    for route in ("whole", "trunk"):
        for phase in (0, 12, 3):
            grad, loss, stats = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda")
            if route == "trunk":
                ctx.train_forward_trunk(p, s)
            else:
                ctx.train_forward(p, s)
            ctx.loss_backward_ppo_vclip(p, s, acts, y, adv, p_old, v_old, clip, epsv, 0.02, grad, loss, stats, forward_done=True,
                                        phase=1 if phase == 12 else phase)
            if phase == 12:
                ctx.loss_backward_ppo_vclip(p, s, acts, y, adv, p_old, v_old, clip, epsv, 0.02, grad, loss, None,
                                            forward_done=True, phase=2)
            torch.cuda.synchronize()
            out[(route, phase)] = (grad, loss, stats)
    g0, l0, s0 = out[("whole", 0)]
    for key, (g, l, st) in out.items():
        assert torch.equal(l, l0) and torch.equal(st, s0), key
        assert torch.equal(g[off:], g0[off:]) if key[1] == 3 else torch.equal(g, g0), key
    return g0, l0, s0


def check_designed_rows(arch_id, arch, A, B, clip, seed=5):
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    from test_hip_network import make_case
    from test_ppo import RATIOS, dev, ppo_restated, unflatten, upload
    params, states, idx, y, adv = make_case(arch, A, B, seed=seed)
    ctx = hip_ops.Context(arch_id, A, max_batch=B)
    p, s, acts = upload(ctx, params), dev(states), dev(idx)
    probs, values = torch.zeros((B, A), device="cuda"), torch.zeros(B, device="cuda")
    ctx.forward(p, s, probs=probs, values=values)
    ratios = RATIOS[np.random.RandomState(seed + 1).randint(0, 6, B)]
    p_old = (probs.cpu().numpy()[np.arange(B), idx].astype(np.float64) / ratios).astype(np.float32)
    v_old, y, kind = design_rows(values.cpu().numpy(), y, EPSV)
    assert np.abs(values.cpu().numpy()).max() < 12.8
    grad, loss, stats = vclip_all_routes(ctx, p, s, acts, dev(y), dev(adv), dev(p_old), dev(v_old), clip, EPSV)
    nconv = len(onet.ARCHS[arch][0])
    masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(nconv)}
    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
    ref = onet.forward(params, states, arch, dtype=np.float64)
    R = ppo_restated(ref["pi"], idx, adv, p_old, clip, 0.02)
    Rv = vclip_restated(ref["v"], v_old, y, EPSV)
    # kind 0's tie is a tie for the values the device holds (d exact); the oracle's fp64 values are not fp32 numbers, so the
    # restatement decides kind 0 from the device's values and every other kind from its own (margin 0.2 against a 1e-5 bar)
    v_dev = ctx.debug_activation(25, B).cpu().numpy()
    Rd = vclip_restated(v_dev, v_old, y, EPSV)
    assert_designed(Rd, kind)
    assert np.array_equal(Rv["vclipped"][kind != 0], Rd["vclipped"][kind != 0]) and np.array_equal(Rv["clamped"], Rd["clamped"])
    vclipped = Rd["vclipped"]
    y_eff = np.where(vclipped, ref["v"], y.astype(np.float64))
    L, g_ref = onet.loss_and_grads(params, states, np.eye(A)[idx], y_eff, R["adv_eff"].astype(np.float64), 0.02, arch,
                                   dtype=np.float64, relu_masks=masks)
    vv, yy, oo = ref["v"].astype(np.float64), y.astype(np.float64), v_old.astype(np.float64)
    l1, l2 = (yy - vv) ** 2, (yy - (oo + np.clip(vv - oo, -EPSV, EPSV))) ** 2
    want_critic = np.mean(0.25 * np.where(kind == 0, l1, np.maximum(l1, l2)))
    lo, st = loss.cpu().numpy(), stats.cpu().numpy()
    want_loss = 5.0 * (R["actor"] + want_critic)
    print("%s A=%d B=%d: loss %g / %g actor %g / %g critic %g / %g clip_fraction %g / %g value_clip_fraction %g / %g" %
          (arch, A, B, lo[0], want_loss, lo[1], R["actor"], lo[2], want_critic, st[0], R["clip_fraction"], st[2], vclipped.mean()))
    assert abs(lo[0] - want_loss) < 1e-4 * max(1.0, abs(want_loss))
    assert abs(lo[1] - R["actor"]) < 1e-4 * max(1.0, abs(R["actor"])) and abs(lo[2] - want_critic) < 1e-4 * max(1.0, abs(want_critic))
    assert st[0] == np.float32(np.float32(np.sum(~R["active"])) / np.float32(B)) and 0 < st[0] < 1
    assert abs(st[1] - R["approx_kl"]) < 1e-4 * max(1.0, abs(R["approx_kl"]))
    assert st[2] == np.float32(np.float32(((kind == 1) | (kind == 2)).sum()) / np.float32(B))      # the designed count / B
    got, gn = unflatten(ctx, grad), onet.global_norm(g_ref)
    for name, want in g_ref.items():
        err, scale = np.abs(got[name] - want).max(), max(np.abs(want).max(), 1e-3 * gn)
        print("  %s: err / scale %.3g" % (name, err / scale))
        assert err / scale < 1e-4, "%s: max abs err %g (scale %g)" % (name, err, scale)
    # with v_old = the ctx's own values the term is inert: paac_loss_backward_ppo's gradient, loss and statistics bit for bit
    n = ctx.layout["total"]
    yd, ad, pd = dev(y), dev(adv), dev(p_old)
    for route, phase in (("whole", 0), ("trunk", 3)):
        fwd = lambda: ctx.train_forward_trunk(p, s) if route == "trunk" else ctx.train_forward(p, s)
        g0, l0, s0 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
        fwd()
        ctx.loss_backward_ppo(p, s, acts, yd, ad, pd, clip, 0.02, g0, l0, s0, forward_done=True, phase=phase)
        own = torch.zeros(B, device="cuda")
        ctx.train_values_into(own, B)
        assert torch.equal(own, ctx.debug_activation(25, B))
        g1, l1_, s1 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.ones(3, device="cuda")
        fwd()
        ctx.loss_backward_ppo_vclip(p, s, acts, yd, ad, pd, own, clip, EPSV, 0.02, g1, l1_, s1, forward_done=True, phase=phase)
        torch.cuda.synchronize()
        assert torch.equal(g0, g1) and torch.equal(l0, l1_), (arch, route, phase)
        assert torch.equal(s0, s1[:2]) and float(s1[2]) == 0.0, (arch, route, phase)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B,clip", [("NATURE", 4, 160, 0.2), ("NIPS", 6, 40, 0.1), ("NATURE", 18, 1280, 0.1)])
def test_designed_rows_against_the_restatement(arch, A, B, clip):
    check_designed_rows(ARCH_ID[arch], arch, A, B, clip)


_USER_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from oracle import network as onet
from paac_amd import _lib, networks
CONVS, FC = [(16, 8, 4), (32, 4, 2), (32, 3, 1)], 256
onet.ARCHS["VCLIP_USER"] = (CONVS, FC)
networks.define_architecture("VCLIP_USER", CONVS, FC)
assert _lib.user_arch() == (CONVS, FC)
import test_ppo_vclip
test_ppo_vclip.check_designed_rows(_lib.ARCH_USER, "VCLIP_USER", 4, 160, 0.2)
print("VCLIP_USER_OK")
"""


@pytest.mark.gpu
def test_designed_rows_on_a_user_architecture():
    """A process holds one user geometry: the same checks in a child process, on the library built for 16,32,32,256."""
    res = subprocess.run([sys.executable, "-c", _USER_CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "VCLIP_USER_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


@pytest.mark.gpu
def test_entry_refuses_bad_vclip_and_null_v_old():
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=8)
    n = ctx.layout["total"]
    p, g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    s = torch.zeros((8, 84, 84, 4), dtype=torch.uint8, device="cuda")
    a, z = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, device="cuda")
    for bad in (0.0, -0.1, float("nan")):
        with pytest.raises(_lib.PaacHipError, match="paac_loss_backward_ppo_vclip: vclip_eps"):
            ctx.loss_backward_ppo_vclip(p, s, a, z, z, z, z, 0.2, bad, 0.02, g)
    with pytest.raises(_lib.PaacHipError, match="paac_loss_backward_ppo_vclip: clip_eps"):
        ctx.loss_backward_ppo_vclip(p, s, a, z, z, z, z, 1.5, 0.2, 0.02, g)
    with pytest.raises(_lib.PaacHipError, match="null v_old"):
        ctx.loss_backward_ppo_vclip(p, s, a, z, z, z, None, 0.2, 0.2, 0.02, g)
    with pytest.raises(_lib.PaacHipError, match="null p_old"):
        ctx.loss_backward_ppo_vclip(p, s, a, z, z, None, z, 0.2, 0.2, 0.02, g)
    ctx.close()


# -- GPU: the loops, both flags on -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(32, 5), (8, 20)])
@pytest.mark.parametrize("sampler", ["numpy", "philox"])
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_both_flags_graph_replay_equals_eager(N, T, sampler, optimizer):
    from test_gae import run_device_loop
    cycles, K = 3, 3
    seen = []

    def check(learner, ro, c):
        seen.append((learner.ppo_stats.cpu().numpy().copy(), learner.adv_stats.cpu().numpy().copy()))

    flags = dict(ppo_epochs=K, optimizer=optimizer, gae_lambda=0.95, adv_norm=True, ppo_vclip=0.05)
    if optimizer == "adam":
        flags.update(e=1e-5, initial_lr=1e-4)
    graph = run_device_loop(N, T, sampler, cycles, use_graph=True, check=check, **flags)
    eager = run_device_loop(N, T, sampler, cycles, use_graph=False, **flags)
    assert all(np.array_equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    assert all(np.isfinite(a).all() for a in graph["state"])
    assert graph["global_step"] == eager["global_step"] == cycles * N * T and graph["lr"] == eager["lr"]
    for stats, norm in seen:
        assert stats.shape == (K, 3) and (stats[0] == 0).all() and np.isfinite(stats).all()
        assert (stats[1:, 2] >= 0).all() and (stats[1:, 2] <= 1).all() and norm[1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["device", "host"])
def test_cycle_equals_the_hand_composition(monkeypatch, loop):
    """Both flags and K = 3 against the same cycle composed from the C entries on the loop's own records: training forward,
    paac_returns_norm_tick (device loop; host loop: the returns entry + paac_adv_normalize), the recording backward on (y,
    adv_n), v_old out of the ctx, the update, then K - 1 x (trunk forward + paac_loss_backward_ppo_vclip + update) -- y, adv,
    adv_n, p_old, v_old, the per-epoch statistics, weights and optimizer slots bit for bit.  (Device loop on its
    recomputed-trunk route, like tests/test_ppo.py's composition.)"""
    import torch
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    from paac_amd import hip_ops
    from paac_amd.paac import DeviceRollout
    monkeypatch.setenv("PAAC_REUSE_ACTING", "0")
    K, clip, epsv = 3, 0.1, 0.05
    flags = dict(ppo_epochs=K, ppo_clip=clip, ppo_vclip=epsv, adv_norm=True, gae_lambda=0.95)
    if loop == "device":
        N, T = 32, 5
        args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                         max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="philox", test_seed=11, **flags)
        L, _, env_creator = build_learner(args)
        L.global_step = L.init_network()
        ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", use_graph=True)
        ro.run_cycle()
        ro.synchronize()
        before = [t.clone() for _, t in L.update_state]
        ro.run_cycle()                                # parity 1: the cycle that is composed by hand below
        ro.synchronize()
        s_all = ro.states[T:2 * T + 1].view((T + 1) * N, 84, 84, 4)
        s, acts = s_all[:T * N], ro.actions.view(-1)
        rec = dict(r=ro.rewards, m=ro.masks, V=ro.values, y=ro.y, adv=ro.adv)
        gs = int(ro.global_step_dev.item())
        assert gs == 2 * N * T
    else:
        N, T = 8, 5
        feeds, befores = [], []
        args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                         max_global_steps=2 * N * T, host_environments=True, record_feeds=True, synthetic_terminal_p=0.1,
                         test_seed=42, **flags)
        L, _, _ = build_learner(args)
        args.feed_callback = feeds.append
        # the weights each cycle starts from: the bench hook runs once per finished cycle
        args.cycle_callback = lambda step: befores.append([t.clone() for _, t in L.update_state])
        np.random.seed(args.test_seed)
        L.train()
        assert len(feeds) == 2
        before = befores[0]
        f = feeds[1]
        dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        s, acts = dev(f["states"]), dev(f["actions"])
        rec = dict(r=dev(f["rewards"]), m=dev(f["masks"]), V=dev(f["values"]), y=dev(f["y"]).view(-1), adv=dev(f["adv"]).view(-1),
                   v_boot=dev(f["v_boot"]), lr=float(np.float32(f["lr"])))
    after = [t.clone() for _, t in L.update_state]
    stats, losses, lr = L.ppo_stats.clone(), L.ppo_loss.clone(), L.lr_dev.clone()
    want = dict(adv_n=L.adv_n.clone(), p_old=L.p_old.clone(), v_old=L.v_old.clone(), adv_stats=L.adv_stats.clone())
    # -- by hand, from the weights before that cycle and the records it left
    for (_, t), b in zip(L.update_state, before):
        t.copy_(b)
    L.ctx.pack_weights(L.network.params)
    p, B = L.network.params, T * N
    y, adv, adv_n, p_old, v_old = [torch.zeros(B, device="cuda") for _ in range(5)]
    nstats = torch.zeros(2, dtype=torch.float64, device="cuda")
    if loop == "device":
        gstep = torch.tensor([N * T], dtype=torch.int64, device="cuda")
        L.lr_dev.zero_()
        L.ctx.train_forward_trunk(p, s_all)
        L.ctx.returns_norm_tick(p, None, rec["r"], rec["m"], rec["V"], L.gamma, y, adv, adv_n, nstats, global_step_dev=gstep,
                                increment=N * T, initial_lr=L.initial_lr, lr_annealing_steps=L.lr_annealing_steps,
                                lr_out_dev=L.lr_dev, gae_lambda=0.95)
        L.ctx.loss_backward_record(p, s, acts, y, adv_n, p_old, L.entropy_beta, L.grad, L.loss_dev, forward_done=True, phase=3)
        phase = 3
    else:
        hip_ops.returns(rec["v_boot"], rec["r"], rec["m"], rec["V"], L.gamma, y, adv, 0.95)
        hip_ops.adv_normalize(adv, adv_n, nstats)
        L.lr_dev.fill_(rec["lr"])
        L.ctx.loss_backward_record(p, s, acts, y, adv_n, p_old, L.entropy_beta, L.grad, L.loss_dev)
        phase = 0
    L.ctx.train_values_into(v_old, B)
    assert torch.equal(v_old, L.ctx.debug_activation(25, B))          # v_old == paac_debug_activation(25) right after epoch 1
    L.apply_gradients()
    st = torch.zeros((K, 3), device="cuda")
    for k in range(1, K):
        L.ctx.train_forward_trunk(p, s)
        L.ctx.loss_backward_ppo_vclip(p, s, acts, y, adv_n, p_old, v_old, clip, epsv, L.entropy_beta, L.grad, L.loss_dev, st[k],
                                      forward_done=True, phase=phase)
        L.apply_gradients()
    torch.cuda.synchronize()
    assert torch.equal(L.lr_dev, lr)
    assert torch.equal(y, rec["y"]) and torch.equal(adv, rec["adv"])          # the recorded arrays are the raw ones
    assert torch.equal(adv_n, want["adv_n"]) and torch.equal(nstats, want["adv_stats"]) and not torch.equal(adv_n, adv)
    assert torch.equal(p_old, want["p_old"]) and torch.equal(v_old, want["v_old"])
    assert torch.equal(st, stats) and torch.equal(L.loss_dev, losses[K - 1])
    for (name, t), a in zip(L.update_state, after):
        assert torch.equal(t, a), name
    assert float(stats[1:, 1].abs().max()) > 0     # epochs 2 and 3 moved the policy
    if loop == "device":
        ro.close()


@pytest.mark.gpu
@pytest.mark.parametrize("epsv", [0.0, 0.05])
def test_metrics_carry_value_clip_fraction_only_with_the_flag(tmp_path, epsv):
    import json
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    N, T, K = 32, 5, 3
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=64 * N * T, synthetic_terminal_p=0.1, sampler="philox", ppo_epochs=K, ppo_vclip=epsv,
                     debugging_folder=str(tmp_path))
    L, _, _ = build_learner(args)
    L.train()
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    epochs = [r for r in recs if r.get("kind") == "ppo_epoch"]
    assert len(epochs) == K and not [r for r in recs if r.get("kind") == "adv_norm"]
    assert all({"epoch", "loss", "actor_loss", "critic_loss", "entropy", "clip_fraction", "approx_kl"} <= set(r) for r in epochs)
    assert all(("value_clip_fraction" in r) == (epsv > 0) for r in epochs)
    if epsv > 0:
        assert [r for r in epochs if r["epoch"] == 1][0]["value_clip_fraction"] == 0.0
        assert all(0.0 <= r["value_clip_fraction"] <= 1.0 for r in epochs)
