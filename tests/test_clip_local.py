"""--clip_norm_type local: tf.clip_by_norm of every variable's gradient on its own (weights and biases separately), then
the unchanged TF RMSProp; global_norm is the norm of the CLIPPED gradients (actor_learner.py:62-64).  Upstream's branch
cannot run -- it hands each (grad, var) tuple to tf.clip_by_norm -- so the checker below is this file's own fp64
restatement of the branch's evident intent, not oracle/network.py (whose clip_by_global_norm refuses 'local')."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH_ID = {"NIPS": 0, "NATURE": 1}


def clip_by_norm_local(grads, clip_norm):
    """TF 1.0.1 clip_ops.clip_by_norm per variable, in fp64:
        l2norm_inv = rsqrt(reduce_sum(t * t)); t * clip_norm * minimum(l2norm_inv, 1.0 / clip_norm)
    then tf.global_norm of the clipped list.  -> (clipped {name: array}, factors {name: f}, clipped global norm).
    A zero tensor: rsqrt(0) = inf, the minimum picks 1 / clip_norm, f = 1."""
    out, factors = {}, {}
    for k, g in grads.items():
        g = np.asarray(g, dtype=np.float64)
        ss = float((g * g).sum())
        inv = np.inf if ss == 0.0 else 1.0 / np.sqrt(ss)
        factors[k] = clip_norm * min(inv, 1.0 / clip_norm)
        out[k] = g * factors[k]
    return out, factors, float(np.sqrt(sum(float((v * v).sum()) for v in out.values())))


def rmsprop_fp64(var, g, ms, mom, lr, decay, momentum, eps):
    """TF ApplyRMSProp (actor_learner.py:31-34) in fp64 on flat arrays."""
    ms_e = ms + (g * g - ms) * (1.0 - decay)
    mom_e = momentum * mom.astype(np.float64) + lr * g / np.sqrt(ms_e + eps)
    return var - mom_e, ms_e, mom_e


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_accepts_local():
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--clip_norm_type", "local"])
    assert args.clip_norm_type == "local"


def test_header_enum_matches_lib():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    m = re.search(r"enum\s*\{\s*PAAC_CLIP_IGNORE\s*=\s*(\d+),\s*PAAC_CLIP_GLOBAL\s*=\s*(\d+),\s*PAAC_CLIP_LOCAL\s*=\s*(\d+)\s*\}", hdr)
    assert m, "PAAC_CLIP_LOCAL missing from the header's clip enum"
    assert tuple(int(x) for x in m.groups()) == (_lib.CLIP_IGNORE, _lib.CLIP_GLOBAL, _lib.CLIP_LOCAL) == (0, 1, 2)
    assert "paac_grad_tensor_stats" in _lib.EXPORTED_SYMBOLS


def test_restatement_factors():
    rs = np.random.RandomState(0)
    g = {"zero": np.zeros(7), "small": rs.randn(50) * 1e-3, "large": rs.randn(50) * 10.0}
    clipped, f, gn = clip_by_norm_local(g, 3.0)
    assert f["zero"] == 1.0 and f["small"] == 1.0
    assert np.array_equal(clipped["small"], g["small"]) and not np.any(clipped["zero"])
    assert abs(np.linalg.norm(clipped["large"]) - 3.0) < 1e-12
    assert abs(gn - np.sqrt(9.0 + np.sum(g["small"] ** 2))) < 1e-12


# -- GPU: the optimizer step on its own --------------------------------------------------------------------------------

# target norm of each tensor's gradient after grad_scale, as a multiple of clip_norm (0: the tensor is exactly zero)
NORM_PATTERN = (4.0, 0.3, 0.0, 2.5, 0.6, 1.7, 0.2, 3.0, 0.5, 8.0, 0.05, 1.3)


def local_gradient(ctx, clip_norm, gscale, seed):
    """Flat gradient whose tensors sit above, below and at zero relative to clip_norm (after gscale)."""
    lay = ctx.layout
    rs = np.random.RandomState(seed)
    flat = np.zeros(lay["total"], dtype=np.float32)
    for i, t in enumerate(lay["tensors"]):
        v = rs.randn(t["size"])
        want = NORM_PATTERN[i % len(NORM_PATTERN)] * clip_norm / gscale
        flat[t["offset"]:t["offset"] + t["size"]] = (v * want / np.linalg.norm(v)).astype(np.float32)
    return flat


def split(ctx, flat):
    return {t["name"]: np.asarray(flat[t["offset"]:t["offset"] + t["size"]], dtype=np.float64) for t in ctx.layout["tensors"]}


def check_local_step(ctx, gscale, momentum, seed=3):
    """ctx.clip_rmsprop(..., CLIP_LOCAL) against the fp64 restatement + TF RMSProp (bars of test_clip_rmsprop_parity)."""
    import torch
    from paac_amd import _lib
    n = ctx.layout["total"]
    clip_norm = 0.5
    rs = np.random.RandomState(seed)
    var = rs.randn(n).astype(np.float32) * 0.1
    g = local_gradient(ctx, clip_norm, gscale, seed + 1)
    ms = (1.0 + rs.rand(n)).astype(np.float32)
    mom = (rs.randn(n) * 1e-3).astype(np.float32)
    lr = np.float32(0.0224)
    dv, dg, dms, dmom = [torch.from_numpy(a.copy()).cuda() for a in (var, g, ms, mom)]
    gn_dev = torch.zeros(1, device="cuda")
    ctx.clip_rmsprop(dv, dg, dms, dmom, torch.tensor([lr], device="cuda"), 0.99, momentum, 0.1, clip_norm, _lib.CLIP_LOCAL,
                     gscale, gn_dev)
    ts = ctx.grad_tensor_stats()
    torch.cuda.synchronize()
    clipped, f, gn = clip_by_norm_local({k: v * gscale for k, v in split(ctx, g).items()}, clip_norm)
    fs = np.array(list(f.values()))
    # the mix the test is about: clipped tensors, tensors under the bound, an all-zero one
    assert (fs < 0.99).sum() >= 3 and (fs == 1.0).sum() >= 3
    assert any(not np.any(g[t["offset"]:t["offset"] + t["size"]]) for t in ctx.layout["tensors"])
    gc = np.zeros(n)
    for t in ctx.layout["tensors"]:
        gc[t["offset"]:t["offset"] + t["size"]] = clipped[t["name"]].reshape(-1)
    var_e, ms_e, mom_e = rmsprop_fp64(var, gc, ms, mom, lr, 0.99, momentum, 0.1)
    assert abs(gn_dev.item() - gn) / gn < 1e-5
    assert np.abs(dms.cpu().numpy() - ms_e).max() < 1e-6
    assert np.abs(dmom.cpu().numpy() - mom_e).max() < 1e-7
    assert np.abs(dv.cpu().numpy() - var_e).max() < 1e-6
    assert np.all(np.isfinite(ts)) and np.abs(ts[:, 5] - fs).max() < 1e-5 * fs.max()
    raw = split(ctx, g)
    for i, t in enumerate(ctx.layout["tensors"]):
        ss = float((raw[t["name"]] ** 2).sum()) * gscale * gscale
        assert abs(ts[i, 1] - ss) <= 1e-5 * max(ss, 1e-30), t["name"]
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,gscale,momentum", [("NATURE", 6, 1.0, 0.0), ("NATURE", 6, 0.5, 0.9), ("NIPS", 4, 1.0, 0.9),
                                                    ("NIPS", 4, 0.5, 0.0)])
def test_local_step_parity(arch, A, gscale, momentum):
    from paac_amd import hip_ops
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=8)
    if arch == "NATURE":
        assert ctx.layout["total"] > ctx.layout["total_unpadded"]       # A = 6: bias tensors end in pads
    assert check_local_step(ctx, gscale, momentum)
    ctx.close()


_USER_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from paac_amd import _lib, hip_ops, networks
networks.define_architecture("TINY3", %(convs)r, %(fc)d)
from test_clip_local import check_local_step
ctx = hip_ops.Context(_lib.ARCH_USER, 6, max_batch=8)
assert len(ctx.layout["tensors"]) == 12
for gscale, momentum in ((1.0, 0.9), (0.5, 0.0)):
    check_local_step(ctx, gscale, momentum)
ctx.close()
print("USER_LOCAL_OK")
"""


@pytest.mark.gpu
def test_local_step_parity_three_conv_user_architecture():
    """12 tensors (the --user_arch build path of test_user_arch_gpu.py: a library per geometry, so a child process)."""
    script = _USER_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), convs=[(16, 8, 4), (32, 4, 2), (32, 3, 1)],
                                 fc=256)
    res = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "USER_LOCAL_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


@pytest.mark.gpu
def test_grad_tensor_stats_needs_a_local_step():
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=8)
    n = ctx.layout["total"]
    z = lambda: torch.zeros(n, device="cuda")
    ctx.clip_rmsprop(z(), z(), torch.ones(n, device="cuda"), z(), torch.tensor([0.01], device="cuda"), 0.99, 0.0, 0.1, 3.0,
                     _lib.CLIP_GLOBAL)
    with pytest.raises(_lib.PaacHipError, match="local"):
        ctx.grad_tensor_stats()
    ctx.close()


# -- GPU: packed copies, gradient routes, summaries --------------------------------------------------------------------

def make_case(arch, A, B, seed):
    from oracle import network as onet
    rs = np.random.RandomState(seed)
    params = onet.init_params(arch, A, rs, dtype=np.float32)
    states = rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)
    return params, states, rs.randint(0, A, B).astype(np.int32), rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32)


def upload(ctx, params):
    import torch
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return torch.from_numpy(flat).cuda()


@pytest.mark.gpu
def test_local_step_keeps_packed_weights_current():
    """Managed mode, Nature (fused tower): the forward and backward right after a local step read the packed copies the step
    wrote -- equal, bit for bit, to those after an explicit pack_weights."""
    import torch
    from paac_amd import _lib, hip_ops
    arch, A, B = "NATURE", 4, 24
    params, states, idx, y, adv = make_case(arch, A, B, seed=9)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    p = upload(ctx, params)
    s = torch.from_numpy(states).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (idx, y, adv)]
    n = ctx.layout["total"]
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    before = torch.zeros((B, A), device="cuda")
    ctx.forward(p, s, logits=before)
    grad = torch.zeros(n, device="cuda")
    ctx.loss_backward(p, s, *dev, 0.02, grad)
    step = lambda: ctx.clip_rmsprop(p, grad, torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"),
                                    torch.tensor([0.05], device="cuda"), 0.99, 0.0, 0.1, 0.05, _lib.CLIP_LOCAL)
    step()
    f = ctx.grad_tensor_stats()[:, 5]
    assert (f < 1.0).any() and (f == 1.0).any()
    after = torch.zeros((B, A), device="cuda")
    ctx.forward(p, s, logits=after)
    ctx.pack_weights(p)
    repacked = torch.zeros((B, A), device="cuda")
    ctx.forward(p, s, logits=repacked)
    torch.cuda.synchronize()
    assert torch.equal(after, repacked) and not torch.equal(after, before)
    step()
    g_after = torch.zeros(n, device="cuda")
    ctx.loss_backward(p, s, *dev, 0.02, g_after)
    ctx.pack_weights(p)
    g_repacked = torch.zeros(n, device="cuda")
    ctx.loss_backward(p, s, *dev, 0.02, g_repacked)
    torch.cuda.synchronize()
    assert torch.equal(g_after, g_repacked)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B,clip_norm", [("NATURE", 4, 160, 0.05), ("NIPS", 6, 24, 0.3)])
def test_local_step_is_bit_identical_on_both_gradient_routes(arch, A, B, clip_norm):
    """loss_backward(phase=3) (the norm pass folds the pending split-K slabs) and phase=0 (grad_finalize_kernel did): the
    same parameters, slots, clipped norm and per-tensor summaries, bit for bit."""
    import torch
    from paac_amd import _lib, hip_ops
    params, states, idx, y, adv = make_case(arch, A, B, seed=21)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    n = ctx.layout["total"]
    s = torch.from_numpy(states).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (idx, y, adv)]
    out = []
    for phase in (0, 3):
        p = upload(ctx, params)
        grad = torch.zeros(n, device="cuda")
        ms, mom, gn = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
        ctx.loss_backward(p, s, *dev, 0.02, grad, phase=phase)
        ctx.clip_rmsprop(p, grad, ms, mom, torch.tensor([0.05], device="cuda"), 0.99, 0.9, 0.1, clip_norm, _lib.CLIP_LOCAL,
                         gnorm_out=gn)
        ts = ctx.grad_tensor_stats()
        torch.cuda.synchronize()
        out.append((p.cpu().numpy(), grad.cpu().numpy(), ms.cpu().numpy(), mom.cpu().numpy(), gn.cpu().numpy(), ts))
    assert (out[0][5][:, 5] < 1.0).any() and (out[0][5][:, 5] == 1.0).any()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed", "negative_with_real_zeros"])
def test_local_grad_stats_are_the_clipped_summaries(case):
    """grad_stats in local mode: raw and clipped mean / stddev / max / min over the reference's P elements (pads excluded),
    global_norm of the clipped gradient, and the per-tensor block (raw L2 norm, factor)."""
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NATURE"], 6, max_batch=8)       # A = 6: bias tensors end in pads
    n = ctx.layout["total"]
    gscale, clip_norm = 0.5, 0.5
    flat = local_gradient(ctx, clip_norm, gscale, seed=8)
    if case != "mixed":
        flat = -np.abs(flat)
        for t in ctx.layout["tensors"]:
            if t["size"] > 100:
                flat[t["offset"]:t["offset"] + t["size"]:17] = 0.0
    z = lambda: torch.zeros(n, device="cuda")
    ctx.clip_rmsprop(z(), torch.from_numpy(flat).cuda(), torch.ones(n, device="cuda"), z(), torch.tensor([0.01], device="cuda"),
                     0.99, 0.0, 0.1, clip_norm, _lib.CLIP_LOCAL, gscale)
    got = ctx.grad_stats(clip_norm, _lib.CLIP_LOCAL)
    raw = {k: v * gscale for k, v in split(ctx, flat).items()}
    clipped, f, gn = clip_by_norm_local(raw, clip_norm)
    assert abs(got["global_norm"] - gn) / gn < 1e-5
    for name, d in (("raw_gradients", raw), ("clipped_gradients", clipped)):
        x = np.concatenate([v.reshape(-1) for v in d.values()])
        want = dict(mean=x.mean(), stddev=np.sqrt(((x - x.mean()) ** 2).mean()), max=x.max(), min=x.min())
        for k, w in want.items():
            assert abs(got[name][k] - w) <= 2e-5 * max(abs(w), np.abs(x).max() * 1e-2), (case, name, k, got[name][k], w)
    assert list(got["tensors"]) == [t["name"] for t in ctx.layout["tensors"]]
    for k, v in got["tensors"].items():
        norm = float(np.sqrt((raw[k] ** 2).sum()))
        assert abs(v["norm"] - norm) <= 1e-5 * max(norm, 1e-30) and abs(v["factor"] - f[k]) <= 1e-5, k
    ctx.close()


# -- GPU: the loops --------------------------------------------------------------------------------------------------

@pytest.fixture
def local_oracle(monkeypatch):
    """OracleLoop's clip step (oracle.network.clip_by_global_norm) with 'local' restated; records the factors."""
    from oracle import network as onet
    orig = onet.clip_by_global_norm
    factors = []

    def clip(grads, clip_norm, mode="global"):
        if mode != "local":
            return orig(grads, clip_norm, mode)
        out, f, gn = clip_by_norm_local(grads, clip_norm)
        factors.append(f)
        return out, gn

    monkeypatch.setattr(onet, "clip_by_global_norm", clip)
    return factors


def assert_binds_on_some(factors):
    f = np.array(list(factors[0].values()))           # cycle 1
    assert (f < 1.0).any() and (f == 1.0).any(), factors[0]


@pytest.mark.gpu
def test_device_loop_local_matches_oracle(local_oracle):
    from test_learner_gpu import OracleLoop, build_learner, make_args
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 32, 5, 3
    args = make_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.05, sampler="numpy", test_seed=11,
                     clip_norm_type="local", clip_norm=0.15)
    learner, params, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, env_creator.device_env_spec, sampler="numpy", use_graph=True)
    loop = OracleLoop(args, params, env_creator, "NATURE")
    for c in range(cycles):
        want = loop.cycle()
        ro.run_cycle()
        ro.synchronize()
        assert np.array_equal(ro.actions.view(-1).cpu().numpy(), np.argmax(want["actions"], axis=1)), "cycle %d" % c
        assert np.array_equal(ro.rollout_states().cpu().numpy(), want["states"]), "cycle %d" % c
        assert abs(float(learner.gnorm_dev.item()) - want["gnorm"]) <= 1e-4 * want["gnorm"], "cycle %d" % c
    assert_binds_on_some(local_oracle)
    got = learner.network.get_parameters()
    for k, v in want["params"].items():
        assert np.abs(got[k] - v).max() < 2e-4, k
    ro.close()


@pytest.mark.gpu
def test_host_loop_local_matches_oracle(local_oracle):
    from test_learner_gpu import build_learner, make_args, oracle_cycles
    N, T, cycles = 8, 5, 3
    feeds = []
    args = make_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=cycles * N * T, host_environments=True, record_feeds=True, feed_callback=feeds.append,
                     synthetic_terminal_p=0.1, test_seed=42, clip_norm_type="local", clip_norm=0.5)
    learner, params, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    learner.train()
    want = oracle_cycles(args, params, env_creator, cycles, "NIPS")
    assert_binds_on_some(local_oracle)
    assert len(feeds) == cycles
    for c in range(cycles):
        assert np.array_equal(feeds[c]["states"], want[c]["states"]), "states differ in cycle %d" % c
        assert np.array_equal(feeds[c]["actions"], np.argmax(want[c]["actions"], axis=1)), "actions differ in cycle %d" % c
    got = learner.network.get_parameters()
    for k, v in want[-1]["params"].items():
        assert np.abs(got[k] - v).max() < 2e-4, k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["local", "global"])
def test_metrics_gradients_record(mode):
    """metrics.jsonl: in local mode the gradients record gains {"tensors": {name: {"norm", "factor"}}} and global_norm /
    the progress record's grad_norm carry the clipped norm; the global mode's records keep their fields."""
    from test_learner_gpu import build_learner, make_args
    N = 256                                           # a progress record every 2048 / N = 8 cycles (paac.py:172)
    args = make_args(game="pong", arch="NIPS", emulator_counts=N, max_local_steps=1, max_global_steps=8 * N,
                     clip_norm_type=mode, clip_norm=0.5)
    learner, _, _ = build_learner(args)
    learner.train()
    recs = [json.loads(l) for l in open(os.path.join(args.debugging_folder, "metrics.jsonl"))]
    grads = [r for r in recs if r["kind"] == "gradients"]
    prog = [r for r in recs if r["kind"] == "progress"]
    assert len(grads) == 1 and len(prog) == 1
    g = grads[0]
    if mode == "global":
        assert set(g) == {"kind", "time", "global_step", "global_norm", "raw_gradients", "clipped_gradients"}
        return
    names = [t["name"] for t in learner.ctx.layout["tensors"]]
    assert list(g["tensors"]) == names
    f = np.array([g["tensors"][k]["factor"] for k in names])
    norms = np.array([g["tensors"][k]["norm"] for k in names])
    assert np.all(np.isfinite(f)) and np.all(f > 0.0) and np.all(f <= 1.0)
    want_f = np.array([0.5 * min(1.0 / x if x > 0 else np.inf, 2.0) for x in norms])
    assert np.abs(f - want_f).max() < 1e-5
    clipped_norm = float(np.sqrt(np.sum((f * norms) ** 2)))
    assert abs(g["global_norm"] - clipped_norm) <= 1e-5 * clipped_norm
    assert abs(prog[0]["grad_norm"] - clipped_norm) <= 1e-5 * clipped_norm


@pytest.mark.gpu
def test_local_checkpoint_resumes_and_evaluates():
    """A local-mode run's checkpoint restores the weights and RMSProp slots exactly; the resumed learner keeps training in
    local mode; the eval harness (paac_amd.test) runs on the folder whose args.json says 'local'."""
    from test_learner_gpu import build_learner, make_args
    from paac_amd import logger_utils, train
    from paac_amd.paac import PAACLearner
    args = make_args(game="pong", arch="NIPS", emulator_counts=4, max_local_steps=2, max_global_steps=16,
                     clip_norm_type="local", clip_norm=0.5)
    logger_utils.save_args(args, args.debugging_folder)
    learner, params, _ = build_learner(args)
    learner.train()
    saved = learner.network.get_parameters()
    rms = learner.network.get_parameters(learner.rms)
    nc, ec = train.get_network_and_environment_creator(args)
    l2 = PAACLearner(nc, ec, args)
    assert l2.clip_norm_type == "local"
    assert l2.init_network() == 16
    for k, v in l2.network.get_parameters().items():
        assert np.array_equal(v, saved[k])
    for k, v in l2.network.get_parameters(l2.rms).items():
        assert np.array_equal(v, rms[k]) and not np.all(v == 1.0)
    l2.max_global_steps = 32
    l2.train()
    moved = l2.network.get_parameters()
    assert all(np.isfinite(v).all() for v in moved.values()) and any(not np.array_equal(moved[k], saved[k]) for k in saved)
    assert json.load(open(os.path.join(args.debugging_folder, "args.json")))["clip_norm_type"] == "local"
    res = subprocess.run([sys.executable, "-m", "paac_amd.test", "-f", args.debugging_folder, "-tc", "2", "-np", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "Performed 2 tests" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
