"""-m gpu: input gradients (include/paac_hip.h: paac_input_grad; csrc/conv1_dgrad.h) against a float64 autograd reference, the
fused FGSM epilogue against its numpy statement, the entry's refusals, and the attacked device evaluation."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USER_SPEC = "16:8:3,32:4:2,256"          # O1 = 26: pixel row / column 83 is covered by no window; stride 3: the direct kernel


def make_case(ctx, B, seed):
    from paac_amd import networks
    rs = np.random.RandomState(seed)
    params = networks.initial_values(ctx.layout, rs)
    states = rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)
    states[rs.rand(B, 84, 84, 4) < 1.0 / 3.0] = 0
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return params, states, torch.from_numpy(flat).cuda(), torch.from_numpy(states).cuda()


def reference(ctx, params, states, seed_of):
    """float64 CPU forward with every ReLU replaced by the DEVICE's mask (debug_activation(21..24), read after the call), and
    autograd of seed_of(logits, values) to the scaled input -> float64 [B, 84, 84, 4]."""
    import torch.nn.functional as F
    from paac_amd import hip_ops
    B = states.shape[0]
    convs, _ = hip_ops.arch_geometry(ctx.arch)
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    x = (torch.from_numpy(states).float() * np.float32(1.0 / 255.0)).double().requires_grad_()
    a = x.permute(0, 3, 1, 2)
    for i, (_, _, stride) in enumerate(convs):
        a = F.conv2d(a, t64(params["conv%d_weights" % (i + 1)]).permute(3, 2, 0, 1), t64(params["conv%d_biases" % (i + 1)]), stride=stride)
        mask = ctx.debug_activation(21 + i, B).cpu().reshape(B, a.shape[2], a.shape[3], a.shape[1]) > 0
        a = a * mask.permute(0, 3, 1, 2).double()
    n = len(convs) + 1
    h = a.permute(0, 2, 3, 1).reshape(B, -1) @ t64(params["fc%d_weights" % n]) + t64(params["fc%d_biases" % n])
    h = h * (ctx.debug_activation(24, B).cpu().reshape(B, -1) > 0).double()
    logits = h @ t64(params["actor_output_weights"]) + t64(params["actor_output_biases"])
    values = (h @ t64(params["critic_output_weights"]) + t64(params["critic_output_biases"])).reshape(B)
    seed_of(logits, values).backward()
    return x.grad.numpy()


def check_against_reference(ctx, B, A, mode, seed=0):
    params, states, p, s = make_case(ctx, B, seed)
    rs = np.random.RandomState(seed + 1)
    kw, sl, sv = {}, rs.randn(B, A).astype(np.float32), rs.randn(B).astype(np.float32)
    if mode == "seeds":
        kw = dict(seed_logits=torch.from_numpy(sl).cuda(), seed_value=torch.from_numpy(sv).cuda())
    dx = ctx.input_gradient(p, s, mode=mode, **kw).cpu().numpy()
    torch.cuda.synchronize()
    if mode == "seeds":
        seed_of = lambda logits, values: (logits * torch.from_numpy(sl).double()).sum() + (values * torch.from_numpy(sv).double()).sum()
    elif mode == "value":
        seed_of = lambda logits, values: values.sum()
    else:                                  # the argmax is the device's own: from the probabilities its forward left
        best = ctx.debug_activation(26, B).cpu().reshape(B, A).argmax(dim=1)
        seed_of = lambda logits, values: torch.log_softmax(logits, dim=1)[torch.arange(B), best].sum()
    ref = reference(ctx, params, states, seed_of)
    assert dx.shape == ref.shape and np.isfinite(dx).all()
    err = np.abs(dx - ref).reshape(B, -1).max(axis=1)
    scale = np.abs(ref).reshape(B, -1).max(axis=1)
    print("max relative error per row: %.3g" % (err / scale).max())
    assert (err <= 1e-4 * scale).all(), (err / scale).max()
    return dx


CASES = [(arch, B, A, mode) for arch, batches in (("NIPS", (1, 5, 33)), ("NATURE", (1, 5, 33, 513)))
         for B in batches for A in (3, 18) for mode in ("seeds", "value", "logp_argmax")]


@pytest.mark.parametrize("arch,B,A,mode", CASES)
def test_against_float64(arch, B, A, mode):
    from paac_amd import hip_ops
    ctx = hip_ops.Context({"NIPS": 0, "NATURE": 1}[arch], A, max_batch=max(B, 8))
    dx = check_against_reference(ctx, B, A, mode)
    assert dx[:, 83].any() and dx[:, :, 83].any()          # 84 = 19 * 4 + 8: the last pixel row and column are covered
    ctx.close()


def user_arch_case():
    """(child process: a process holds one library)"""
    from paac_amd import _lib, hip_ops, networks
    from paac_amd.build import parse_user_arch, user_arch_library
    convs, fc = parse_user_arch(USER_SPEC)
    # (the project's build has made this library -- __graft_entry__.INPUT_GRAD_USER_ARCH; built here only where it is missing)
    networks.define_architecture("USER", convs, fc, build=not os.path.exists(user_arch_library(convs, fc)[0]))
    ctx = hip_ops.Context(_lib.ARCH_USER, 6, max_batch=5)
    dx = check_against_reference(ctx, 5, 6, "value")
    assert not dx[:, 83].any() and not dx[:, :, 83].any() and dx[:, 82].any() and dx[:, :, 82].any()
    ctx.close()


def test_first_layer_outside_the_cell_form():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("levels", [1, 8, 255])
def test_fused_fgsm_epilogue_is_exact(levels):
    from paac_amd import evaluation, hip_ops
    ctx = hip_ops.Context(1, 4, max_batch=5)
    _, states, p, s = make_case(ctx, 5, 3)
    dx, adv = torch.zeros((5, 84, 84, 4), device="cuda"), torch.zeros_like(s)
    ctx.input_gradient(p, s, mode="value", out=dx, fgsm_levels=levels, states_out=adv)
    assert np.array_equal(adv.cpu().numpy(), evaluation.fgsm_perturb(states, dx.cpu().numpy(), levels))
    only = torch.zeros_like(s)                                        # the form without dX: the same frames
    ctx.input_gradient(p, s, mode="value", fgsm_levels=levels, states_out=only)
    assert torch.equal(only, adv) and not torch.equal(adv, s)
    ctx.close()


def test_refusals_and_state():
    from paac_amd import _lib, hip_ops
    A, B = 4, 70
    ctx = hip_ops.Context(1, A, max_batch=B)
    _, _, p, s = make_case(ctx, B, 4)
    dx = torch.full((B, 84, 84, 4), 7.0, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    raw = lambda batch=B, mode=1, out=dx, levels=0, so=None: ctx.lib.paac_input_grad(
        ctx.handle, vp(p), vp(s), batch, mode, None, None, None, vp(out), levels, vp(so), None)
    other = torch.zeros_like(s)
    for kw in (dict(batch=0), dict(batch=B + 1), dict(mode=4), dict(mode=-1), dict(mode=2), dict(levels=-1), dict(levels=256),
               dict(levels=3), dict(out=None), dict(levels=3, so=s)):
        assert raw(**kw) < 0 and _lib.load().paac_last_error(), kw
    ctx.train_forward_trunk(p, s)                                    # 70 rows: the heads stay pending
    assert raw() < 0 and b"pending" in _lib.load().paac_last_error()
    ctx.train_forward(p, s)
    ctx.keep_next_forward(0)
    assert raw() < 0 and b"paac_keep_next_forward" in _lib.load().paac_last_error()
    ctx.keep_next_forward(-1)
    # an owed acting sample (paac_act_step_pipe)
    N = 4
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    mt = hip_ops.mt_state_from_numpy(np.random.RandomState(0).get_state(), ctx.device)
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    ctx.act_step_pipe(p, s[:N], mt, torch.zeros(N, dtype=torch.int32, device="cuda"), f32(N, A), f32(N), 1, 0, 0,
                      torch.zeros(1, dtype=torch.int64, device="cuda"), 0, other[:N], f32(N), f32(N), f32(N),
                      torch.zeros(N, dtype=torch.int32, device="cuda"))
    assert ctx.act_step_pending() and raw() < 0 and b"paac_act_step_pipe" in _lib.load().paac_last_error()
    ctx.act_step_flush()
    ctx.set_managed_weights(False)
    torch.cuda.synchronize()
    assert torch.all(dx == 7.0)                                      # no refusal launched anything
    with pytest.raises(ValueError):
        ctx.input_gradient(p, s, mode="gradient")
    with pytest.raises(ValueError):
        ctx.input_gradient(p, s, fgsm_levels=3)
    # ... and the entry leaves nothing behind: train_forward + loss_backward give the bits they give alone
    rs = np.random.RandomState(5)
    idx, y, adv = (torch.from_numpy(a).cuda() for a in (rs.randint(0, A, B).astype(np.int32), rs.randn(B).astype(np.float32),
                                                        rs.randn(B).astype(np.float32)))
    grads = []
    for with_entry in (False, True):
        if with_entry:
            ctx.input_gradient(p, s, mode="logp_argmax", out=dx)
        g = torch.zeros(ctx.layout["total"], device="cuda")
        ctx.train_forward(p, s)
        ctx.loss_backward(p, s, idx, y, adv, 0.02, g, forward_done=True)
        grads.append(g)
    assert torch.equal(grads[0], grads[1]) and grads[0].abs().max() > 0 and not torch.all(dx == 7.0)
    ctx.close()


def test_attacked_evaluation_steps_the_true_world():
    import test_evaluation_gpu as te
    from paac_amd import evaluation, hip_ops
    network, env_creator = te.fresh_network(te.catch_args())
    spec = env_creator.device_env_spec
    ctx = hip_ops.Context(network.arch_id, 3, max_batch=8)
    runs = {}
    for name, kw in (("plain", {}), ("off", dict(attack_eps=0)), ("attacked", dict(attack_eps=255))):
        ev = evaluation.DeviceEvaluator(network, ctx, spec, count=8, noops=2, record=True, seed=te.SEED, **kw)
        runs[name] = ev.run()
        assert (ev.scratch is not None) == (name == "attacked")
        ev.close()
    for x, y in zip(runs["plain"], runs["off"]):
        assert np.array_equal(x, y)
    scores, lengths, trace, noops_e = runs["attacked"]
    steps = min(len(trace), len(runs["plain"][2]))
    assert not np.array_equal(trace[:steps], runs["plain"][2][:steps])          # the policy saw other frames ...
    want = evaluation.replay_on_twins(env_creator, trace, noops_e)              # ... the games did not
    assert np.array_equal(scores, want[0]) and np.array_equal(lengths, want[1])
    # the same through the captured blocks, replayed twice
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=8, noops=2, seed=te.SEED, attack_eps=255, steps_per_launch=4)
    first, second = ev.run(), ev.run()
    assert ev.use_graph and np.array_equal(first[0], scores) and np.array_equal(second[0], scores)
    assert np.array_equal(first[1], lengths) and np.array_equal(second[1], lengths)
    ev.close()
    ctx.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    user_arch_case()
