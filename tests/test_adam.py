"""--optimizer adam: TF 1.0.1 tf.train.AdamOptimizer(lr, beta1, beta2, epsilon=e, name='OptimizerVariables') applied to the
clipped gradients exactly where RMSProp is applied (actor_learner.py:31-34,70).  The checker is this file's own fp64
restatement of TF's ApplyAdam (oracle/ restates RMSProp only); the bias-correction powers are fp32 variables advanced by
fp32 products, so they are compared bit for bit with the np.float32 product chain."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH_ID = {"NIPS": 0, "NATURE": 1}


# -- the restatement ---------------------------------------------------------------------------------------------------

def power_chain(beta, length):
    """beta_power after length - 1 updates: the fp32 variable starts at beta and is multiplied by beta once per update."""
    p = np.float32(beta)
    for _ in range(length - 1):
        p = np.float32(p * np.float32(beta))
    return p


def adam_fp64(var, g, m, v, powers, lr, beta1, beta2, eps):
    """TF ApplyAdam on flat arrays, in fp64 from the fp32 powers and lr the step reads:
        alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power)
        m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); var -= m * alpha / (sqrt(v) + eps)
    -> (var, m, v)."""
    b1p, b2p = float(powers[0]), float(powers[1])
    alpha = float(lr) * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    g = np.asarray(g, dtype=np.float64)
    m = m + (g - m) * (1.0 - float(np.float32(beta1)))
    v = v + (g * g - v) * (1.0 - float(np.float32(beta2)))
    return var - m * alpha / (np.sqrt(v) + float(np.float32(eps))), m, v


def clip_fp64(tensors, mode, clip_norm):
    """{name: fp64 array} -> (clipped, global norm reported): ignore, tf.clip_by_global_norm, or tf.clip_by_norm per tensor
    (TF 1.0.1: clip_norm * min(rsqrt(ss), 1 / clip_norm), a zero tensor keeps factor 1; the norm of the clipped list)."""
    gn = float(np.sqrt(sum(float((t * t).sum()) for t in tensors.values())))
    if mode == "ignore":
        return dict(tensors), gn
    if mode == "global":
        f = clip_norm * min(1.0 / gn, 1.0 / clip_norm) if gn > 0 else 1.0
        return {k: t * f for k, t in tensors.items()}, gn
    out = {}
    for k, t in tensors.items():
        ss = float((t * t).sum())
        out[k] = t * (clip_norm * min(np.inf if ss == 0.0 else 1.0 / np.sqrt(ss), 1.0 / clip_norm))
    return out, float(np.sqrt(sum(float((t * t).sum()) for t in out.values())))


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_optimizer_flags_and_args_json(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    d = p.parse_args([])
    assert (d.optimizer, d.beta1, d.beta2, d.e, d.alpha) == ("rmsprop", 0.9, 0.999, 0.1, 0.99)
    a = p.parse_args(["--optimizer", "adam", "--beta1", "0.8", "--beta2", "0.99"])
    assert (a.optimizer, a.beta1, a.beta2) == ("adam", 0.8, 0.99)
    with pytest.raises(SystemExit):
        p.parse_args(["--optimizer", "sgd"])
    logger_utils.save_args(a, str(tmp_path))
    saved = logger_utils.load_args(os.path.join(str(tmp_path), "args.json"))
    assert (saved["optimizer"], saved["beta1"], saved["beta2"]) == ("adam", 0.8, 0.99)
    assert "Adam" in [t for o, _, _, _, t in train.REFERENCE_FLAGS if o == ("--e",)][0]


def test_restatement_first_steps():
    lr, b1, b2 = np.float32(0.01), 0.9, 0.999
    powers = np.array([power_chain(b1, 1), power_chain(b2, 1)])
    g = np.array([2.0, -0.5, 0.0, 1e-3])
    z = np.zeros(4)
    # first step: m = (1 - b1) g, v = (1 - b2) g^2, alpha = lr sqrt(1 - b2) / (1 - b1) -> the step is lr * sign(g) * |g| /
    # (|g| + eps / sqrt(1 - b2)): about lr for |g| >> eps, and exactly 0 for an exact-zero gradient (no NaN)
    c1, c2 = 1.0 - float(np.float32(b1)), 1.0 - float(np.float32(b2))      # the betas are fp32 constants, as in TF
    assert abs(c1 - 0.1) < 1e-7 and abs(c2 - 0.001) < 1e-7
    var, m, v = adam_fp64(z, g, z, z, powers, lr, b1, b2, 1e-8)
    assert np.allclose(m, c1 * g, rtol=1e-12, atol=0) and np.allclose(v, c2 * g * g, rtol=1e-12, atol=0)
    assert np.allclose(var[[0, 1, 3]], -float(lr) * np.sign(g[[0, 1, 3]]), rtol=1e-3)
    assert var[2] == 0.0 and np.all(np.isfinite(var))
    # eps = 0.1 dominates a small gradient's sqrt(v): the step is proportional to g
    var, _, _ = adam_fp64(z, g, z, z, powers, lr, b1, b2, 0.1)
    b1p, b2p = float(powers[0]), float(powers[1])
    want = -float(lr) * np.sqrt(1 - b2p) / (1 - b1p) * c1 * g / (np.sqrt(c2) * np.abs(g) + float(np.float32(0.1)))
    assert np.allclose(var, want, rtol=1e-12) and var[2] == 0.0
    # all-zero moments and gradient over many steps stay zero
    var, m, v = z, z, z
    for k in range(1, 5):
        var, m, v = adam_fp64(var, z, m, v, [power_chain(b1, k), power_chain(b2, k)], lr, b1, b2, 1e-8)
    assert not np.any(var) and not np.any(m) and not np.any(v)
    # the chain is fp32: not the fp64 power
    assert power_chain(b2, 1000) == np.float32(power_chain(b2, 999) * np.float32(b2))
    assert float(power_chain(0.9, 3)) == float(np.float32(np.float32(np.float32(0.9) * np.float32(0.9)) * np.float32(0.9)))


def test_header_declares_clip_adam():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    m = re.search(r"int\s+paac_clip_adam\s*\(([^;]*)\);", hdr)
    assert m, "paac_clip_adam missing from the header"
    assert len(m.group(1).split(",")) == len(_lib._SIGNATURES["paac_clip_adam"][1]) == 16
    assert "beta_powers" in m.group(1)
    assert "paac_clip_adam" in _lib.EXPORTED_SYMBOLS


def test_tensor_of_key_and_network_filter_accept_unscoped_keys():
    from paac_amd import networks
    from paac_amd.session import checkpoint_key, tensor_of_key
    assert tensor_of_key("beta1_power") == (None, None) and tensor_of_key("beta2_power") == (None, None)
    assert tensor_of_key("local_learning_1/conv1_weights/OptimizerVariables_1") == ("conv1_weights", "OptimizerVariables_1")
    got = {}
    fake = types.SimpleNamespace(name="local_learning", get_parameters=lambda: {}, set_parameters=got.update)
    saver = networks.Network.make_saver(fake)
    w = np.ones((2, 2), np.float32)
    saver.set_arrays({checkpoint_key("local_learning", "conv1_weights"): w,
                      checkpoint_key("local_learning", "conv1_weights", "OptimizerVariables"): w * 2,
                      "beta1_power": np.float32(0.5), "beta2_power": np.float32(0.9)})
    assert list(got) == ["conv1_weights"] and np.array_equal(got["conv1_weights"], w)


class _FlatNet(object):
    """The slice of a Network the optimizer checkpoint mapping uses, on the CPU."""

    def __init__(self):
        self.name = "local_learning"
        self.layout = dict(tensors=[dict(name="conv1_weights", shape=(2, 3), offset=0, size=6),
                                    dict(name="conv1_biases", shape=(3,), offset=8, size=3)], total=12)

    def get_parameters(self, flat):
        host = flat.numpy()
        return {t["name"]: host[t["offset"]:t["offset"] + t["size"]].reshape(t["shape"]).copy() for t in self.layout["tensors"]}


def _cpu_learner(optimizer):
    import torch
    from paac_amd.actor_learner import ActorLearner
    L = ActorLearner.__new__(ActorLearner)
    L.network, L.optimizer = _FlatNet(), optimizer
    rs = np.random.RandomState(1)
    if optimizer == "adam":
        L.adam_m = torch.from_numpy(rs.randn(12).astype(np.float32))
        L.adam_v = torch.from_numpy(rs.rand(12).astype(np.float32))
        L.beta_powers = torch.tensor([power_chain(0.9, 4), power_chain(0.999, 4)])
    else:
        L.rms = torch.from_numpy(rs.rand(12).astype(np.float32))
        L.mom = torch.zeros(12)
    return L


def test_adam_checkpoint_keys_round_trip_and_refuse_rmsprop(tmp_path):
    import torch
    from paac_amd import tf_bundle
    L = _cpu_learner("adam")
    d = L._get_optimizer_arrays()
    assert sorted(d) == sorted(["beta1_power", "beta2_power"] + ["local_learning_1/%s/%s" % (t, s) for t in
                                ("conv1_weights", "conv1_biases") for s in ("OptimizerVariables", "OptimizerVariables_1")])
    assert np.array_equal(d["local_learning_1/conv1_biases/OptimizerVariables"], L.adam_m.numpy()[8:11])
    assert np.array_equal(d["local_learning_1/conv1_biases/OptimizerVariables_1"], L.adam_v.numpy()[8:11])
    assert d["beta1_power"].shape == () and d["beta1_power"] == power_chain(0.9, 4)
    # through the TF bundle container (scalars included) and back into a fresh learner: the same bits
    tf_bundle.write(os.path.join(str(tmp_path), "-7"), d)
    back = tf_bundle.read(os.path.join(str(tmp_path), "-7"))
    L2 = _cpu_learner("adam")
    for t in (L2.adam_m, L2.adam_v, L2.beta_powers):
        t.zero_()
    L2._set_optimizer_arrays(back)
    assert torch.equal(L2.adam_m[[0, 1, 2, 3, 4, 5, 8, 9, 10]], L.adam_m[[0, 1, 2, 3, 4, 5, 8, 9, 10]])
    assert torch.equal(L2.adam_v[[0, 1, 2, 3, 4, 5, 8, 9, 10]], L.adam_v[[0, 1, 2, 3, 4, 5, 8, 9, 10]])
    assert torch.equal(L2.beta_powers, L.beta_powers)
    # an RMSProp optimizer checkpoint has the same slot keys but no powers: refused, naming both optimizers
    rms = _cpu_learner("rmsprop")._get_optimizer_arrays()
    assert "beta1_power" not in rms
    with pytest.raises(KeyError, match=r"RMSProp.*Adam"):
        L2._set_optimizer_arrays(rms)
    # and an RMSProp learner still restores its own checkpoint as before
    R = _cpu_learner("rmsprop")
    R.rms.zero_()
    R._set_optimizer_arrays(rms)
    assert torch.equal(R.rms[:6], _cpu_learner("rmsprop").rms[:6])


# -- GPU: the optimizer step on its own --------------------------------------------------------------------------------

NORM_PATTERN = (4.0, 0.3, 0.0, 2.5, 0.6, 1.7, 0.2, 3.0, 0.5, 8.0, 0.05, 1.3)


def pad_mask(lay):
    real = np.zeros(lay["total"], dtype=bool)
    for t in lay["tensors"]:
        real[t["offset"]:t["offset"] + t["size"]] = True
    return ~real


def gradient(lay, clip_norm, gscale, seed):
    """Flat gradient whose tensors sit above, below and at zero relative to clip_norm (after gscale); pads zero."""
    rs = np.random.RandomState(seed)
    flat = np.zeros(lay["total"], dtype=np.float32)
    for i, t in enumerate(lay["tensors"]):
        x = rs.randn(t["size"])
        want = NORM_PATTERN[(i + seed) % len(NORM_PATTERN)] * clip_norm / gscale
        flat[t["offset"]:t["offset"] + t["size"]] = (x * want / np.linalg.norm(x)).astype(np.float32)
    return flat


def check_adam_steps(ctx, mode, gscale, eps, steps=3, beta1=0.9, beta2=0.999, seed=3):
    """`steps` consecutive ctx.clip_adam calls against the fp64 restatement, each from the device's state before it (the
    bars of test_clip_rmsprop_parity); the powers bit-exact to the fp32 chain; the pads stay zero."""
    import torch
    from paac_amd import _lib
    lay = ctx.layout
    n, pads = lay["total"], pad_mask(lay)
    clip_norm, lr = 0.5, np.float32(0.0224)
    rs = np.random.RandomState(seed)
    var = rs.randn(n).astype(np.float32) * 0.1
    var[pads] = 0.0
    dv, dm, ds = torch.from_numpy(var).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    powers = torch.tensor([beta1, beta2], dtype=torch.float32, device="cuda")
    lr_dev, gn_dev = torch.tensor([lr], device="cuda"), torch.zeros(1, device="cuda")
    code = {"ignore": _lib.CLIP_IGNORE, "global": _lib.CLIP_GLOBAL, "local": _lib.CLIP_LOCAL}[mode]
    for k in range(steps):
        g = gradient(lay, clip_norm, gscale, seed + 1 + k)
        before = [t.cpu().numpy().astype(np.float64) for t in (dv, dm, ds)]
        p_before = powers.cpu().numpy()
        ctx.clip_adam(dv, torch.from_numpy(g).cuda(), dm, ds, powers, lr_dev, beta1, beta2, eps, clip_norm, code, gscale,
                      gn_dev)
        torch.cuda.synchronize()
        raw = {t["name"]: g[t["offset"]:t["offset"] + t["size"]].astype(np.float64) * gscale for t in lay["tensors"]}
        clipped, gn = clip_fp64(raw, mode, clip_norm)
        gc = np.zeros(n)
        for t in lay["tensors"]:
            gc[t["offset"]:t["offset"] + t["size"]] = clipped[t["name"]].reshape(-1)
        var_e, m_e, v_e = adam_fp64(*before[:1], gc, before[1], before[2], p_before, lr, beta1, beta2, eps)
        got_v, got_m, got_s = dv.cpu().numpy(), dm.cpu().numpy(), ds.cpu().numpy()
        what = (mode, gscale, eps, k)
        assert abs(gn_dev.item() - gn) <= 1e-5 * gn, what
        assert np.abs(got_m - m_e).max() < 1e-6, what
        assert np.abs(got_s - v_e).max() < 1e-7, what
        assert np.abs(got_v - var_e).max() < 1e-6, what
        assert np.all(np.isfinite(got_v)), what
        assert not np.any(got_v[pads]) and not np.any(got_m[pads]) and not np.any(got_s[pads]), what
        chain = np.array([power_chain(beta1, k + 2), power_chain(beta2, k + 2)], dtype=np.float32)
        assert np.array_equal(powers.cpu().numpy(), chain), (what, powers.cpu().numpy(), chain)
    # the mix the test is about: a tensor with an exact-zero gradient in some step
    assert any(NORM_PATTERN[(i + seed + 1 + k) % len(NORM_PATTERN)] == 0.0 for i in range(len(lay["tensors"]))
               for k in range(steps))
    return True


CASES = [(mode, gscale, eps) for mode in ("ignore", "global", "local") for gscale in (1.0, 0.5) for eps in (0.1, 1e-8)]


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A", [("NATURE", 6), ("NIPS", 4)])
def test_adam_step_parity(arch, A):
    from paac_amd import hip_ops
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=8)
    if arch == "NATURE":
        assert ctx.layout["total"] > ctx.layout["total_unpadded"]       # A = 6: bias tensors end in pads
    for mode, gscale, eps in CASES:
        assert check_adam_steps(ctx, mode, gscale, eps)
    ctx.close()


_USER_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from paac_amd import _lib, hip_ops, networks
networks.define_architecture("TINY3", %(convs)r, %(fc)d)
from test_adam import CASES, check_adam_steps
ctx = hip_ops.Context(_lib.ARCH_USER, 6, max_batch=8)
assert len(ctx.layout["tensors"]) == 12
for mode, gscale, eps in CASES:
    check_adam_steps(ctx, mode, gscale, eps)
ctx.close()
print("USER_ADAM_OK")
"""


@pytest.mark.gpu
def test_adam_step_parity_three_conv_user_architecture():
    """12 tensors (the --user_arch build of 16,32,32,256: a library per geometry, so a child process)."""
    script = _USER_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), convs=[(16, 8, 4), (32, 4, 2), (32, 3, 1)],
                                 fc=256)
    res = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "USER_ADAM_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


@pytest.mark.gpu
def test_adam_refuses_bad_hyper_parameters():
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=8)
    n = ctx.layout["total"]
    z = lambda k=n: torch.zeros(k, device="cuda")
    for b1, b2, eps in ((1.0, 0.999, 0.1), (0.9, 1.0, 0.1), (-0.1, 0.999, 0.1), (0.9, 0.999, 0.0)):
        with pytest.raises(_lib.PaacHipError, match="paac_clip_adam"):
            ctx.clip_adam(z(), z(), z(), z(), z(2), z(1), b1, b2, eps, 3.0, _lib.CLIP_GLOBAL)
    ctx.close()


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


def adam_state(n):
    import torch
    return (torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"),
            torch.tensor([0.9, 0.999], dtype=torch.float32, device="cuda"))


@pytest.mark.gpu
def test_adam_step_keeps_packed_weights_current():
    """Managed mode, Nature (fused tower): forwards and backwards right after an Adam step read the packed copies the step
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
    m, v, powers = adam_state(n)
    step = lambda mode: ctx.clip_adam(p, grad, m, v, powers, torch.tensor([0.01], device="cuda"), 0.9, 0.999, 1e-3, 0.05, mode)
    for mode in (_lib.CLIP_GLOBAL, _lib.CLIP_LOCAL):
        step(mode)
        after = torch.zeros((B, A), device="cuda")
        ctx.forward(p, s, logits=after)
        ctx.pack_weights(p)
        repacked = torch.zeros((B, A), device="cuda")
        ctx.forward(p, s, logits=repacked)
        torch.cuda.synchronize()
        assert torch.equal(after, repacked) and not torch.equal(after, before)
        before = after
    step(_lib.CLIP_GLOBAL)
    g_after = torch.zeros(n, device="cuda")
    ctx.loss_backward(p, s, *dev, 0.02, g_after)
    ctx.pack_weights(p)
    g_repacked = torch.zeros(n, device="cuda")
    ctx.loss_backward(p, s, *dev, 0.02, g_repacked)
    torch.cuda.synchronize()
    assert torch.equal(g_after, g_repacked)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,B,mode", [("NATURE", 4, 160, "global"), ("NATURE", 4, 160, "local"), ("NIPS", 6, 24, "global")])
def test_adam_step_is_bit_identical_on_both_gradient_routes(arch, A, B, mode):
    """loss_backward(phase=3) (the norm pass folds the pending split-K slabs) and phase=0: the same parameters, moments,
    powers, gradient and norm, bit for bit, over two steps."""
    import torch
    from paac_amd import _lib, hip_ops
    code = {"global": _lib.CLIP_GLOBAL, "local": _lib.CLIP_LOCAL}[mode]
    params, states, idx, y, adv = make_case(arch, A, B, seed=21)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    n = ctx.layout["total"]
    s = torch.from_numpy(states).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (idx, y, adv)]
    out = []
    for phase in (0, 3):
        p = upload(ctx, params)
        grad, gn = torch.zeros(n, device="cuda"), torch.zeros(1, device="cuda")
        m, v, powers = adam_state(n)
        for _ in range(2):
            ctx.loss_backward(p, s, *dev, 0.02, grad, phase=phase)
            ctx.clip_adam(p, grad, m, v, powers, torch.tensor([0.01], device="cuda"), 0.9, 0.999, 1e-8, 0.3, code,
                          gnorm_out=gn)
        torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in (p, m, v, powers, grad, gn)])
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert np.array_equal(out[0][3], np.array([power_chain(0.9, 3), power_chain(0.999, 3)]))
    ctx.close()


@pytest.mark.gpu
def test_adam_graph_replays_equal_eager_steps():
    """The powers advance on the device: one clip_adam captured into a hipGraph and replayed k times == k eager calls, bit
    for bit (parameters, moments, powers, norm)."""
    import torch
    from paac_amd import _lib, hip_ops
    ctx = hip_ops.Context(ARCH_ID["NATURE"], 6, max_batch=8)
    lay, k = ctx.layout, 5
    n = lay["total"]
    g = torch.from_numpy(gradient(lay, 0.5, 1.0, 7)).cuda()
    var0 = torch.from_numpy(np.random.RandomState(2).randn(n).astype(np.float32) * 0.1).cuda()
    lr = torch.tensor([0.0224], device="cuda")
    stream = torch.cuda.Stream()
    res = []
    for replay in (False, True):
        p, gn = var0.clone(), torch.zeros(1, device="cuda")
        m, v, powers = adam_state(n)
        step = lambda: ctx.clip_adam(p, g, m, v, powers, lr, 0.9, 0.999, 1e-8, 0.5, _lib.CLIP_GLOBAL, 1.0, gn)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if replay:
                graph = hip_ops.Graph()
                graph.begin()
                step()
                graph.end()
                assert np.array_equal(powers.cpu().numpy(), np.array([0.9, 0.999], np.float32))    # captured, not run
                for _ in range(k):
                    graph.launch()
            else:
                for _ in range(k):
                    step()
        stream.synchronize()
        res.append([t.cpu().numpy() for t in (p, m, v, powers, gn)])
        if replay:
            graph.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    assert np.array_equal(res[1][3], np.array([power_chain(0.9, k + 1), power_chain(0.999, k + 1)]))
    ctx.close()


# -- GPU: the loops ----------------------------------------------------------------------------------------------------

def adam_args(**kw):
    from test_learner_gpu import make_args
    kw.setdefault("optimizer", "adam")
    kw.setdefault("beta1", 0.8)
    kw.setdefault("beta2", 0.99)
    return make_args(**kw)


def snapshot(learner):
    import torch
    torch.cuda.synchronize()
    net = learner.network
    return dict(p=net.get_parameters(), m=net.get_parameters(learner.adam_m), v=net.get_parameters(learner.adam_v),
                powers=learner.beta_powers.cpu().numpy().copy())


def check_update(args, arch, pre, post, states, actions, y, adv, lr, gnorm, what):
    """One update: the oracle's gradients at the device's pre-update weights, clipped, through the fp64 Adam step from the
    device's pre-update moments and powers, against what the device holds after it."""
    from oracle import network as onet
    A = args.num_actions
    onehot = np.eye(A, dtype=np.float32)[np.asarray(actions).reshape(-1)]
    _, g = onet.loss_and_grads(pre["p"], states, onehot, np.asarray(y, np.float32), np.asarray(adv, np.float32),
                               args.entropy_regularisation_strength, arch, dtype=np.float64)
    gc, gn = clip_fp64(g, args.clip_norm_type, args.clip_norm)
    assert abs(gnorm - gn) <= 1e-4 * gn, (what, gnorm, gn)
    for k in pre["p"]:
        var_e, m_e, v_e = adam_fp64(pre["p"][k].astype(np.float64), gc[k], pre["m"][k].astype(np.float64),
                                    pre["v"][k].astype(np.float64), pre["powers"], np.float32(lr), args.beta1, args.beta2,
                                    args.e)
        assert np.abs(post["p"][k] - var_e).max() < 2e-5, (what, k)
        assert np.abs(post["m"][k] - m_e).max() < 1e-4, (what, k)
    assert np.array_equal(post["powers"], (pre["powers"] * np.array([args.beta1, args.beta2], np.float32)).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["global", "local"])
def test_device_loop_adam_updates(mode):
    """The device-resident cycle (hipGraph replay) with --optimizer adam: every update against the oracle + fp64 Adam from
    the device's pre-update state; then 20 more cycles replayed as 16 + 4 per launch leave the powers at the chain of 21."""
    from test_learner_gpu import build_learner
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 32, 5, 3
    args = adam_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.05, sampler="numpy", test_seed=11,
                     clip_norm_type=mode, clip_norm=0.5)
    learner, params, env_creator = build_learner(args)
    assert learner.optimizer == "adam" and not hasattr(learner, "rms")
    np.random.seed(args.test_seed)
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, env_creator.device_env_spec, sampler="numpy", use_graph=True)
    for c in range(cycles):
        pre = snapshot(learner)
        ro.run_cycle()
        ro.synchronize()
        post = snapshot(learner)
        check_update(args, "NATURE", pre, post, ro.rollout_states().cpu().numpy(), ro.actions.view(-1).cpu().numpy(),
                     ro.y.cpu().numpy(), ro.adv.cpu().numpy(), learner.lr_dev.item(), learner.gnorm_dev.item(), c)
    assert ro.MULTI == 4 and ro.MULTI_LONG == 16
    ro.run_cycles(20 - cycles)            # 17: one single cycle, then 16 in one launch ...
    ro.synchronize()
    assert np.array_equal(learner.beta_powers.cpu().numpy(), np.array([power_chain(0.8, 21), power_chain(0.99, 21)]))
    ro.run_cycles(20)                     # ... and 16 + 4
    ro.synchronize()
    chain = np.array([power_chain(0.8, 41), power_chain(0.99, 41)], dtype=np.float32)
    assert np.array_equal(learner.beta_powers.cpu().numpy(), chain)
    assert all(np.isfinite(v).all() for v in learner.network.get_parameters().values())
    ro.close()


@pytest.mark.gpu
def test_host_loop_adam_updates():
    """The host-plugin loop (PAACLearner._train_host) with --optimizer adam: each update against the oracle's gradients on
    the feed it trained on + fp64 Adam from the device's pre-update state."""
    from test_learner_gpu import build_learner
    N, T, cycles = 8, 5, 3
    records = []
    args = adam_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=cycles * N * T, host_environments=True, record_feeds=True,
                     synthetic_terminal_p=0.1, test_seed=42, clip_norm_type="global", clip_norm=0.5)
    learner, params, env_creator = build_learner(args)
    args.feed_callback = lambda feed: records.append((feed, snapshot(learner), float(learner.gnorm_dev.item())))
    np.random.seed(args.test_seed)
    first = snapshot(learner)
    learner.train()
    assert len(records) == cycles
    pre = first
    for c, (feed, post, gnorm) in enumerate(records):
        check_update(args, "NIPS", pre, post, feed["states"], feed["actions"], feed["y"], feed["adv"], feed["lr"], gnorm, c)
        pre = post


FEED_B = 10


def _feeds(A, count, seed):
    """(states, one-hot actions, critic targets, advantages, lr) of `count` updates."""
    rs = np.random.RandomState(seed)
    return [(rs.randint(0, 256, (FEED_B, 84, 84, 4)).astype(np.uint8), np.eye(A, dtype=np.float32)[rs.randint(0, A, FEED_B)],
             rs.randn(FEED_B).astype(np.float32), rs.randn(FEED_B).astype(np.float32), 0.01 * (1.0 - 0.1 * k))
            for k in range(count)]


def _train_step(learner, feed):
    """The reference's Session.run([train_step, ...], feed_dict) (paac.py:157-165) with this learner's placeholders."""
    net = learner.network
    states, onehot, y, adv, lr = feed
    learner.session.run([learner.train_step], {net.input_ph: states, net.selected_action_ph: onehot,
                                               net.critic_target_ph: y, net.adv_actor_ph: adv, learner.learning_rate: lr})


def _fresh_learner(args):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    nc, ec = train.get_network_and_environment_creator(args)
    return PAACLearner(nc, ec, args)


def _state(learner):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for _, t in learner.update_state]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_adam_resume_is_bit_identical(fmt):
    """K updates, a forced checkpoint, a fresh learner built from the folder, more updates: the same bits as the learner
    that was never interrupted -- weights, moments and powers (the powers lost would restart bias correction)."""
    from test_learner_gpu import make_args
    args = adam_args(game="pong", arch="NIPS", emulator_counts=4, max_local_steps=2, checkpoint_format=fmt, e=1e-3)
    a = _fresh_learner(args)
    assert a.init_network() == 0                 # an empty folder: initialised (and the checkpoint folders made)
    a.network.initialize(np.random.RandomState(0))
    feeds = _feeds(a.num_actions, 6, seed=5)
    for f in feeds[:3]:
        _train_step(a, f)
    a.global_step = 3
    a.save_vars(force=True)
    b = _fresh_learner(args)
    assert b.init_network() == 3
    assert all(np.array_equal(x, y) for x, y in zip(_state(a), _state(b)))
    assert np.array_equal(_state(b)[3], np.array([power_chain(0.8, 4), power_chain(0.99, 4)]))
    for f in feeds[3:]:
        _train_step(a, f)
        _train_step(b, f)
    sa, sb = _state(a), _state(b)
    for (name, _), x, y in zip(a.update_state, sa, sb):
        assert np.array_equal(x, y), name
    # an RMSProp run's optimizer checkpoint in the folder: an Adam learner refuses it, naming both optimizers
    rms_args = make_args(game="pong", arch="NIPS", emulator_counts=4, max_local_steps=2, checkpoint_format=fmt)
    r = _fresh_learner(rms_args)
    r.init_network()
    r.global_step = 10
    r.save_vars(force=True)
    args.debugging_folder = rms_args.debugging_folder
    c = _fresh_learner(args)
    with pytest.raises(KeyError, match=r"RMSProp.*Adam"):
        c.init_network()


@pytest.mark.gpu
def test_adam_tf_bundle_run_is_evaluated():
    """An Adam run with --checkpoint_format tf: its all-variables network bundle holds the slots and beta1_power /
    beta2_power, and the eval harness (python -m paac_amd.test) restores the network from it and plays."""
    from test_learner_gpu import build_learner
    from paac_amd import logger_utils, tf_bundle
    from paac_amd.session import Saver
    args = adam_args(game="pong", arch="NIPS", emulator_counts=4, max_local_steps=2, max_global_steps=16,
                     checkpoint_format="tf")
    logger_utils.save_args(args, args.debugging_folder)
    learner, _, _ = build_learner(args)
    learner.train()
    path = Saver.latest_checkpoint(os.path.join(args.debugging_folder, "checkpoints"))
    keys = tf_bundle.read(path[:-len(".index")])
    assert "beta1_power" in keys and "beta2_power" in keys
    assert keys["beta1_power"] == power_chain(0.8, 1 + 16 // 8)
    res = subprocess.run([sys.executable, "-m", "paac_amd.test", "-f", args.debugging_folder, "-tc", "2", "-np", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "Performed 2 tests" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
