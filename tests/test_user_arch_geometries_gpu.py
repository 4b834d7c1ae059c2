"""-m gpu: user architectures across the geometries --user_arch accepts (paac_amd/build.py: build_user_arch) against the fp64
oracle.  Every geometry is new kernel code (csrc/net_common.h: UserNet) and takes its own routes: the fc + heads kernel only
where fc_heads_waves(FLAT) > 0 (quarter tiles only where fc_heads_quarter_ok), gemm3 only where FLAT % 32 == 0 above 512
rows (else the generic dmm contraction), the family's MFMA data-gradient forms or the direct data-gradient kernel.  A process
holds one library, so each geometry runs in a child process; the children run four at a time.

Each child checks forward / loss / gradients at batches 1, 17, 64, 65 and 600 (A = 2 and 18, managed and unmanaged weights,
and trained-magnitude weights at one batch), the exact-zero data gradient of input rows no window reads, one clip + RMSProp
step, act_mt (the host-plugin acting step), the device loop against the oracle (N = 8: the three-launch acting step; N = 65:
forward + fused sampler) and the counter-based sampler's fused step against its separate calls."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = [
    ("family3", "16,32,32,256"),
    ("k5", "32:8:4,64:5:2,64:3:1,512"),
    ("two_family", "32:8:4,48:4:2,512"),             # two layers, family dgrad forms; NW = 9, no quarter tiles; FLAT % 32 = 16
    ("two_nw0", "16:8:4,16:4:1,256"),                # two layers, direct dgrad; no fc + heads kernel; FLAT % 32 = 16
    ("gaps", "32:12:4,64:2:3,64:3:1,768"),           # conv2 stride 3 > size 2: unread gap and tail rows; quarter tiles
    ("pointwise", "16:4:2,32:1:1,48:5:5,1024"),      # 41 x 41 conv1, 1 x 1 conv2, an unread tail row below conv3
    ("tiny_fc", "32:8:4,64:4:2,64:8:1,512"),         # 2 x 2 last layer: FLAT 256 < H; no fc + heads kernel
    ("wide", "64:16:4,128:3:2,96:3:2,256"),          # conv1 size 16; NW = 6 without quarter tiles; unread tail rows
]

_CHILD = r"""
import json, sys
import numpy as np
ROOT, SPEC = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import torch
from oracle import network as onet
from oracle import sampler as osamp
from paac_amd import _lib, hip_ops, networks
from paac_amd.build import parse_user_arch
import test_learner_gpu as tl

CONVS, FC = parse_user_arch(SPEC)
NAME = "UGEOM"
onet.ARCHS[NAME] = (CONVS, FC)
networks.define_architecture("USER", CONVS, FC)
assert _lib.user_arch() == (CONVS, FC)
dims, FLAT, _ = onet.layer_dims(NAME)
BMAX = 600


def to_flat(ctx, params):
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return flat


def unread(L):
    # input rows (and columns) of conv layer L that no output window reads: VALID gaps (stride > size) and the tail
    read = np.zeros(L["ih"], dtype=bool)
    for o in range(L["oh"]):
        read[o * L["stride"]:o * L["stride"] + L["kh"]] = True
    return np.flatnonzero(~read)


def forward_checks(ctx, p, s, L, B, A, tag):
    for managed in (False, True):
        ctx.set_managed_weights(managed)
        if managed:
            ctx.pack_weights(p)
        logits, probs, values = (torch.zeros((B, A), device="cuda"), torch.zeros((B, A), device="cuda"),
                                 torch.zeros(B, device="cuda"))
        ctx.forward(p, s, logits, probs, values)
        torch.cuda.synchronize()
        what = "%s managed=%d" % (tag, managed)
        assert np.abs(logits.cpu().numpy() - L["logits"]).max() < 1e-4, what
        assert np.abs(values.cpu().numpy() - L["v"]).max() < 1e-4, what
        assert np.abs(probs.cpu().numpy() - L["pi"]).max() < 1e-5, what
    ctx.set_managed_weights(False)


def grads_case(ctx, params, B, A, seed, tag, check_dz=False):
    rs = np.random.RandomState(seed)
    states = rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)
    idx = rs.randint(0, A, B).astype(np.int32)
    y, adv = rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32)
    p = torch.from_numpy(to_flat(ctx, params)).cuda()
    s = torch.from_numpy(states).cuda()
    grad = torch.zeros(ctx.layout["total"], device="cuda")
    ctx.loss_backward(p, s, torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(adv).cuda(), 0.02, grad)
    torch.cuda.synchronize()
    masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(len(CONVS))}
    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
    dzs = {i: ctx.debug_activation(11 + i, B).cpu().numpy() for i in range(len(CONVS) - 1)} if check_dz else {}
    L, g = onet.loss_and_grads(params, states, np.eye(A)[idx], y, adv, 0.02, NAME, dtype=np.float64, relu_masks=masks)
    gh, gn = grad.cpu().numpy(), onet.global_norm(g)
    for t in ctx.layout["tensors"]:
        err = np.abs(gh[t["offset"]:t["offset"] + t["size"]] - g[t["name"]].reshape(-1)).max()
        assert err < 1e-4 * max(np.abs(g[t["name"]]).max(), 1e-3 * gn), (tag, t["name"], err)
    for i, got in dzs.items():
        # the data gradient below conv layer i + 2: exact zeros where that layer reads nothing, the oracle's elsewhere
        Lc, want = dims[i + 1], L["dz%d" % (i + 1)]
        got = got.reshape(want.shape)
        rows = unread(Lc)
        if len(rows):
            assert not got[:, rows, :, :].any() and not got[:, :, rows, :].any(), (tag, "dz%d unread rows" % (i + 1), rows)
        err = np.abs(got - want).max()
        assert err < 1e-4 * np.abs(want).max(), (tag, "dz%d" % (i + 1), err)
    forward_checks(ctx, p, s, L, B, A, tag)
    return p, grad


unread_rows = {"conv%d" % (i + 2): unread(Lc).tolist() for i, Lc in enumerate(dims[1:])}

# -- forward / loss / gradients at the batch classes, two action counts, managed and unmanaged --------------------------
for A, batches in ((2, (1, 64, 600)), (18, (17, 64, 65, 600))):
    ctx = hip_ops.Context(_lib.ARCH_USER, A, max_batch=BMAX)
    params = onet.init_params(NAME, A, np.random.RandomState(A), dtype=np.float32)
    for B in batches:
        p, grad = grads_case(ctx, params, B, A, 100 + B, "A=%d B=%d" % (A, B), check_dz=B in (17, 600))
    if A == 18:
        # one clip + RMSProp step on the device's own gradient of the last case (global mode, the clip active)
        n = ctx.layout["total"]
        gflat = grad.cpu().numpy()
        gd = {t["name"]: gflat[t["offset"]:t["offset"] + t["size"]].astype(np.float64) for t in ctx.layout["tensors"]}
        clip = 0.5 * onet.global_norm(gd)
        gc, gn_o = onet.clip_by_global_norm(gd, clip, "global")
        p64 = {t["name"]: params[t["name"]].reshape(-1).astype(np.float64) for t in ctx.layout["tensors"]}
        ms64 = {k: np.full_like(v, 1.25) for k, v in p64.items()}
        mom64 = {k: np.zeros_like(v) for k, v in p64.items()}
        lr = np.float32(0.0224)
        p_e, ms_e, mom_e = onet.rmsprop_step(p64, gc, ms64, mom64, float(lr), 0.99, 0.0, 0.1)
        dv = p.clone()
        dms = torch.full((n,), 1.25, device="cuda")
        dmom = torch.zeros(n, device="cuda")
        gn_dev = torch.zeros(1, device="cuda")
        ctx.clip_rmsprop(dv, grad, dms, dmom, torch.tensor([lr], device="cuda"), 0.99, 0.0, 0.1, clip, _lib.CLIP_GLOBAL, 1.0,
                         gn_dev)
        torch.cuda.synchronize()
        assert abs(gn_dev.item() - gn_o) / gn_o < 1e-5
        hv, hms, hmom = dv.cpu().numpy(), dms.cpu().numpy(), dmom.cpu().numpy()
        for t in ctx.layout["tensors"]:
            sl, k = slice(t["offset"], t["offset"] + t["size"]), t["name"]
            assert np.abs(hms[sl] - ms_e[k]).max() < 1e-6, k
            assert np.abs(hmom[sl] - mom_e[k]).max() < 1e-7, k
            assert np.abs(hv[sl] - p_e[k]).max() < 1e-6, k
        # trained-network magnitudes (|logits|, |v| > 3): an absolute 1e-4 is a relative 1e-5 bar there
        st = np.random.RandomState(9).randint(0, 256, (64, 84, 84, 4)).astype(np.uint8)
        scale = 3.5
        while True:
            big = {k: (v * scale).astype(np.float32) for k, v in params.items()}
            ref = onet.forward(big, st, NAME, dtype=np.float64)
            if min(np.abs(ref["logits"]).max(), np.abs(ref["v"]).max()) > 3.0:
                break
            scale *= 1.5
            assert scale < 100, "no trained-magnitude scale"
        grads_case(ctx, big, 64, A, 9, "trained-scale A=18 B=64")
    ctx.close()

# -- act_mt (policy + numpy-parity sampler for host environments): the sampler stream over the probabilities it returns -
for A, N in ((4, 8), (6, 64)):
    ctx = hip_ops.Context(_lib.ARCH_USER, A, max_batch=N)
    params = onet.init_params(NAME, A, np.random.RandomState(3), dtype=np.float32)
    p = torch.from_numpy(to_flat(ctx, params)).cuda()
    rs = np.random.RandomState(21)
    mt = hip_ops.mt_state_from_numpy(rs.get_state(), "cuda")
    for step in range(3):
        st = np.random.RandomState(step).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
        acts = torch.zeros(N, dtype=torch.int32, device="cuda")
        probs, values = torch.zeros((N, A), device="cuda"), torch.zeros(N, device="cuda")
        ctx.act_mt(p, torch.from_numpy(st).cuda(), mt, acts, probs, values)
        torch.cuda.synchronize()
        ref = onet.forward(params, st, NAME, dtype=np.float64)
        assert np.abs(probs.cpu().numpy() - ref["pi"]).max() < 1e-5 and np.abs(values.cpu().numpy() - ref["v"]).max() < 1e-4
        want = osamp.sample_mt_restated(probs.cpu().numpy(), rs)[0]
        assert np.array_equal(acts.cpu().numpy(), want), ("act_mt", A, N, step)
        assert hip_ops.mt_state_to_numpy(mt)[2] == rs.get_state()[2]
    ctx.close()

# -- the device loop against the oracle: the three-launch acting step (N = 8), forward + fused sampler (N = 65) ----------
tl.check_device_loop_matches_oracle("breakout", 8, 5, 2, NAME, False, user_arch=SPEC)
tl.check_device_loop_matches_oracle("seaquest", 65, 2, 1, NAME, False, user_arch=SPEC)

# -- the counter-based sampler (paac_amd.train's default): fused step == separate calls -------------------------------
tl.check_philox_step_equals_separate_calls(_lib.ARCH_USER, NAME, 6, 8)
tl.check_philox_step_equals_separate_calls(_lib.ARCH_USER, NAME, 18, 65)
print("GEOMETRY_OK " + json.dumps(unread_rows))
"""


def _run(spec):
    try:
        return subprocess.run([sys.executable, "-c", _CHILD, ROOT, spec], cwd=ROOT, capture_output=True, text=True,
                              timeout=1500)
    except subprocess.TimeoutExpired as exc:
        return exc


@pytest.fixture(scope="module")
def results():
    with ThreadPoolExecutor(max_workers=4) as ex:       # the fp64 oracle is the long pole: four children share the CPUs
        return dict(zip([g for g, _ in GEOMETRIES], ex.map(_run, [spec for _, spec in GEOMETRIES])))


@pytest.mark.parametrize("gid,spec", GEOMETRIES, ids=[g for g, _ in GEOMETRIES])
def test_user_geometry_matches_the_oracle(results, gid, spec):
    res = results[gid]
    assert not isinstance(res, subprocess.TimeoutExpired), "%s timed out" % spec
    assert res.returncode == 0 and "GEOMETRY_OK" in res.stdout, (spec, res.stdout[-2000:], res.stderr[-6000:])
    unread_rows = json.loads(res.stdout.split("GEOMETRY_OK ", 1)[1].splitlines()[0])
    if gid in ("gaps", "pointwise", "wide"):        # the exact-zero check had rows to look at
        assert any(unread_rows.values()), unread_rows
