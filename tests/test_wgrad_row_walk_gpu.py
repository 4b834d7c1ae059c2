"""The weight gradients' patch rows are walked, not decomposed (csrc/dmm.h: RowWalk, PAAC_WGRAD_ROW_WALK).

The FRAG_MN A operand of every conv weight gradient used to decompose the row index of each load into (sample, oy, ox) with two
divisions; now the lane's first row is decomposed once, the first row of every later group is reached by a step of 16 with
carries, and the three rows behind it are read off it.
The addresses requested must be the same, load for load:
  * no GPU: a host restatement of the walk next to the division form, every (geometry, first group, k-slot) -- of the method,
    written out again in Python, not of the header itself;
  * -m gpu: the gradient against the float64 oracle at batch rows where K ranges start and end inside a sample and whole
    parts are dead, with the default tuning and with the largest K split forced on every conv weight-gradient op;
  * -m gpu: the same gradients from the build that keeps the division form (paac_amd.build.build_rowdiv), byte for byte.
A process holds one library, so each library computes its gradients in a child process (one per library, shared by the tests).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from paac_amd import build as pbuild       # noqa: E402  (no GPU needed: paths and the compiler driver)

USER_SPEC = "32:8:4,64:5:2,64:3:1,512"     # a 5x5 stride-2 layer: 20 -> 8 -> 6, OPIX 400 / 64 / 36
BATCHES = (1, 2, 3, 5, 33)
TUNINGS = ("default", "maxsplit")
ARCHS = ("NATURE", "NIPS", "USER")


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: the walk against the division form
# ---------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF
OOB = 0x80000000


class Geom(object):
    def __init__(self, IH, IW, C, OH, OW, S, PH, PW, KH, KW):
        self.IH, self.IW, self.C, self.OH, self.OW, self.S, self.PH, self.PW, self.KH, self.KW = IH, IW, C, OH, OW, S, PH, PW, KH, KW
        self.OPIX = OH * OW
        self.KWC = KW * C
        self.PADDED = bool(PH or PW)


def division_offsets(G, ES, GS, g_begin, stages, kq, f_kh, f_kwc, f_ok, k_end):
    """csrc/dmm.h, load_group, PAAC_WGRAD_ROW_WALK=0: one offset per load, in issue order."""
    f_kw = f_kwc // G.C
    out = []
    for g in range(g_begin, g_begin + stages):
        for gs in range(GS):
            k16 = (g * GS + gs) * 16
            for s in range(4):
                r = k16 + 4 * kq + s
                off = OOB
                if f_ok and r < k_end:
                    b, rem = divmod(r, G.OPIX)
                    oy, ox = divmod(rem, G.OW)
                    iy = oy * G.S - G.PH + f_kh
                    ix0 = ox * G.S - G.PW
                    ok = True
                    if G.PADDED:
                        ok = 0 <= iy < G.IH and 0 <= ix0 + f_kw < G.IW
                    if ok:
                        off = ((((b * G.IH + iy) * G.IW + ix0) * G.C + f_kwc) * ES) & M32
                out.append(off)
    return out


class RowWalk(object):
    """csrc/dmm.h: RowWalk (32-bit unsigned offset arithmetic)."""

    def __init__(self, G, ES):
        self.G = G
        self.SX = G.S * G.C * ES
        self.SY = G.S * G.IW * G.C * ES
        self.SB = G.IH * G.IW * G.C * ES
        self.ES = ES

    def start(self, r, f_kh, f_kwc):
        G = self.G
        b, rem = divmod(r, G.OPIX)
        self.oy, self.ox = divmod(rem, G.OW)
        self.off = ((((b * G.IH + self.oy * G.S - G.PH + f_kh) * G.IW + self.ox * G.S - G.PW) * G.C + f_kwc) * self.ES) & M32

    def step(self, N):
        G = self.G
        QB, R = divmod(N, G.OPIX)
        QY, QX = divmod(R, G.OW)
        self.off = (self.off + QB * self.SB + QY * self.SY + QX * self.SX) & M32
        if R != 0:
            if QX != 0:
                self.ox += QX
                cx = self.ox >= G.OW
                if cx:
                    self.ox -= G.OW
                    self.off = (self.off + self.SY - G.OW * self.SX) & M32
                self.oy += QY + 1 if cx else QY
            else:
                self.oy += QY
            if self.oy >= G.OH:
                self.oy -= G.OH
                self.off = (self.off + self.SB - G.OH * self.SY) & M32
            assert 0 <= self.ox < G.OW and 0 <= self.oy < G.OH       # one carry each is enough

    def ahead(self, s):
        G = self.G
        r = RowWalk(G, self.ES)
        r.off, r.oy, r.ox = self.off, self.oy, self.ox
        if s == 0:
            return r
        if not G.PADDED and G.OW > s:
            wx = self.SY - G.OW * self.SX
            wrap = wx + self.SB - G.OH * self.SY if self.oy == G.OH - 1 else wx
            r.off = (self.off + s * self.SX + (wrap if self.ox >= G.OW - s else 0)) & M32
        else:
            for _ in range(s):
                r.step(1)
        return r


def walk_offsets(G, ES, GS, g_begin, stages, kq, f_kh, f_kwc, f_ok, k_end):
    """csrc/dmm.h, load_group, PAAC_WGRAD_ROW_WALK=1."""
    f_kw = f_kwc // G.C
    walk = RowWalk(G, ES)
    walk.start(16 * GS * g_begin + 4 * kq, f_kh, f_kwc)
    walk_end = k_end - 4 * kq if f_ok else -(1 << 30)
    out = []
    for g in range(g_begin, g_begin + stages):
        for gs in range(GS):
            k16 = (g * GS + gs) * 16
            for s in range(4):
                row = walk.ahead(s)
                ok = k16 + s < walk_end
                if G.PADDED:
                    iy = row.oy * G.S - G.PH + f_kh
                    ix = row.ox * G.S - G.PW + f_kw
                    ok = ok and 0 <= iy < G.IH and 0 <= ix < G.IW
                out.append(row.off if ok else OOB)
                if s == 3:
                    walk.step(16)
    return out


def conv_chain(convs):
    """[(filters, size, stride), ...] over 84 x 84 x 4 -> the layers' geometries and the fc one."""
    size, chans, out = 84, 4, []
    for f, k, s in convs:
        o = (size - k) // s + 1
        out.append(Geom(size, size, chans, o, o, s, 0, 0, k, k))
        size, chans = o, f
    out.append(Geom(1, 1, size * size * chans, 1, 1, 1, 0, 0, 1, 1))
    return out


def all_geometries():
    import __graft_entry__ as entry
    geoms = {}
    geoms["nature"] = conv_chain([(32, 8, 4), (64, 4, 2), (64, 3, 1)])
    geoms["nips"] = conv_chain([(16, 8, 4), (32, 4, 2)])
    for spec in entry.USER_ARCHS:
        geoms[spec] = conv_chain(pbuild.parse_user_arch(spec)[0])
    # zero padding (user architectures are VALID today, the contraction's PADDED test is kept): SAME-like layers
    geoms["padded"] = [Geom(9, 9, 4, 9, 9, 1, 1, 1, 3, 3), Geom(10, 7, 2, 5, 4, 2, 2, 1, 5, 3), Geom(3, 3, 4, 2, 2, 2, 1, 1, 3, 3)]
    return [(name, i, G) for name, gl in sorted(geoms.items()) for i, G in enumerate(gl)]


@pytest.mark.parametrize("name,layer,G", all_geometries(), ids=lambda v: None if isinstance(v, Geom) else str(v))
def test_walk_requests_the_addresses_of_the_division_form(name, layer, G):
    """Every first group 0..nstages of a K range of two samples or more (whole samples and parts of them, a K tail that is no
    multiple of 16 where OPIX is none) with every k-slot, both stage widths and both element sizes; from each start a part
    of three stages and the two dead stages behind it, so consecutive starts overlap and every stage of the range is compared
    from several starts.

    Not exhaustive in the lane constants: an unpadded geometry is checked with the two ends of the kernel only, (0, 0) and
    (KH - 1, KWC - 4).  They enter the walk through start() alone, as one term of the first offset, and no step, carry or
    validity test reads them; a padded geometry, whose validity test does, takes every (kh, kw).

    RowWalk above is a transcription by hand of the struct in csrc/dmm.h: this test checks the method, not the header.  An
    edit to dmm.h alone is caught by test_walked_rows_give_the_bits_of_the_division_form, which needs a GPU."""
    batch = max(2, -(-40 // G.OPIX))                     # at least 40 rows: several groups also where OPIX < 16
    K = batch * G.OPIX
    if G.PADDED:
        lanes = [(kh, kw * G.C) for kh in range(G.KH) for kw in range(G.KW)]
    else:
        lanes = [(0, 0), (G.KH - 1, G.KWC - 4 if G.KWC >= 4 else 0)]
    checked = 0
    for ES, GS in ((4, 1), (4, 2), (1, 2), (1, 1)):
        stage = 16 * GS
        nstages = -(-K // stage)
        per_part, dead = 3, 2
        for g_begin in range(nstages + 1):
            g_end = min(g_begin + per_part, nstages)
            k_end = min(K, g_end * stage)
            for kq in range(4):
                for f_kh, f_kwc in lanes:
                    for f_ok in (True, False):
                        args = (G, ES, GS, g_begin, per_part + dead, kq, f_kh, f_kwc, f_ok, k_end)
                        want = division_offsets(*args)
                        assert walk_offsets(*args) == want, (name, layer, ES, GS, g_begin, kq, f_kh, f_kwc)
                        checked += len(want)
    assert checked > 0


# ---------------------------------------------------------------------------------------------------------------------
# -m gpu: gradients of the walked form against the oracle and against the division form
# ---------------------------------------------------------------------------------------------------------------------
_WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch
from oracle import network as onet
from paac_amd import _lib, hip_ops
from paac_amd import build as pbuild

_lib.use_library(%(lib)r)
ARCHS, BATCHES, ORACLE, OUT = %(archs)r, %(batches)r, %(oracle)r, %(out)r
A = 6
CONV_WGRAD_OPS = {6: 0, 8: 0, 10: 100}       # conv3 / conv2 (fp32 MFMA), conv1 (exact bf16): the 64-feature, 4-wave body
MAX_SPLIT = 64                               # W_SPLITS_MAX (csrc/net_common.h)
if "USER" in ARCHS:
    onet.ARCHS["USER"] = pbuild.parse_user_arch(%(spec)r)
ids = {"NIPS": _lib.ARCH_NIPS, "NATURE": _lib.ARCH_NATURE, "USER": _lib.ARCH_USER}
grads, ratios = {}, {}
for arch in ARCHS:
    nconv = len(onet.ARCHS[arch][0]) if arch == "USER" else (3 if arch == "NATURE" else 2)
    for B in BATCHES:
        rs = np.random.RandomState(100 + B)
        params = onet.init_params(arch, A, rs, dtype=np.float32)
        states = rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)
        idx = rs.randint(0, A, B).astype(np.int32)
        y, adv = rs.randn(B).astype(np.float32), rs.randn(B).astype(np.float32)
        want = None
        for tuning in ("default", "maxsplit"):
            ctx = hip_ops.Context(ids[arch], A, max_batch=B)
            if tuning == "maxsplit":
                for op, cfg in CONV_WGRAD_OPS.items():
                    if op == 6 and nconv < 3:
                        continue
                    for cls in (0, 1, 2):
                        _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, op, cls, cfg, MAX_SPLIT, 2), "set_tuning")
            flat = np.zeros(ctx.layout["total"], dtype=np.float32)
            for t in ctx.layout["tensors"]:
                flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
            p, s = torch.from_numpy(flat).cuda(), torch.from_numpy(states).cuda()
            grad = torch.zeros(ctx.layout["total"], device="cuda")
            ctx.loss_backward(p, s, torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(adv).cuda(), 0.02, grad)
            torch.cuda.synchronize()
            gh = grad.cpu().numpy()
            key = "%%s_%%d_%%s" %% (arch, B, tuning)
            grads[key] = gh
            if ORACLE:
                if want is None:        # the masks are the forward's, which the weight gradients' tuning does not touch
                    masks = {"a%%d" %% (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(nconv)}
                    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
                    _, want = onet.loss_and_grads(params, states, np.eye(A)[idx], y, adv, 0.02, arch, dtype=np.float64, relu_masks=masks)
                gn = onet.global_norm(want)
                # the comparison of tests/test_hip_network.py (_backward_parity): max abs error over max(|want|, 1e-3 |g|)
                ratios[key] = {t["name"]: float(np.abs(gh[t["offset"]:t["offset"] + t["size"]] - want[t["name"]].reshape(-1)).max() /
                                                 max(np.abs(want[t["name"]]).max(), 1e-3 * gn)) for t in ctx.layout["tensors"]}
            ctx.close()
np.savez(OUT + ".npz", **grads)
with open(OUT + ".json", "w") as f:
    json.dump(ratios, f)
print("WGRAD_ROWS_OK")
"""


def _rowdiv_library(spec):
    """The division-form build.  The one build() left in the tree is taken as it is only while it is newer than every source
    and header; otherwise it is built now, and a compile error fails the test.  None (a skip) only where there is no
    compiler to build it with."""
    path = pbuild.rowdiv_library(spec)
    if pbuild.library_is_current(path):
        return path
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        return None
    return pbuild.build_rowdiv(spec)


class _Runs(object):
    """One child process per library, started when a test first asks for it."""

    def __init__(self, tmp):
        self.tmp, self.done = tmp, {}

    def get(self, user, rowdiv):
        key = (user, rowdiv)
        if key not in self.done:
            self.done[key] = self._run(user, rowdiv)
        return self.done[key]

    def _run(self, user, rowdiv):
        spec = USER_SPEC if user else None
        if rowdiv:
            lib = _rowdiv_library(spec)
            if lib is None:
                return None
        elif user:
            lib = pbuild.user_arch_library(*pbuild.parse_user_arch(spec))[0]      # __graft_entry__.USER_ARCHS: build() made it
            if not os.path.exists(lib):
                lib = pbuild.build_user_arch(*pbuild.parse_user_arch(spec))
        else:
            lib = pbuild.LIB
        out = os.path.join(self.tmp, "grads_%d_%d" % (user, rowdiv))
        script = _WORKER % dict(root=ROOT, lib=lib, archs=("USER",) if user else ("NATURE", "NIPS"), batches=BATCHES,
                                oracle=not rowdiv, out=out, spec=USER_SPEC)
        res = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and "WGRAD_ROWS_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
        with open(out + ".json") as f:
            ratios = json.load(f)
        return dict(np.load(out + ".npz")), ratios


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return _Runs(str(tmp_path_factory.mktemp("wgrad_rows")))


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("arch", ARCHS)
def test_gradient_against_the_oracle(runs, arch, B, tuning):
    """The flat gradient of paac_loss_backward against the float64 oracle, tests/test_hip_network.py's comparison and bar:
    every tensor within 1e-4 of max(|gradient|, 1e-3 of the global norm)."""
    _, ratios = runs.get(arch == "USER", False)
    for name, ratio in ratios["%s_%d_%s" % (arch, B, tuning)].items():
        print("%s B=%d %s %s: err / scale = %.3g" % (arch, B, tuning, name, ratio))
        assert ratio < 1e-4, "%s: err / scale %g" % (name, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ARCHS)
def test_walked_rows_give_the_bits_of_the_division_form(runs, arch):
    """Same addresses, load for load, so the same sums: the default build and the PAAC_WGRAD_ROW_WALK=0 build give byte-equal
    gradients at every batch and both tunings."""
    old = runs.get(arch == "USER", True)
    if old is None:
        pytest.skip("no current division-form library in the tree and no hipcc to build one")
    new = runs.get(arch == "USER", False)
    for B in BATCHES:
        for tuning in TUNINGS:
            key = "%s_%d_%s" % (arch, B, tuning)
            assert new[0][key].tobytes() == old[0][key].tobytes(), key
            assert np.any(new[0][key] != 0), key
