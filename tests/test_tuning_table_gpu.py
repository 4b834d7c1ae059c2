"""-m gpu: every launch configuration the library instantiates (csrc/net_common.h: PAAC_*_CFGS), not only the rows the default
tuning table holds: tools/tune_gemm.py may write any of them into the table and PAAC_TUNE_OVERRIDE lets a whole run use any.

  1. paac_debug_cfg_known / paac_debug_cfg_body enumerate the ids; their counts are the table sizes net_common.h states, so a
     new table row is covered by 2. without an edit here, and a row the query does not know fails 1.
  2. every known id of a family (forward, data gradient, weight gradient) is forced on all ops of the family, on the per-layer
     route (PAAC_TOWER=0: what a user architecture runs; the stock networks' conv layers run on the towers otherwise), at row
     counts ragged in every GEMM's M, and checked against the float64 oracle with test_hip_network.py's bars.  The profiler
     records say that the per-layer launches ran and, by their instruction mix, on which path (1 fp32 MFMA, 3 exact bf16,
     6 split bf16).
  3. the K split and the XCD-tied grid dimension of a Tune record, forced on the default ids: splits that do not divide the K
     groups, splits that leave empty tail slabs (a forced split skips pick_ksplit's trimming), a split above the fc forward's
     slab count (clamped).
  4. an id outside the tables is refused by paac_debug_set_tuning and by PAAC_TUNE_OVERRIDE (it used to launch nothing)."""
import ctypes
import functools
import hashlib
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import network as onet
from test_hip_network import ARCH_ID, check_activations, make_case, unflatten, upload_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_OF_OP = {0: "conv1_fwd", 1: "conv2_fwd", 2: "conv3_fwd", 3: "fc_fwd", 4: "fc_wgrad", 5: "fc_dgrad", 6: "conv3_wgrad",
                7: "conv3_dgrad", 8: "conv2_wgrad", 9: "conv2_dgrad", 10: "conv1_wgrad"}
OPS = {"fwd": (0, 1, 2, 3), "dgrad": (5, 7, 9), "wgrad": (4, 6, 8, 10)}
OP_TOWER = 11
EXACT, SPLIT, NARROW = 100, 200, 300             # kExactBf16, kSplitBf16, kNarrow
UNKNOWN = -2                                     # paac_debug_cfg_body: an id the launchers refuse
ID_RANGE = range(400)


def _query():
    """-> (known(op, cfg), body(op, cfg)) of the built library, or None when it cannot be loaded (the cases below then fail)."""
    try:
        from paac_amd import _lib
        lib = _lib.load()
    except Exception:
        return None
    return (lambda op, cfg: bool(lib.paac_debug_cfg_known(op, cfg))), (lambda op, cfg: int(lib.paac_debug_cfg_body(op, cfg)))


QUERY = _query()


def _family_ids(family):
    """ids at least one op of the family knows"""
    if QUERY is None:
        return [pytest.param(-1, id="library-not-loadable")]
    return [c for c in ID_RANGE if any(QUERY[0](op, c) for op in OPS[family])]


def _mix_of(op, cfg):
    body = QUERY[1](op, cfg)
    return (6,) if SPLIT <= body < NARROW else (3,) if EXACT <= body < SPLIT else (1,)


# ---- 1. enumeration ---------------------------------------------------------------------------------------------------------
def _header_tables():
    """Table sizes as net_common.h states them: the k*Cfgs constants and the number of X(...) entries of every list."""
    src = open(os.path.join(ROOT, "paac_amd", "csrc", "net_common.h")).read()
    m = re.search(r"constexpr int kFwdCfgs = (\d+), kDgradCfgs = (\d+), kWgradCfgs = (\d+);", src)
    sizes = dict(zip(("kFwdCfgs", "kDgradCfgs", "kWgradCfgs"), map(int, m.groups())))
    joined = src.replace("\\\n", " ")
    for name in ("FWD", "DGRAD", "WGRAD", "FWD_SPLIT", "DGRAD_SPLIT", "WGRAD_SPLIT", "FWD_NARROW"):
        line = re.search(r"#define PAAC_%s_CFGS\(X\)(.*)" % name, joined).group(1)
        sizes[name] = [int(i) for i in re.findall(r"X\((\d+),", line)]
    for name, base in (("kExactBf16", EXACT), ("kSplitBf16", SPLIT), ("kNarrow", NARROW)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == base
    return sizes


def test_known_ids_are_the_tables_of_net_common_h():
    assert QUERY is not None, "libpaac_hip.so could not be loaded"
    known, body = QUERY
    T = _header_tables()
    assert len(T["FWD"]) == T["kFwdCfgs"] and len(T["DGRAD"]) == T["kDgradCfgs"] and len(T["WGRAD"]) == T["kWgradCfgs"]

    def band(op, lo):           # (ids known, ids that run as themselves) in [lo, lo + 100), as offsets
        ks = [c - lo for c in range(lo, lo + 100) if known(op, c)]
        return ks, [k for k in ks if body(op, lo + k) == lo + k]

    for op in OPS["fwd"]:
        assert band(op, 0) == (T["FWD"], T["FWD"]), op
        if op == 0:             # conv1 (u8 frames): the plain and the exact-bf16 path, nothing else
            assert band(op, EXACT) == (T["FWD"], T["FWD"])
            assert band(op, SPLIT) == ([], []) and band(op, NARROW) == ([], [])
            continue
        assert band(op, EXACT) == ([], []), op
        # an entry the split / narrow path does not instantiate is known as its plain form
        assert band(op, SPLIT) == (T["FWD"], T["FWD_SPLIT"]), op
        assert band(op, NARROW) == (T["FWD"], T["FWD_NARROW"] if op in (1, 2) else []), op      # (the fc has no narrow bodies)
        for k in T["FWD"]:
            if k not in T["FWD_SPLIT"]:
                assert body(op, SPLIT + k) == k
    for op in OPS["dgrad"]:
        assert band(op, 0) == (T["DGRAD"], T["DGRAD"]) and band(op, SPLIT) == (T["DGRAD"], T["DGRAD_SPLIT"]), op
        assert band(op, EXACT) == ([], []) and band(op, NARROW) == ([], []), op
    for op in OPS["wgrad"]:
        if op == 10:            # conv1: 64 features per wave only (entries 4 and 5 run as entry 0); exact path for every later band
            alone = [k for k in T["WGRAD"] if k not in (4, 5)]
            assert band(op, 0) == (T["WGRAD"], alone) and band(op, EXACT) == (T["WGRAD"], alone)
            assert band(op, SPLIT) == (T["WGRAD"], []) and band(op, NARROW) == (T["WGRAD"], [])
            assert body(op, 4) == 0 and body(op, EXACT + 5) == EXACT and body(op, SPLIT + 4) == EXACT and body(op, SPLIT + 2) == EXACT + 2
            continue
        assert band(op, 0) == (T["WGRAD"], T["WGRAD"]) and band(op, SPLIT) == (T["WGRAD"], T["WGRAD_SPLIT"]), op
        assert band(op, EXACT) == (T["WGRAD"], []) and band(op, NARROW) == ([], []), op          # fp32 operands: exact = plain
    for op in FAMILY_OF_OP:
        assert known(op, -1) and known(op, -7) and body(op, -1) == -1      # the size heuristic
        assert not known(op, 13) and body(op, 99) == UNKNOWN
    # the tower: region counts, anything else = automatic
    assert all(known(OP_TOWER, c) for c in (-1, 0, 1, 2, 3, 4, 8, 9, 77))
    assert [c for c in range(0, 12) if body(OP_TOWER, c) == c] == [1, 2, 4, 8, 9]
    assert not known(12, 0) and not known(-1, 0)                           # no such op


# ---- 2. every known id of a family ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(arch, A, B):
    """One set of inputs and the oracle's forward per shape, shared by every id (read-only)."""
    params, states, idx, y, adv = make_case(arch, A, B, seed=17)
    ref = onet.forward(params, states, arch, dtype=np.float64, keep=True)
    return params, states, idx, y, adv, ref


_ORACLE_BACKWARD = {}      # (shape, digest of the device's ReLU masks) -> oracle loss terms and gradients


def _oracle_backward(arch, A, B, masks):
    params, states, idx, y, adv, _ = _case(arch, A, B)
    h = hashlib.sha1()
    for k in sorted(masks):
        h.update(np.packbits(masks[k]).tobytes())
    key = (arch, A, B, h.hexdigest())
    if key not in _ORACLE_BACKWARD:
        _ORACLE_BACKWARD[key] = onet.loss_and_grads(params, states, np.eye(A)[idx], y, adv, 0.02, arch, dtype=np.float64,
                                                    relu_masks=masks)
    return _ORACLE_BACKWARD[key]


def _get_tuning(ctx, op, cls):
    from paac_amd import _lib
    c, k, x = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(ctx.lib.paac_debug_get_tuning(ctx.handle, op, cls, ctypes.byref(c), ctypes.byref(k), ctypes.byref(x)), "get_tuning")
    return c.value, k.value, x.value


def _run(monkeypatch, arch, A, B, force, tower="0", once="0", backward=True):
    """Fresh context (PAAC_TOWER / PAAC_FC_DGRAD_ONCE are read at creation), `force` = [(op, class, cfg, ksplit, xcd), ...] written
    into its table, one forward and one whole backward: activations, logits, values, loss terms and every gradient against the
    float64 oracle with the bars of test_hip_network.py (_forward_parity / _backward_parity; ReLU masks from the device).
    -> (gradients by name -- the logits when backward=False --, {family: mix} of the forward, {family: mix} of the training
    forward + backward)."""
    from paac_amd import hip_ops, _lib
    params, states, idx, y, adv, ref = _case(arch, A, B)
    monkeypatch.setenv("PAAC_TOWER", tower)
    monkeypatch.setenv("PAAC_FC_DGRAD_ONCE", once)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    for op, cls, cfg, ks, xcd in force:
        _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, op, cls, cfg, ks, xcd), "set_tuning")
    p = upload_params(ctx, params)
    s = torch.from_numpy(states).cuda()
    logits = torch.zeros((B, A), device="cuda")
    values = torch.zeros((B,), device="cuda")
    ctx.prof_enable(True)
    ctx.forward(p, s, logits, None, values)
    torch.cuda.synchronize()
    fwd = {name: mix for name, b, ms, mix in ctx.prof_read(with_mix=True)}
    check_activations(ctx, ref["cache"], arch, B, 1.0)
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert np.abs(values.cpu().numpy() - ref["v"]).max() < 1e-4
    if not backward:
        ctx.close()
        return logits.cpu().numpy(), fwd, {}
    grad = torch.zeros(ctx.layout["total"], device="cuda")
    loss = torch.zeros(4, device="cuda")
    ctx.loss_backward(p, s, torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(adv).cuda(), 0.02,
                      grad, loss)
    torch.cuda.synchronize()
    bwd = {name: mix for name, b, ms, mix in ctx.prof_read(with_mix=True)}
    ctx.prof_enable(False)
    nconv = 3 if arch == "NATURE" else 2
    masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, B).cpu().numpy() > 0 for i in range(nconv)}
    masks["h"] = ctx.debug_activation(4, B).cpu().numpy() > 0
    flips = sum(int((masks[k].reshape(-1) != (ref["cache"][k].reshape(-1) > 0)).sum()) for k in masks)
    total = sum(m.size for m in masks.values())
    assert flips <= max(4, total * 2e-6), "%d of %d ReLU masks differ from the float64 oracle" % (flips, total)
    L, g_ref = _oracle_backward(arch, A, B, masks)
    lo = loss.cpu().numpy()
    assert abs(lo[0] - L["loss"]) < 1e-4 * max(1.0, abs(L["loss"]))
    assert abs(lo[1] - L["actor"]) < 1e-4 * max(1.0, abs(L["actor"])) and abs(lo[2] - L["critic"]) < 1e-4 * max(1.0, abs(L["critic"]))
    assert abs(lo[3] - L["entropy"].mean()) < 1e-4
    got = unflatten(ctx, grad)
    gn_ref = onet.global_norm(g_ref)
    for name, want in g_ref.items():
        err = np.abs(got[name] - want).max()
        scale = max(np.abs(want).max(), 1e-3 * gn_ref)
        assert err / scale < 1e-4, "%s: max abs err %g (scale %g)" % (name, err, scale)
    ctx.close()
    return got, fwd, bwd


def _assert_per_layer_route(arch, fwd, bwd):
    """The per-layer launches ran, not the towers and not the paired weight gradients."""
    convs = (1, 2, 3) if arch == "NATURE" else (1, 2)
    for i in convs:
        assert "conv%d_fwd" % i in fwd, fwd
    assert "conv_tower" not in fwd and "fc_fwd" in fwd and "heads_fwd" in fwd, fwd
    if bwd:
        for i in convs:
            assert "conv%d_fwd" % i in bwd and "conv%d_wgrad" % i in bwd, bwd
        for i in convs[1:]:
            assert "conv%d_dgrad" % i in bwd, bwd
        assert "fc_wgrad" in bwd and "fc_dgrad" in bwd, bwd
        assert not {"conv_tower", "dgrad_tower", "fc_conv3_wgrad", "conv2_conv1_wgrad"} & set(bwd), bwd


def _force_family(family, cfg, ksplit_of):
    """`cfg` on every op of the family that knows it (another op keeps its default entry), in classes 0 and 1."""
    assert QUERY is not None, "libpaac_hip.so could not be loaded"
    ops = [op for op in OPS[family] if QUERY[0](op, cfg)]
    assert ops
    return ops, [(op, cls, cfg, ksplit_of(op), -1) for op in ops for cls in (0, 1)]


# NATURE A = 6 at 37 rows: ragged in every GEMM's M (the fc sees 37 rows, conv3 37 x 49); NIPS A = 4 at 21 rows.  Up to 64 rows
# the fc forward is the fc + head partials kernel, which reads no table: the fc's forward bodies run at 69 rows.
@pytest.mark.parametrize("arch,A,B", [("NATURE", 6, 37), ("NIPS", 4, 21), ("NATURE", 6, 69)])
@pytest.mark.parametrize("cfg", _family_ids("fwd"))
def test_every_forward_configuration(cfg, arch, A, B, monkeypatch):
    ops, force = _force_family("fwd", cfg, lambda op: 8 if op == 3 else 0)
    _, fwd, _ = _run(monkeypatch, arch, A, B, force, backward=False)
    _assert_per_layer_route(arch, fwd, None)
    for op in ops:
        if FAMILY_OF_OP[op] in fwd and (op != 3 or B > 64):
            assert fwd[FAMILY_OF_OP[op]] == _mix_of(op, cfg), (op, fwd)


# (PAAC_FC_DGRAD_ONCE=0: up to 192 rows the fc data gradient is the split-once kernel otherwise, which reads no table)
@pytest.mark.parametrize("arch,A,B", [("NATURE", 6, 37), ("NIPS", 4, 21)])
@pytest.mark.parametrize("cfg", _family_ids("dgrad"))
def test_every_data_gradient_configuration(cfg, arch, A, B, monkeypatch):
    ops, force = _force_family("dgrad", cfg, lambda op: 0)
    _, fwd, bwd = _run(monkeypatch, arch, A, B, force)
    _assert_per_layer_route(arch, fwd, bwd)
    for op in ops:
        if FAMILY_OF_OP[op] in bwd:
            assert bwd[FAMILY_OF_OP[op]] == _mix_of(op, cfg), (op, bwd)


@pytest.mark.parametrize("arch,A,B", [("NATURE", 6, 37), ("NIPS", 4, 21)])
@pytest.mark.parametrize("cfg", _family_ids("wgrad"))
def test_every_weight_gradient_configuration(cfg, arch, A, B, monkeypatch):
    ops, force = _force_family("wgrad", cfg, lambda op: 1 if op == 4 else 16)
    _, fwd, bwd = _run(monkeypatch, arch, A, B, force)
    _assert_per_layer_route(arch, fwd, bwd)
    for op in ops:
        if FAMILY_OF_OP[op] in bwd:
            assert bwd[FAMILY_OF_OP[op]] == _mix_of(op, cfg), (op, bwd)


# ---- 3. the K split and the XCD knob ----------------------------------------------------------------------------------------
def test_fc_forward_k_splits(monkeypatch):
    """OP_FC_FWD's blockIdx.z split on the default id of its class: 1, 3 (the K stages do not divide over 3 slabs x the body's
    K waves), FC_SPLITS_MAX = 8, and a value above it, which is clamped to 8: the same launch, the same bits."""
    from paac_amd import hip_ops
    arch, A, B = "NATURE", 6, 69
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    cfg, _, xcd = _get_tuning(ctx, 3, 1)
    ctx.close()
    assert cfg >= 0
    out = {ks: _run(monkeypatch, arch, A, B, [(3, 1, cfg, ks, xcd)], tower="1", backward=False)[0]      # oracle bars
           for ks in (1, 3, 8, 100)}
    assert np.array_equal(out[100], out[8])
    assert not np.array_equal(out[1], out[8])                 # the split is really taken from the record
    for ks in (1, 3):
        assert np.abs(out[ks] - out[8]).max() < 2e-5 * max(1.0, np.abs(out[8]).max())


# conv weight gradients at 37 rows on the ids the size heuristic picks there (entry 0: four K waves; conv1 on the exact-bf16
# path).  K groups of 16: conv3 114, conv2 188, conv1 925.  5 divides none of them; 64 x 4 K waves = 256 parts leave conv3's slabs
# 29 .. 63, conv2's 47 .. 63 and conv1's 58 .. 63 empty: grad_finalize_kernel must still sum 64 slabs to the same gradient.
# tower "1": conv2's and conv1's weight gradients share a launch (dmm_pair_kernel) with these splits.
@pytest.mark.parametrize("tower", ["0", "1"])
def test_conv_weight_gradient_k_splits(tower, monkeypatch):
    arch, A, B = "NATURE", 6, 37
    got = {}
    for ks in (1, 5, 64):
        force = [(op, 0, EXACT if op == 10 else 0, ks, 2) for op in (6, 8, 10)]
        got[ks], fwd, bwd = _run(monkeypatch, arch, A, B, force, tower=tower, once="1")       # oracle bars
        if tower == "0":
            _assert_per_layer_route(arch, fwd, bwd)
        else:
            assert "conv2_conv1_wgrad" in bwd and "conv3_wgrad" in bwd, bwd
    for ks in (5, 64):
        for name, want in got[1].items():
            if name.startswith("conv"):
                scale = max(np.abs(want).max(), 1e-6)
                assert np.abs(got[ks][name] - want).max() / scale < 2e-5, (ks, name)
    assert any(not np.array_equal(got[64][n], got[1][n]) for n in got[1] if n.startswith("conv"))     # other slabs did run


@pytest.mark.parametrize("xcd", [-1, 0, 1, 2])
def test_xcd_tied_grid_dimension(xcd, monkeypatch):
    """Every op of the class-1 table row on its default id and K split with the XCD-tied grid dimension forced (the grid is
    padded to a multiple of 8 in that dimension; the padding workgroups must leave at once), per-layer route, 69 rows."""
    from paac_amd import hip_ops
    arch, A, B = "NATURE", 6, 69
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    rows = {op: _get_tuning(ctx, op, 1) for op in FAMILY_OF_OP}
    ctx.close()
    force = [(op, 1, cfg, ks, xcd) for op, (cfg, ks, _) in rows.items() if cfg >= 0]
    assert len(force) >= 10, rows
    _, fwd, bwd = _run(monkeypatch, arch, A, B, force)
    _assert_per_layer_route(arch, fwd, bwd)


# ---- 4. ids outside the tables are refused ----------------------------------------------------------------------------------
@pytest.mark.parametrize("op,cfg", [(1, 13), (1, 250), (1, 399), (1, 1000), (0, 205), (0, 301), (3, 113), (4, 9), (6, 309),
                                    (5, 12), (7, 104), (9, 399), (10, 9)])
def test_set_tuning_refuses_an_unknown_id(op, cfg):
    from paac_amd import hip_ops, _lib
    ctx = hip_ops.Context(ARCH_ID["NATURE"], 4, max_batch=8)
    before = _get_tuning(ctx, op, 1)
    assert ctx.lib.paac_debug_cfg_known(op, cfg) == 0
    with pytest.raises(_lib.PaacHipError, match="configuration id %d" % cfg):
        _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, op, 1, cfg, 0, -1), "set_tuning")
    assert _get_tuning(ctx, op, 1) == before                   # the entry is as it was
    _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, op, 1, -1, 0, -1), "set_tuning")      # the heuristic: always accepted
    assert _get_tuning(ctx, op, 1) == (-1, 0, -1)
    ctx.close()


@pytest.mark.parametrize("override,names", [("1:1:13:0:-1", "1:1:13:0:-1"), ("3:1:4:2:-1,10:0:9:1:2", "10:0:9:1:2"),
                                            ("12:0:0:0:0", "12:0:0:0:0"), ("3:3:0:0:0", "3:3:0:0:0"), ("3:1:four", "3:1:four"),
                                            ("3:1:4:2:-1;6:1:1:64:2", "3:1:4:2:-1;6:1:1:64:2")])
def test_tune_override_refuses_what_it_cannot_apply(override, names, monkeypatch):
    from paac_amd import hip_ops, _lib
    monkeypatch.setenv("PAAC_TUNE_OVERRIDE", override)
    with pytest.raises(_lib.PaacHipError) as e:
        hip_ops.Context(ARCH_ID["NATURE"], 4, max_batch=8)
    assert "PAAC_TUNE_OVERRIDE" in str(e.value) and names in str(e.value), str(e.value)


def test_valid_tune_override_still_applies(monkeypatch):
    from paac_amd import hip_ops
    monkeypatch.setenv("PAAC_TUNE_OVERRIDE", "3:1:4:2:-1,6:1:201:16:2,11:0:4:0:-1,5:2:-1:0:-1,")
    ctx = hip_ops.Context(ARCH_ID["NATURE"], 4, max_batch=8)
    assert _get_tuning(ctx, 3, 1) == (4, 2, -1) and _get_tuning(ctx, 6, 1) == (201, 16, 2)
    assert _get_tuning(ctx, 11, 0) == (4, 0, -1) and _get_tuning(ctx, 5, 2) == (-1, 0, -1)
    ctx.close()
    monkeypatch.setenv("PAAC_TUNE_OVERRIDE", "")
    hip_ops.Context(ARCH_ID["NATURE"], 4, max_batch=8).close()
