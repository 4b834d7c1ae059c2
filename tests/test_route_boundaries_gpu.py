"""-m gpu: every batch size at which a network call changes kernels, against the float64 oracle, through the C-ABI.

  * 513 rows and up (PAAC_GEMM3_MIN_ROWS): the fc layer on csrc/gemm3.h -- 128-row workgroup tiles, so row counts that are no
    multiple of 128 run its row clamp and its guarded stores; the weight gradient (K = rows, 32 per stage; only when
    rows % 32 == 0) at odd and even stage counts, with the bias gradient from its column sums; the mixed route at
    rows % 32 != 0 (gemm3 data gradient, dmm weight gradient);
  * 192 / 193 rows: the bound of fc_dgrad_once_kernel (csrc/fc_dgrad_once.h), its last row tile ragged at 177 .. 191;
  * 64 / 65 and 512 / 513 rows: batch_class, i.e. the whole tuning-table row, the pairing and the dH planes;
  * 256 / 257 and 512 / 513 rows of the managed acting forward: fc + head partials kernel -> split-K fc -> gemm3.

The bars are those of tests/test_hip_network.py's helpers.  Which kernel ran is read from the profiler: a family's record
carries the MFMA products per fp32 multiply of the body that ran (1 fp32 MFMA, 6 split bf16), and gemm3.h (6) does not read
the tuning table -- so with the dmm bodies of the fc layer forced to a plain fp32 id, a 6 is gemm3 (or the split-once kernel)
and a 1 is dmm."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_fc_dgrad_once_gpu import _run
from test_hip_network import (TRAINED, _backward_parity, _forward_parity, _managed_forward_parity,
                              _trunk_forward_fused_heads_bit_identity)

OP_FC_FWD, OP_FC_WGRAD, OP_FC_DGRAD, OP_CONV3_WGRAD = 3, 4, 5, 6


def _plain_fc(*ops):
    """prepare(): the dmm bodies of the given fc ops on a plain fp32-MFMA id in every batch class (instruction mix 1)."""
    def prepare(ctx):
        from paac_amd import _lib
        for op in ops:
            for cls in (0, 1, 2):
                _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, op, cls, 1, 1 if op == OP_FC_WGRAD else 0, -1), "set_tuning")
    return prepare


def _pair_fc_conv3(ctx):
    """prepare(): the class-1 pairing of the fc and conv3 weight gradients (net_bwd.hip: fc_wgrad_held) in class 2 as well."""
    from paac_amd import _lib
    _plain_fc(OP_FC_FWD, OP_FC_DGRAD)(ctx)
    _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, OP_FC_WGRAD, 2, 1, 1, 0), "set_tuning")
    _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, OP_CONV3_WGRAD, 2, 1, 64, 2), "set_tuning")


def _mixes(records, batch):
    """family -> instruction mix, of the records of `batch` rows"""
    return {name: mix for name, b, ms, mix in records if b == batch}


# ---- 1. backward above 512 rows at ragged row counts ------------------------------------------------------------------
# NATURE 513: one valid row in the fifth 128-row block, rows % 32 != 0; 544: 17 stages of the weight gradient (odd), 4 1/4 row
# blocks; 576: 18 stages, 4 1/2 row blocks.  NIPS (H = 256, FLAT = 2592): 544, and 520 (rows % 32 != 0).
@pytest.mark.parametrize("arch,A,B,scale", [("NATURE", 4, 513, 1.0), ("NATURE", 6, 544, 1.0), ("NATURE", 4, 544, TRAINED),
                                            ("NATURE", 18, 576, 1.0), ("NIPS", 6, 544, 1.0), ("NIPS", 4, 520, 1.0)])
def test_backward_parity_above_512_rows_at_ragged_row_counts(arch, A, B, scale):
    records = []
    _backward_parity(arch, A, B, scale, prepare=_plain_fc(OP_FC_FWD, OP_FC_DGRAD), records=records)   # fc biases included
    got = _mixes(records, B)
    assert got["fc_fwd"] == (6,) and got["fc_dgrad"] == (6,), got           # gemm3.h, not the dmm bodies forced above
    if B % 32 == 0:
        assert got["fc_wgrad"] == (6,) and "fc_conv3_wgrad" not in got, got
    else:       # K = rows is no whole number of 32-deep stages: the weight gradient stays on dmm, alone or paired with conv3's
        assert ("fc_conv3_wgrad" in got) != (got.get("fc_wgrad", (6,)) != (6,)), got


def test_backward_parity_at_513_rows_with_the_weight_gradients_paired():
    """The mixed route with the pairing of the smaller classes: gemm3 data gradient, fc + conv3 weight gradients in one dmm
    launch."""
    records = []
    _backward_parity("NATURE", 4, 513, 1.0, prepare=_pair_fc_conv3, records=records)
    got = _mixes(records, 513)
    assert got["fc_fwd"] == (6,) and got["fc_dgrad"] == (6,), got
    assert got["fc_conv3_wgrad"] == (1, 1) and "fc_wgrad" not in got and "conv3_wgrad" not in got, got


# ---- 2. forward of the same route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,A,B", [("NATURE", 4, 513), ("NATURE", 6, 544), ("NIPS", 6, 513), ("NIPS", 4, 544)])
def test_forward_parity_above_512_rows_at_ragged_row_counts(arch, A, B):
    records = []
    _forward_parity(arch, A, B, 1.0, prepare=_plain_fc(OP_FC_FWD), records=records)
    assert _mixes(records, B)["fc_fwd"] == (6,), records


@pytest.mark.parametrize("A", [4, 18])
@pytest.mark.parametrize("B", [257, 300, 512, 513])
def test_managed_acting_forward_beyond_the_head_partials_kernel(A, B):
    """From 257 rows a managed context runs the tower with plain-row output and the split-K fc (dmm) + per-row heads launch;
    from 513 the fc is gemm3's.  First on the default table, then with the fc's dmm body forced to a plain fp32 id to see which
    of the two kernels the batch takes."""
    _managed_forward_parity(A, B, 1.0)
    records = []
    _managed_forward_parity(A, B, 1.0, prepare=_plain_fc(OP_FC_FWD), records=records)
    got = _mixes(records, B)
    assert "conv_tower" in got and "heads_fwd" in got, got
    assert got["fc_fwd"] == ((6,) if B >= 513 else (1,)), got


# ---- 3. the bound of fc_dgrad_once_kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,A,B", [("NATURE", 4, 177), ("NATURE", 4, 191), ("NATURE", 6, 192), ("NATURE", 4, 193),
                                      ("NIPS", 6, 192)])
def test_backward_parity_around_the_split_once_bound(arch, A, B, monkeypatch):
    monkeypatch.setenv("PAAC_FC_DGRAD_ONCE", "1")
    _backward_parity(arch, A, B, 1.0)
    # ... and which fc data gradient that was: with the generic body on a plain fp32 id, the split-once kernel still shows 6
    records = []
    _backward_parity(arch, A, B, 1.0, prepare=_plain_fc(OP_FC_DGRAD), records=records)
    assert _mixes(records, B)["fc_dgrad"] == ((6,) if B <= 192 else (1,)), records


@pytest.mark.parametrize("trunk", [False, True])
def test_split_once_route_at_its_last_row_count_has_the_generic_routes_bits(trunk, monkeypatch):
    """192 rows, every register tile full: dX and every gradient equal the generic route's bit for bit (Nature above 64 rows:
    test_fc_dgrad_once_gpu.py: test_once_route_against_generic_route)."""
    new, dx1, xf1 = _run(monkeypatch, "1", "NATURE", 4, 192, 1.0, trunk)
    old, dx0, xf0 = _run(monkeypatch, "0", "NATURE", 4, 192, 1.0, trunk)
    assert np.array_equal(xf1, xf0)
    assert np.abs(dx1).max() > 0
    assert np.array_equal(dx1, dx0)
    for name, want in old.items():
        assert np.array_equal(new[name], want), name


def test_first_row_count_beyond_the_split_once_bound_falls_back(monkeypatch):
    """193 rows: no planes are written, the generic route runs, the switch changes no bit."""
    new, dx1, _ = _run(monkeypatch, "1", "NATURE", 4, 193, 1.0, False)
    old, dx0, _ = _run(monkeypatch, "0", "NATURE", 4, 193, 1.0, False)
    assert np.array_equal(dx1, dx0)
    for name in old:
        assert np.array_equal(new[name], old[name]), name


# ---- 4. batch-class edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,A,B", [("NATURE", 4, 64), ("NATURE", 4, 65), ("NIPS", 6, 64), ("NIPS", 6, 65), ("NATURE", 4, 512)])
def test_backward_parity_at_the_batch_class_edges(arch, A, B):
    _backward_parity(arch, A, B, 1.0)


# (16, 32): 512 update rows + 32 bootstrap rows = 544 forward rows -- forward in class 2 (gemm3 fc), backward in class 1
@pytest.mark.parametrize("T,N", [(1, 64), (1, 65), (16, 32)])
@pytest.mark.parametrize("phase", [0, 3])
def test_trunk_forward_with_heads_in_the_backward_at_the_class_edges(T, N, phase):
    _trunk_forward_fused_heads_bit_identity("NATURE", 4, T, N, phase)
