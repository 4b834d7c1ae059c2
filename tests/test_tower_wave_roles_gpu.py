"""csrc/tower.h, TowerGeom::ROLES: at the small regions (up to 32 rows, 8 regions of 4x2 per sample) conv2 / conv3 run on
four GEMM waves -- one per channel tile over all of K, no partial sums through LDS -- and waves 4-7 write the kept fp32
conv1 / conv2 rows (WRITE_ALL) from the three bf16 planes in LDS while the GEMMs run.

The cases go through the same C entries as the other tower tests and do not depend on which schedule the library was built
with: a library built with -DPAAC_T_ROLES=0 (python -m paac_amd.build --ksplit, selected with PAAC_HIP_LIB) runs the K-split
schedule through the same cases."""
import functools

import numpy as np
import pytest

from oracle import network as onet

TRAINED = 3.5        # tests/test_hip_network.py: weights at which logits and values are of order 5-20
A = 4


def _split3(x):
    """split3_bf16 / store_split4 on the host: truncate to bf16, subtract (exact), repeat."""
    x = np.asarray(x, dtype=np.float32)
    trunc = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    hi = trunc(x)
    r1 = x - hi
    mid = trunc(r1)
    r2 = r1 - mid
    return hi, mid, trunc(r2)


def test_planes_rebuild_the_fp32_value_exactly():
    """What the helper waves rely on: (lo + mid) + hi, in fp32, is the value the planes were split from, bit for bit, for 0
    and for every x >= 2^-103 (as after ReLU).  Below that the remainders x - hi, r1 - mid are subnormal and their bf16
    truncation drops bits; a conv output that small and not 0 would need bias and products to cancel 70 binary orders below
    the rounding step of the sum itself."""
    rs = np.random.RandomState(0)
    x = np.concatenate([
        np.abs(rs.randn(200000)).astype(np.float32) * np.float32(10.0) ** rs.randint(-20, 6, 200000).astype(np.float32),
        rs.randint(0x0C000000, 0x7F7FFFFF, 200000).astype(np.uint32).view(np.float32),      # any finite pattern from 2^-103 up
        np.array([0.0, 1.0, 255.0, 2.0 ** -103, 2.0 ** -103 * (2.0 - 2.0 ** -23), 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23,
                  3.3895314e38], np.float32)])
    x = x[(x == 0) | (x >= np.float32(2.0 ** -103))]
    assert x.size > 399000
    hi, mid, lo = _split3(x)
    back = (lo + mid) + hi
    assert back.dtype == np.float32
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))


def _states(B, seed):
    """u8 observations with constant frames: sample 0 stacks an all-0 and an all-255 frame with two random ones; with three
    or more samples, sample 1 is all 0 and the last one all 255."""
    rs = np.random.RandomState(seed)
    s = rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)
    s[0, :, :, 0] = 0
    s[0, :, :, 1] = 255
    if B >= 3:
        s[1] = 0
        s[B - 1] = 255
    return s


@functools.lru_cache(maxsize=None)
def _case(B, scale):
    """Parameters, observations and the float64 oracle forward of a case: computed once, shared, never modified."""
    rs = np.random.RandomState(100 + B)
    params = onet.init_params("NATURE", A, rs, dtype=np.float32)
    if scale != 1.0:
        params = {k: (v * scale).astype(np.float32) for k, v in params.items()}
    states = _states(B, 200 + B)
    ref = onet.forward(params, states, "NATURE", dtype=np.float64, keep=True)
    for v in list(params.values()) + [states]:
        v.setflags(write=False)
    return params, states, ref


def _unpack_act3(packed, B):
    """fc_heads_kernel's A-fragment order [row tile b/16][K group k/16][(k%16)/4 * 16 + b%16][k%4] -> rows [B, 3136]."""
    tiles = (B + 15) // 16
    v = packed.reshape(tiles, 3136 // 16, 4, 16, 4)            # [tile][k group][q = (k%16)/4][r = b%16][e = k%4]
    return v.transpose(0, 3, 1, 2, 4).reshape(tiles * 16, 3136)[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, TRAINED])
@pytest.mark.parametrize("B", [1, 5, 16, 17, 32])
def test_tower_wave_roles(B, scale):
    torch = pytest.importorskip("torch")
    from paac_amd import _lib, hip_ops
    params, states, ref = _case(B, scale)
    cache = ref["cache"]
    pad = (B + 15) // 16 * 16                                   # the fragment-order act3 buffer is padded to whole row tiles
    MB = max(2 * B, pad)
    ctx = hip_ops.Context(1, A, max_batch=MB)
    lay = ctx.layout
    host = np.zeros(lay["total"], dtype=np.float32)
    for t in lay["tensors"]:
        host[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    p = torch.from_numpy(host).cuda()
    s = torch.from_numpy(states).cuda()
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    rows = lambda what, n_rows, lo, hi: ctx.debug_activation(what, n_rows).cpu().numpy().reshape(n_rows, -1)[lo:hi]

    # (1) a plain WRITE_ALL training forward of the rows: training-set rows [0, B)
    ctx.train_forward_trunk(p, s)
    torch.cuda.synchronize()
    train = [rows(20 + i, B, 0, B) for i in (1, 2, 3)]
    for i, got in enumerate(train, 1):
        want = cache["a%d" % i].reshape(B, -1)
        err = np.abs(got - want).max()
        print("B=%d scale=%g WRITE_ALL training forward: conv%d max abs err %.3g of max %.3g" % (B, scale, i, err, np.abs(want).max()))
        assert err <= 1e-5 * np.abs(want).max(), "conv%d" % i       # the bar of check_activations
    assert np.abs(train[2] - cache["a3"].reshape(B, -1)).max() < 1e-4

    # conv1's K loop is the same sequence of products in every region layout, and the 4-region layout stores act1 from the
    # accumulators: what the helper waves rebuild from the planes has the same bits
    for cls in (0, 1, 2):
        _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, 11, cls, 4, 0, -1), "set_tuning")
    ctx.train_forward_trunk(p, s)
    torch.cuda.synchronize()
    act1_direct = rows(21, B, 0, B)
    for cls in (0, 1, 2):
        _lib.check(ctx.lib.paac_debug_set_tuning(ctx.handle, 11, cls, -1, 0, -1), "set_tuning")
    assert np.array_equal(train[0].view(np.uint32), act1_direct.view(np.uint32))

    # (2) the acting forward, WRITE_ALL = false: conv3's output only, in fragment order
    logits, values = torch.zeros((B, A), device="cuda"), torch.zeros((B,), device="cuda")
    ctx.forward(p, s, logits=logits, values=values)
    torch.cuda.synchronize()
    act3 = _unpack_act3(ctx.debug_activation(3, pad).cpu().numpy(), B)
    err3 = np.abs(act3 - cache["a3"].reshape(B, -1)).max()
    print("B=%d scale=%g acting forward: conv3 max abs err %.3g of max %.3g" % (B, scale, err3, np.abs(cache["a3"]).max()))
    assert err3 < 1e-4
    assert np.abs(logits.cpu().numpy() - ref["logits"]).max() < 1e-4
    assert np.abs(values.cpu().numpy() - ref["v"]).max() < 1e-4

    # (3) the acting forward that keeps its rows (WRITE_ALL = true, fragment-order act3 + a plain-row copy), twice: rows
    # [B, 2B) of the training set.  Pixels in the region overlaps are written by two workgroups -- with the same value if
    # both launches leave the same bits
    kept_runs = []
    for rep in range(2):
        ctx.keep_next_forward(B)
        logits_k = torch.zeros((B, A), device="cuda")
        ctx.forward(p, s, logits=logits_k)
        torch.cuda.synchronize()
        kept = [rows(20 + i, 2 * B, B, 2 * B) for i in (1, 2, 3)]
        packed = _unpack_act3(ctx.debug_activation(3, pad).cpu().numpy(), B)
        kept_runs.append(kept + [packed, logits_k.cpu().numpy()])
    for x, y in zip(*kept_runs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    k1, k2, k3, packed, logits_k = kept_runs[0]
    # kept rows: the bits a plain WRITE_ALL training forward of the same rows leaves
    for i, (got, want) in enumerate(zip((k1, k2, k3), train), 1):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "kept conv%d rows" % i
    # act3_packed and act3_rows hold the same values
    assert np.array_equal(packed.view(np.uint32), k3.view(np.uint32))
    assert np.abs(packed - cache["a3"].reshape(B, -1)).max() < 1e-4
    assert np.abs(logits_k - ref["logits"]).max() < 1e-4
    ctx.close()
