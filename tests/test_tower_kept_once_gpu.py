"""csrc/tower.h, TowerGeom::cut: the eight-region tower stores every kept conv1 / conv2 pixel from one owner.  A pixel nobody
stored would keep what the forward before left there: the kept rows after observations X and then Y into the same rows must be
the bits a fresh context leaves after Y alone -- for the acting forward that keeps its rows and for the training forward -- and
those bits are the ones the four-region layout stores from its accumulators (conv1) and the oracle's values (conv2, conv3)."""
import functools

import numpy as np
import pytest

from oracle import network as onet

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

A = 4


@functools.lru_cache(maxsize=None)
def _case(B):
    """Parameters, the two sets of observations and the float64 oracle forward of the second: computed once, never modified."""
    rs = np.random.RandomState(300 + B)
    params = onet.init_params("NATURE", A, rs, dtype=np.float32)
    x, y = (rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8) for _ in range(2))
    ref = onet.forward(params, y, "NATURE", dtype=np.float64, keep=True)
    for v in list(params.values()) + [x, y]:
        v.setflags(write=False)
    return params, x, y, ref


def _make(params, B):
    from paac_amd import hip_ops
    ctx = hip_ops.Context(1, A, max_batch=max(2 * B, 16))
    host = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        host[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    p = torch.from_numpy(host).cuda()
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    return ctx, p


def _rows(ctx, lo, hi):
    """Training-set rows [lo, hi) of the three conv layers, on the host."""
    torch.cuda.synchronize()
    return [ctx.debug_activation(20 + i, hi).cpu().numpy().reshape(hi, -1)[lo:hi].copy() for i in (1, 2, 3)]


def _acting(ctx, p, s, B):
    """An acting forward that keeps its rows in training-set rows [B, 2B)."""
    ctx.keep_next_forward(B)
    ctx.forward(p, s, logits=torch.zeros((B, A), device="cuda"))
    return _rows(ctx, B, 2 * B)


def _training(ctx, p, s, B):
    ctx.train_forward_trunk(p, s)
    return _rows(ctx, 0, B)


def _bits_equal(got, want, what):
    for i, (g, w) in enumerate(zip(got, want), 1):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)), "%s: kept conv%d rows" % (what, i)


@pytest.mark.parametrize("B", [1, 3])
def test_every_kept_pixel_is_stored(B):
    from paac_amd import _lib
    params, x, y, ref = _case(B)
    sx, sy = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()

    ctx, p = _make(params, B)
    first = _acting(ctx, p, sx, B)
    acting = _acting(ctx, p, sy, B)
    assert all(not np.array_equal(f, a) for f, a in zip(first, acting))      # X's rows were there to be overwritten
    _training(ctx, p, sx, B)
    training = _training(ctx, p, sy, B)
    ctx.close()

    fresh, q = _make(params, B)
    want_acting = _acting(fresh, q, sy, B)
    want_training = _training(fresh, q, sy, B)
    _bits_equal(acting, want_acting, "acting forward, X then Y against Y alone")
    _bits_equal(training, want_training, "training forward, X then Y against Y alone")
    _bits_equal(acting, training, "acting against training forward")

    # conv1's K loop is the same sequence of products in every region layout, and the four-region layout stores act1 from the
    # accumulators
    for cls in (0, 1, 2):
        _lib.check(fresh.lib.paac_debug_set_tuning(fresh.handle, 11, cls, 4, 0, -1), "set_tuning")
    act1_direct = _training(fresh, q, sy, B)[0]
    for cls in (0, 1, 2):
        _lib.check(fresh.lib.paac_debug_set_tuning(fresh.handle, 11, cls, -1, 0, -1), "set_tuning")
    fresh.close()
    assert np.array_equal(training[0].view(np.uint32), act1_direct.view(np.uint32))

    cache = ref["cache"]
    for i in (2, 3):
        want = cache["a%d" % i].reshape(B, -1)
        err = np.abs(training[i - 1] - want).max()
        print("B=%d conv%d max abs err %.3g of max %.3g" % (B, i, err, np.abs(want).max()))
        assert err <= 1e-5 * np.abs(want).max(), "conv%d" % i
