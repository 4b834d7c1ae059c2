"""-m gpu: the fc data gradient with operands split once (csrc/fc_dgrad_once.h, PAAC_FC_DGRAD_ONCE=1, the default) against the
float64 oracle and against the generic route (PAAC_FC_DGRAD_ONCE=0), through the C-ABI.  The switch is read when a context is
created: a fresh context per setting."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_hip_network import ARCH_ID, SATURATED, TRAINED, _backward_parity, make_case, unflatten, upload_params

# rows: one ragged row tile / two and a half / the headline's ten; NIPS: H = 256, FLAT = 2592 (the other column count)
CASES = [("NATURE", 4, 5, 1.0), ("NATURE", 4, 40, 1.0), ("NATURE", 4, 40, TRAINED), ("NATURE", 4, 160, 1.0),
         ("NIPS", 6, 24, 1.0), ("NIPS", 6, 24, SATURATED)]


def _run(monkeypatch, once, arch, A, B, scale, trunk):
    """One whole backward on a fresh context -> (gradients by name, dX of the fc layer, last conv output).  trunk: the training
    forward stops after the fc layer and the backward's first launch finishes the heads (heads_train_kernel on the three-conv
    network) instead of the separate heads-gradient launch (heads_bwd_kernel): the two producers of dH."""
    from paac_amd import hip_ops
    monkeypatch.setenv("PAAC_FC_DGRAD_ONCE", once)
    params, states, idx, y, adv = make_case(arch, A, B, seed=11, weight_scale=scale)
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B)
    p = upload_params(ctx, params)
    s = torch.from_numpy(states).cuda()
    grad = torch.zeros(ctx.layout["total"], device="cuda")
    dev = [torch.from_numpy(a).cuda() for a in (idx, y, adv)]
    if trunk:
        ctx.train_forward_trunk(p, s)
    ctx.loss_backward(p, s, *dev, 0.02, grad, forward_done=trunk)
    torch.cuda.synchronize()
    nconv = 3 if arch == "NATURE" else 2
    dx = ctx.debug_activation(10 + nconv, B).cpu().numpy()
    xf = ctx.debug_activation(nconv, B).cpu().numpy()
    got = unflatten(ctx, grad)
    ctx.close()
    return got, dx, xf


@pytest.mark.parametrize("arch,A,B,scale", CASES)
def test_once_route_meets_the_oracle_bars(arch, A, B, scale, monkeypatch):
    """(a) the bars of test_backward_parity, on the new route."""
    monkeypatch.setenv("PAAC_FC_DGRAD_ONCE", "1")
    _backward_parity(arch, A, B, scale)


@pytest.mark.parametrize("trunk", [False, True])
@pytest.mark.parametrize("arch,A,B,scale", CASES)
def test_once_route_against_generic_route(arch, A, B, scale, trunk, monkeypatch):
    """(b) everything downstream of dX -- the conv layers' gradients -- on the two routes, to test_backward_parity's bar (1e-4
    of the tensor's largest entry, floored at 1e-3 of the global norm); (c) dX, read back through the debug-activation entry, is
    bit-zero wherever the kept conv output is 0 (about half of it)."""
    new, dx1, xf1 = _run(monkeypatch, "1", arch, A, B, scale, trunk)
    old, dx0, xf0 = _run(monkeypatch, "0", arch, A, B, scale, trunk)
    assert np.array_equal(xf1, xf0)
    gn = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in old.values()))
    for name, want in old.items():
        if not name.startswith("conv"):
            assert np.array_equal(new[name], want), name        # heads and fc weight gradient: untouched by the switch
            continue
        err = np.abs(new[name] - want).max()
        bar = max(np.abs(want).max(), 1e-3 * gn)
        assert err / bar < 1e-4, "%s: max abs err %g (scale %g)" % (name, err, bar)
    assert np.abs(dx1 - dx0).max() <= 1e-4 * max(np.abs(dx0).max(), 1e-30)
    assert np.abs(dx1).max() > 0
    if arch == "NATURE" and B > 64:
        # where the generic route runs its tuned split-bf16 body (Nature, 65 to 512 rows: four K quarters of 128, summed in
        # order) the new kernel keeps its sums term for term: dX, and with it a whole training run, has the same bits
        assert np.array_equal(dx1, dx0)
        for name, want in old.items():
            assert np.array_equal(new[name], want), name
    elif B >= 16 and scale == 1.0:
        assert not np.array_equal(dx1, dx0)                     # elsewhere the generic route is the fp32 MFMA: other roundings
    for dx, xf in ((dx1, xf1), (dx0, xf0)):
        assert (xf <= 0).sum() > xf.size // 8
        assert np.all(dx.view(np.uint32)[xf <= 0] == 0)          # +0.0, not a small number and not -0.0


def test_rows_beyond_the_bound_fall_back(monkeypatch):
    """(d) both producers of dH write the planes, so the case without planes is a batch beyond the kernel's 192 rows: no planes
    are written, the generic route runs -- the oracle bars hold and the switch changes no bit."""
    monkeypatch.setenv("PAAC_FC_DGRAD_ONCE", "1")
    _backward_parity("NATURE", 4, 200, 1.0)
    new, dx1, _ = _run(monkeypatch, "1", "NATURE", 4, 200, 1.0, False)
    old, dx0, _ = _run(monkeypatch, "0", "NATURE", 4, 200, 1.0, False)
    assert np.array_equal(dx1, dx0)
    for name in old:
        assert np.array_equal(new[name], old[name]), name
