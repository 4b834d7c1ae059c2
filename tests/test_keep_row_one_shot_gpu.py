"""paac_keep_next_forward is one shot (include/paac_hip.h): the pending row is the only thing an acting forward takes from the
context instead of from its own arguments (csrc/common.h: ForwardCall).  Who consumes it, who cancels it and which refusal leaves
it pending, read back from the conv activations of the training set (paac_debug_activation 21..23; the kept fc activations lie in
the training set's slab buffer, which has no read-back)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_act_pipeline import Run, _context

pytestmark = pytest.mark.gpu

A, N, MAX_BATCH = 4, 4, 12


def _make():
    ctx, p = _context("NATURE", A, MAX_BATCH, True)
    rs = np.random.RandomState(9)
    a, b = (torch.from_numpy(rs.randint(0, 256, size=(N, 84, 84, 4)).astype(np.uint8)).cuda() for _ in range(2))
    return ctx, p, a, b


def _rows(ctx, r0):
    """Training-set rows [r0, r0 + N) of the three conv layers, on the host."""
    torch.cuda.synchronize()
    return [ctx.debug_activation(20 + i, MAX_BATCH).cpu().numpy().reshape(MAX_BATCH, -1)[r0:r0 + N].copy() for i in (1, 2, 3)]


def _equal(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_one_shot():
    ctx, p, a, b = _make()
    probs = torch.zeros((N, A), device="cuda")
    ctx.keep_next_forward(4)
    ctx.forward(p, a, probs=probs)
    kept = _rows(ctx, 4)
    assert all(np.abs(k).max() > 0 for k in kept)           # a's activations, not what the allocation held
    ctx.forward(p, b, probs=probs)                          # no new keep_next_forward: nothing is kept
    assert _equal(_rows(ctx, 4), kept)
    ctx.close()


def test_bootstrap_forward_cancels_a_pending_row():
    ctx, p, a, b = _make()
    probs = torch.zeros((N, A), device="cuda")
    ctx.keep_next_forward(0)
    ctx.forward(p, a, probs=probs)                          # rows [0, 4) hold something known: a's activations
    was = _rows(ctx, 0)
    ctx.keep_next_forward(0)
    ctx.bootstrap_forward_trunk(p, a, 8)                    # its own rows, and of those the fc activations only
    ctx.forward(p, b, probs=probs)                          # ... so b's are not kept
    assert _equal(_rows(ctx, 0), was)
    ctx.close()


def test_refusal_for_an_owed_sample_leaves_the_row_pending():
    from paac_amd.synthetic import terminal_threshold
    ctx, p, a, b = _make()
    probs = torch.zeros((N, A), device="cuda")
    r = Run(N, A, 1)
    r.step(ctx.act_step_pipe, p, 0, terminal_threshold(0.15))
    assert ctx.act_step_pending()
    ctx.keep_next_forward(0)
    with pytest.raises(RuntimeError, match="paac_act_step_flush"):
        ctx.forward(p, a, probs=probs)
    ctx.act_step_flush()
    ctx.forward(p, a, probs=probs)                          # the row set before the refusal is still honoured
    got = _rows(ctx, 0)
    ctx.close()
    fresh, q, _, _ = _make()
    fresh.keep_next_forward(0)
    fresh.forward(q, a, probs=probs)
    want = _rows(fresh, 0)
    fresh.close()
    assert all(np.abs(w).max() > 0 for w in want)
    assert _equal(got, want)
