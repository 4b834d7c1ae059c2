"""The conv tower launch of a pipelined acting step carries, on its helper waves, the heads finish of the step before and the
frame shift of its own step (csrc/tower.h: RIDER; PAAC_ACT_TOWER_RIDER, read when the context is created: 1 -- the default --
the heads finish, 2 both, 0 neither).  Every route gives the bits of paac_act_step_mt; what a tower did carry is read back from the context
(paac_act_tower_rode: 1 heads finish | 2 frame shift)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_act_pipeline import ENV_OFF, ENV_SEED, STEPS, Run, _context, _raw_pipe, _same

gpu = pytest.mark.gpu
FINISH, SHIFT = 1, 2


def test_finish_record_layout():
    """Host only: the record the tower's heads finish leaves for the sampler -- fp64 conditional probabilities and packed
    thresholds [N][A - 1], fp32 probabilities [N][A], one exact-zero word per helper wave -- at the limits of the routine that
    fills it (32 environments, 7 actions, 64 column groups): disjoint, naturally aligned, a few KB."""
    from paac_amd import _lib
    out = (ctypes.c_int64 * 8)()
    assert _lib.load().paac_act_finish_layout(out, 8) == 0
    size, pj, thr, probs, zero, max_n, max_a, max_tiles = [int(v) for v in out]
    assert (max_n, max_a, max_tiles) == (32, 7, 64)
    d, na = max_n * (max_a - 1), max_n * max_a
    spans = sorted([(pj, 8 * d), (thr, 8 * d), (probs, 4 * na), (zero, 4 * 4)])
    assert spans[0][0] == 0
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1
    assert spans[-1][0] + spans[-1][1] <= size <= 4096
    assert pj % 8 == 0 and thr % 8 == 0 and probs % 4 == 0 and zero % 4 == 0
    assert _lib.load().paac_act_finish_layout(out, 7) != 0


def _rode(ctx):
    return int(ctx.lib.paac_act_tower_rode(ctx.handle))


def _ctx(monkeypatch, mode, arch, A, N, managed=True):
    monkeypatch.setenv("PAAC_ACT_TOWER_RIDER", str(mode))
    return _context(arch, A, N, managed)


_REF = {}


def _reference(arch, A, N):
    """paac_act_step_mt from the shared seed, once per shape: the snapshots after eight and after nine steps and every stack."""
    key = (arch, A, N)
    if key not in _REF:
        from paac_amd.synthetic import terminal_threshold
        ctx, p = _context(arch, A, N, True)
        thr = terminal_threshold(0.15)
        ref = Run(N, A, STEPS + 1)
        for t in range(STEPS):
            ref.step(ctx.act_step_mt, p, t, thr)
        want8 = ref.snapshot(STEPS)
        ref.step(ctx.act_step_mt, p, STEPS, thr, wrap=True)
        want9 = ref.snapshot(STEPS + 1)
        _REF[key] = (want8, want9, ref.stacks.cpu(), ref.wrap.cpu())
        ctx.close()
    return _REF[key]


SHAPES = [("NATURE", 4, 32),      # the headline
          ("NATURE", 7, 32),      # the action corner of the fused heads finish
          ("NATURE", 2, 1),       # one environment, J = 1; it ends an episode at step 4 (test_act_pipeline)
          ("NATURE", 4, 5)]       # a partial 8-row tile, 35 shift units on 40 tower workgroups


@gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("arch,A,N", SHAPES)
def test_ridden_towers_equal_act_step_mt(monkeypatch, arch, A, N, mode):
    """Eight (and nine) consecutive pipelined steps against paac_act_step_mt, bit for bit: probabilities, values, actions, the
    MT19937 state, rewards, masks, episode totals, every stack slot, the wrap copy and the finished ring -- the last debt paid
    by the flush, by a ninth step and by the bootstrap forward."""
    from paac_amd.synthetic import terminal_threshold
    want8, want9, stacks, wrap = _reference(arch, A, N)
    assert want8["fin_n"] > 0
    ctx, p = _ctx(monkeypatch, mode, arch, A, N)
    thr = terminal_threshold(0.15)
    full = FINISH | (SHIFT if mode == 2 else 0)

    a = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        a.step(ctx.act_step_pipe, p, t, thr)
        assert _rode(ctx) == (full if t else full & SHIFT)          # (nothing is owed at the first step)
    ctx.act_step_flush()
    _same(a.snapshot(STEPS), want8, "flush")
    assert torch.equal(a.stacks[:STEPS + 1].cpu(), stacks[:STEPS + 1])

    b = Run(N, A, STEPS + 1)
    for t in range(STEPS + 1):
        b.step(ctx.act_step_pipe, p, t, thr, wrap=t == STEPS)
    _same(b.snapshot(STEPS), want8, "ninth step")
    assert torch.equal(b.stacks.cpu(), stacks) and torch.equal(b.wrap.cpu(), wrap)
    ctx.act_step_flush()
    _same(b.snapshot(STEPS + 1), want9, "ninth step + flush")

    c = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        c.step(ctx.act_step_pipe, p, t, thr)
    ctx.bootstrap_forward_trunk(p, c.stacks[STEPS], 0)
    assert not ctx.act_step_pending() and _rode(ctx) == FINISH      # (the plain tower carries the finish of step T - 1)
    _same(c.snapshot(STEPS), want8, "bootstrap forward")
    assert torch.equal(c.stacks[:STEPS + 1].cpu(), stacks[:STEPS + 1])
    ctx.close()


@gpu
@pytest.mark.parametrize("arch,A,N", [("NATURE", 6, 33), ("NIPS", 2, 5)])
def test_shapes_outside_keep_their_route(monkeypatch, arch, A, N):
    """More than 32 rows (four regions per sample: no eight-region tower) and the two-conv tower (no helper waves): nothing
    rides, and the steps still equal paac_act_step_mt."""
    from paac_amd.synthetic import terminal_threshold
    want8, _, stacks, _ = _reference(arch, A, N)
    ctx, p = _ctx(monkeypatch, 2, arch, A, N)
    thr = terminal_threshold(0.15)
    a = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        a.step(ctx.act_step_pipe, p, t, thr)
        assert _rode(ctx) == 0
    ctx.act_step_flush()
    _same(a.snapshot(STEPS), want8, "unridden")
    assert torch.equal(a.stacks[:STEPS + 1].cpu(), stacks[:STEPS + 1])
    ctx.close()


@gpu
def test_unmanaged_weights_ride_the_kept_rows_tower(monkeypatch):
    """Without managed weights the acting tower is the variant that also stores the kept rows on its helper waves."""
    from paac_amd.synthetic import terminal_threshold
    arch, A, N = "NATURE", 4, 5
    want8, _, stacks, _ = _reference(arch, A, N)
    ctx, p = _ctx(monkeypatch, 2, arch, A, N, managed=False)
    thr = terminal_threshold(0.15)
    a = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        a.step(ctx.act_step_pipe, p, t, thr)
    assert _rode(ctx) == FINISH | SHIFT
    ctx.act_step_flush()
    _same(a.snapshot(STEPS), want8, "kept-rows tower")
    assert torch.equal(a.stacks[:STEPS + 1].cpu(), stacks[:STEPS + 1])
    ctx.close()


@gpu
def test_flush_right_after_a_step_finishes_the_heads_itself(monkeypatch):
    """A debt that no tower follows: the flush finishes the heads from the partials, whatever the switch says."""
    from paac_amd.synthetic import terminal_threshold
    arch, A, N = "NATURE", 4, 32
    ctx, p = _ctx(monkeypatch, 2, arch, A, N)
    thr = terminal_threshold(0.15)
    ref = Run(N, A, 2)
    for t in range(2):
        ref.step(ctx.act_step_mt, p, t, thr)
        want = ref.snapshot(t + 1)
        a = Run(N, A, 2)
        for u in range(t + 1):
            a.step(ctx.act_step_pipe, p, u, thr)
        assert ctx.act_step_pending()
        ctx.act_step_flush()
        _same(a.snapshot(t + 1), want, "flush after %d step(s)" % (t + 1))
        assert torch.equal(a.stacks[:t + 2], ref.stacks[:t + 2])
    ctx.close()


@gpu
def test_aliased_second_copy_is_still_refused(monkeypatch):
    """The tower shifts the frames only where neither stack written is the one it reads.  The entry has always refused such a
    step outright (stacks shifted in place), the second copy included: that stands, nothing is launched, and the step that
    follows takes the ordinary route."""
    from paac_amd.synthetic import terminal_threshold
    arch, A, N = "NATURE", 4, 5
    ctx, p = _ctx(monkeypatch, 2, arch, A, N)
    thr = terminal_threshold(0.15)
    r = Run(N, A, 1)
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)
    from paac_amd import hip_ops
    ctx.prof_enable(True)
    rc = ctx.lib.paac_act_step_pipe(ctx.handle, vp(p), vp(r.stacks[0]), N, vp(r.mt), vp(r.act[0]), vp(r.probs), vp(r.val[0]),
                                    ENV_SEED, ENV_OFF, thr, vp(r.tick), 0, vp(r.stacks[1]), vp(r.stacks[0]), vp(r.rew[0]),
                                    vp(r.msk[0]), vp(r.ep_r), vp(r.ep_l), vp(r.fin), vp(None), vp(None), 0, hip_ops._stream())
    assert rc != 0 and "in place" in ctx.lib.paac_last_error().decode()
    assert not ctx.act_step_pending() and ctx.prof_read() == []
    assert _raw_pipe(ctx, p, r, 0, thr, r.stacks[0], r.stacks[1]) == 0 and _rode(ctx) == SHIFT
    ctx.act_step_flush()
    ctx.prof_enable(False)
    ctx.close()


@gpu
def test_interleaved_routes(monkeypatch):
    """Two contexts in one process, created with the switch at 0 and at 2, stepped alternately from the same seed: each ends in
    the snapshot of paac_act_step_mt."""
    from paac_amd.synthetic import terminal_threshold
    arch, A, N = "NATURE", 4, 32
    want8, _, stacks, _ = _reference(arch, A, N)
    thr = terminal_threshold(0.15)
    c0, p0 = _ctx(monkeypatch, 0, arch, A, N)
    c2, p2 = _ctx(monkeypatch, 2, arch, A, N)
    r0, r2 = Run(N, A, STEPS + 1), Run(N, A, STEPS + 1)
    for t in range(STEPS):
        r0.step(c0.act_step_pipe, p0, t, thr)
        r2.step(c2.act_step_pipe, p2, t, thr)
        assert _rode(c0) == 0 and _rode(c2) == (FINISH | SHIFT if t else SHIFT)
    c2.act_step_flush()
    c0.act_step_flush()
    for r, what in ((r0, "switch 0"), (r2, "switch 2")):
        _same(r.snapshot(STEPS), want8, what)
        assert torch.equal(r.stacks[:STEPS + 1].cpu(), stacks[:STEPS + 1])
    c0.close()
    c2.close()


@gpu
def test_default_carries_the_heads_finish(monkeypatch):
    """With the switch unset the tower carries the heads finish and the fc launch keeps the shift (1: stage 2 measured level)."""
    from paac_amd.synthetic import terminal_threshold
    monkeypatch.delenv("PAAC_ACT_TOWER_RIDER", raising=False)
    ctx, p = _context("NATURE", 4, 5, True)
    r = Run(5, 4, 2)
    for t in range(2):
        r.step(ctx.act_step_pipe, p, t, terminal_threshold(0.15))
    assert _rode(ctx) == FINISH
    ctx.act_step_flush()
    ctx.close()
