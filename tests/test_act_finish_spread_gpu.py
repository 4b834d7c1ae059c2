"""csrc/tower.h, RIDER: the heads finish of the step before rides tower workgroups 0 .. 3, one helper wave each -- workgroup q
finishes rows 8 q .. 8 q + 7 and writes any_zero[q].  The shapes are the row counts at which one more finishing workgroup gets
live rows (8 | 9, 16 | 17, 24 | 25) and the action corner; every route gives the bits of paac_act_step_mt."""
import pytest

torch = pytest.importorskip("torch")

from test_act_pipeline import STEPS, Run, _context, _same

pytestmark = pytest.mark.gpu
FINISH, SHIFT = 1, 2

SHAPES = [("NATURE", 4, 8),       # workgroup 0's rows alone, all of them live
          ("NATURE", 4, 9),       # one live row in workgroup 1
          ("NATURE", 4, 17),      # ... in workgroup 2
          ("NATURE", 4, 25),      # ... in workgroup 3
          ("NATURE", 7, 9)]       # the action corner: every lane of an 8-lane group is an output

_REF = {}


def _reference(arch, A, N):
    """paac_act_step_mt from the shared seed, once per shape: the snapshot after eight steps and every stack."""
    key = (arch, A, N)
    if key not in _REF:
        from paac_amd.synthetic import terminal_threshold
        ctx, p = _context(arch, A, N, True)
        ref = Run(N, A, STEPS)
        for t in range(STEPS):
            ref.step(ctx.act_step_mt, p, t, terminal_threshold(0.15))
        _REF[key] = (ref.snapshot(STEPS), ref.stacks.cpu())
        ctx.close()
    return _REF[key]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("arch,A,N", SHAPES)
def test_spread_finish_equals_act_step_mt(monkeypatch, arch, A, N, mode):
    """Eight pipelined steps and the flush against paac_act_step_mt, bit for bit: probabilities, values, actions, the MT19937
    state, rewards, masks, episode totals, the finished ring and every stack slot."""
    from paac_amd.synthetic import terminal_threshold
    want, stacks = _reference(arch, A, N)
    monkeypatch.setenv("PAAC_ACT_TOWER_RIDER", str(mode))
    ctx, p = _context(arch, A, N, True)
    thr = terminal_threshold(0.15)
    full = FINISH | (SHIFT if mode == 2 else 0)
    a = Run(N, A, STEPS)
    for t in range(STEPS):
        a.step(ctx.act_step_pipe, p, t, thr)
        assert int(ctx.lib.paac_act_tower_rode(ctx.handle)) == (full if t else full & SHIFT)      # (nothing is owed at the first step)
    ctx.act_step_flush()
    _same(a.snapshot(STEPS), want, "flush")
    assert torch.equal(a.stacks.cpu(), stacks)
    ctx.close()
