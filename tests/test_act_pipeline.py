"""The pipelined acting step (include/paac_hip.h: paac_act_step_pipe): two launches per step -- the conv tower, then the fc
launch, which also shifts the step's frames and carries the sampler of the step before -- against paac_act_step_mt's three."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

STEPS = 8
ENV_SEED, ENV_OFF = 5, 3
# The frame counter stays put over a run of steps (the rollout advances it once per cycle): step id = TICK + t + 1.  At 10, the
# first environment (seed 5, offset 3) ends an episode at step 4 (test_terminal_of_the_lone_environment), so that the finished
# ring is non-empty at N = 1 too.
TICK = 10


def test_terminal_of_the_lone_environment():
    from paac_amd import synthetic
    thr = synthetic.terminal_threshold(0.15)
    ends = [t for t in range(STEPS) if synthetic.lowbias32_int(synthetic.synth_key(ENV_SEED, ENV_OFF, TICK + t + 1) ^ 0x3C6EF372) < thr]
    assert ends == [4]


def _context(arch, A, N, managed):
    from oracle import network as onet
    from paac_amd import hip_ops
    ctx = hip_ops.Context({"NIPS": 0, "NATURE": 1}[arch], A, max_batch=N)
    host = onet.init_params(arch, A, np.random.RandomState(1), dtype=np.float32)
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = host[t["name"]].reshape(-1)
    p = torch.from_numpy(flat).cuda()
    if managed:
        ctx.set_managed_weights(True)
        ctx.pack_weights(p)
    return ctx, p


class Run:
    """The buffers of one run of consecutive steps from the seed every run of a test shares: a stack slot and a row of records
    per step."""

    def __init__(self, N, A, steps, mt_seed=77):
        from paac_amd import hip_ops
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
        self.N, self.A = N, A
        self.stacks = z(steps + 1, N, 84, 84, 4, dtype=torch.uint8)
        self.wrap = z(N, 84, 84, 4, dtype=torch.uint8)
        self.act, self.val = z(steps, N, dtype=torch.int32), z(steps, N)
        self.rew, self.msk = z(steps, N), z(steps, N)
        self.probs = z(N, A)
        self.ep_r, self.ep_l = z(N), z(N, dtype=torch.int32)
        self.fin = z(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32)
        self.tick = torch.full((1,), TICK, dtype=torch.int64, device="cuda")
        self.mt = hip_ops.mt_state_from_numpy(np.random.RandomState(mt_seed).get_state(), "cuda")
        hip_ops.synth_reset(ENV_SEED, ENV_OFF, self.stacks[0], None)

    def step(self, fn, p, t, thr, wrap=False):
        fn(p, self.stacks[t], self.mt, self.act[t], self.probs, self.val[t], ENV_SEED, ENV_OFF, thr, self.tick, t, self.stacks[t + 1],
           self.rew[t], self.msk[t], self.ep_r, self.ep_l, self.fin, stack_out2=self.wrap if wrap else None)

    def snapshot(self, steps):
        """Everything `steps` completed steps leave behind, on the host."""
        torch.cuda.synchronize()
        fin = self.fin.cpu().numpy()
        n = int(fin[0])
        return dict(probs=self.probs.cpu().numpy().copy(), val=self.val[:steps].cpu().numpy().copy(),
                    act=self.act[:steps].cpu().numpy().copy(), rew=self.rew[:steps].cpu().numpy().copy(),
                    msk=self.msk[:steps].cpu().numpy().copy(), mt=self.mt.cpu().numpy().copy(), ep_r=self.ep_r.cpu().numpy().copy(),
                    ep_l=self.ep_l.cpu().numpy().copy(), fin_n=n, fin_r=sorted(fin[2:2 + n].tolist()),
                    fin_l=sorted(fin[2 + 4096:2 + 4096 + n].tolist()))


def _same(got, want, what):
    for k, w in want.items():
        g = got[k]
        ok = np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
        assert ok, "%s: %s differs" % (what, k)


SHAPES = [("NATURE", 4, 32),       # the headline shape: quarter tiles, the heads finished in registers
          ("NATURE", 7, 32),       # ... their corner
          ("NATURE", 6, 33),       # 16-wide tiles, the heads finished through LDS
          ("NATURE", 18, 60),      # N * (A - 1) = 1020: the draw limit
          ("NIPS", 2, 5),          # a partial row tile, the nine-wave fc kernel
          ("NIPS", 18, 16),
          ("NATURE", 4, 1)]


@pytest.mark.parametrize("managed", [False, True])
@pytest.mark.parametrize("arch,A,N", SHAPES)
def test_pipelined_steps_equal_act_step_mt(arch, A, N, managed):
    """Eight (and nine) consecutive pipelined steps against paac_act_step_mt from the same seed, bit for bit: probabilities of the
    last step, values and actions of every step, MT19937 state, rewards, masks, episode totals, every stack written (the
    second copy included) and the finished ring.  The last step's debt is paid by the flush, by one more step, and -- with
    managed weights, which that entry needs -- by the bootstrap forward."""
    from paac_amd.synthetic import terminal_threshold
    ctx, p = _context(arch, A, N, managed)
    thr = terminal_threshold(0.15)
    ref = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        ref.step(ctx.act_step_mt, p, t, thr)
    want8 = ref.snapshot(STEPS)
    ref.step(ctx.act_step_mt, p, STEPS, thr, wrap=True)
    want9 = ref.snapshot(STEPS + 1)
    assert want8["fin_n"] > 0                                   # episodes ended

    # paid by the flush
    a = Run(N, A, STEPS + 1)
    for t in range(STEPS):
        a.step(ctx.act_step_pipe, p, t, thr)
    assert ctx.act_step_pending()
    ctx.act_step_flush()
    assert not ctx.act_step_pending()
    _same(a.snapshot(STEPS), want8, "flush")
    assert torch.equal(a.stacks[:STEPS + 1], ref.stacks[:STEPS + 1])

    # paid by one more step (whose own debt the flush then pays); that step also writes the second copy of its stacks
    b = Run(N, A, STEPS + 1)
    for t in range(STEPS + 1):
        b.step(ctx.act_step_pipe, p, t, thr, wrap=t == STEPS)
    _same(b.snapshot(STEPS), want8, "ninth step")
    assert torch.equal(b.stacks, ref.stacks) and torch.equal(b.wrap, ref.wrap) and torch.equal(b.wrap, ref.stacks[STEPS + 1])
    ctx.act_step_flush()
    _same(b.snapshot(STEPS + 1), want9, "ninth step + flush")

    # paid by the bootstrap forward's fc launch
    if managed:
        c = Run(N, A, STEPS + 1)
        for t in range(STEPS):
            c.step(ctx.act_step_pipe, p, t, thr)
        ctx.bootstrap_forward_trunk(p, c.stacks[STEPS], 0)
        assert not ctx.act_step_pending()
        _same(c.snapshot(STEPS), want8, "bootstrap forward")
        assert torch.equal(c.stacks[:STEPS + 1], ref.stacks[:STEPS + 1])
    ctx.close()


def _raw_pipe(ctx, p, r, t, thr, states, stack_out, raw=None):
    """paac_act_step_pipe itself, past the wrapper's own checks; returns the entry's status."""
    from paac_amd import hip_ops
    N = states.shape[0]
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None else 0)
    return ctx.lib.paac_act_step_pipe(ctx.handle, vp(p), vp(states), N, vp(r.mt), vp(r.act[t]), vp(r.probs), vp(r.val[t]), ENV_SEED,
                                      ENV_OFF, thr, vp(r.tick), t, vp(stack_out), vp(None), vp(r.rew[t]), vp(r.msk[t]),
                                      vp(r.ep_r), vp(r.ep_l), vp(r.fin), vp(raw), vp(None), 0, hip_ops._stream())


def test_refusals_launch_nothing_and_change_nothing():
    from paac_amd import _lib, hip_ops
    from paac_amd.synthetic import terminal_threshold
    arch, A, N = "NATURE", 18, 65
    ctx, p = _context(arch, A, N, True)
    thr = terminal_threshold(0.15)
    ctx.prof_enable(True)
    big = Run(N, A, 2)
    err = lambda: ctx.lib.paac_last_error().decode()
    # shapes outside the small route: more than PAAC_ACT_STEP_MAX_ENVS environments, more than 1024 draws
    assert _raw_pipe(ctx, p, big, 0, thr, big.stacks[0], big.stacks[1]) != 0 and "paac_act_step_mt" in err()
    assert _raw_pipe(ctx, p, big, 0, thr, big.stacks[0][:64], big.stacks[1][:64]) != 0 and "1024" in err()
    r = Run(32, A, 3)
    s0, s1 = r.stacks[0], r.stacks[1]
    # stacks shifted in place; path B
    assert _raw_pipe(ctx, p, r, 0, thr, s0, s0) != 0 and "in place" in err()
    raw = torch.zeros((32, 2, hip_ops.RAW_H, hip_ops.RAW_W), dtype=torch.uint8, device="cuda")
    assert _raw_pipe(ctx, p, r, 0, thr, s0, s1, raw=raw) != 0 and "raw_scratch" in err()
    assert not ctx.act_step_pending() and ctx.prof_read() == []
    # one step, owed: every entry that would read its sample, and every other acting forward, names the flush
    ref = Run(32, A, 3)
    ref.step(ctx.act_step_mt, p, 0, thr)
    want = ref.snapshot(1)
    assert len(ctx.prof_read()) == 3              # (the reference step's three launches)
    r.step(ctx.act_step_pipe, p, 0, thr)
    assert ctx.act_step_pending() and len(ctx.prof_read()) == 2
    n = ctx.layout["total"]
    grad, loss, y = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(32, device="cuda")
    adv, adv_n, stats = torch.zeros(32, device="cuda"), torch.zeros(32, device="cuda"), torch.zeros(2, device="cuda")
    rec = (r.rew[:1], r.msk[:1], r.val[:1])       # the records of a T = 1 rollout; v_boot given: nothing else is missing
    refused = [lambda: r.step(ctx.act_step_mt, p, 1, thr),
               lambda: ctx.forward(p, s1, probs=r.probs),
               lambda: ctx.loss_backward(p, s0, r.act[0], y, y, 0.02, grad, loss),
               lambda: ctx.loss_backward(p, s0, r.act[0], y, y, 0.02, grad, loss, p_old_out=adv),
               lambda: ctx.loss_backward_returns(p, s0, r.act[0], y, *rec, 0.99, adv, adv_n, 0.02, grad, loss),
               lambda: ctx.loss_backward_ppo(p, s0, r.act[0], y, y, adv, 0.1, 0.02, grad, loss, stats),
               lambda: ctx.returns_norm_tick(p, y, *rec, 0.99, adv, adv_n, adv_n),
               lambda: ctx.record_policy(p, r.act[0], 32, y, None, 0),
               # a forward too large to carry the sample in its fc launch
               lambda: ctx.bootstrap_forward_trunk(p, big.stacks[0], 0)]
    for call in refused:
        with pytest.raises(RuntimeError, match="paac_act_step_flush"):
            call()
    assert ctx.act_step_pending() and ctx.prof_read() == []
    ctx.act_step_flush()
    ctx.prof_enable(False)
    _same(r.snapshot(1), want, "after the refusals")
    assert torch.equal(r.stacks[1], ref.stacks[1]) and float(grad.abs().max()) == 0.0
    assert float(adv.abs().max()) == 0.0 and float(adv_n.abs().max()) == 0.0
    ctx.close()


# A geometry without the fc + head partials kernel (csrc/fc_heads.h: fc_heads_waves == 0) is a user architecture, whose library
# a process holds instead of the NIPS geometry: a child process (the library is the one tests/test_user_arch_geometries_gpu.py
# builds for "two_nw0", cached in-tree by its shape).
_NO_FC_HEADS = "16:8:4,16:4:1,256"
_CHILD = r"""
import sys
ROOT, SPEC = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tests")
import numpy as np, torch
from paac_amd import _lib, hip_ops, networks
from paac_amd.build import parse_user_arch
from paac_amd.synthetic import terminal_threshold
import test_act_pipeline as t
convs, fc = parse_user_arch(SPEC)
networks.define_architecture("USER", convs, fc)
assert _lib.user_arch() == (convs, fc)
A, N = 4, 8
ctx = hip_ops.Context(_lib.ARCH_USER, A, max_batch=N)
p = torch.from_numpy(np.random.RandomState(1).randn(ctx.layout["total"]).astype(np.float32) * 0.01).cuda()
thr = terminal_threshold(0.15)
ctx.prof_enable(True)
r, ref = t.Run(N, A, 1), t.Run(N, A, 1)
assert t._raw_pipe(ctx, p, r, 0, thr, r.stacks[0], r.stacks[1]) != 0
assert "fc + head partials" in ctx.lib.paac_last_error().decode()
assert not ctx.act_step_pending() and ctx.prof_read() == []
torch.cuda.synchronize()
for k in ("stacks", "act", "val", "rew", "msk", "probs", "ep_r", "ep_l", "fin", "mt"):
    assert torch.equal(getattr(r, k), getattr(ref, k)), k
ref.step(ctx.act_step_mt, p, 0, thr)          # ... and paac_act_step_mt serves the geometry
torch.cuda.synchronize()
assert len(ctx.prof_read()) > 0
print("REFUSED_OK")
"""


def test_geometry_without_fc_heads_is_refused():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _CHILD, root, _NO_FC_HEADS], cwd=root, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "REFUSED_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


def _device_loop(monkeypatch, N, T, cycles, pipeline, use_graph):
    from test_learner_gpu import build_learner, make_args
    from paac_amd.paac import DeviceRollout
    monkeypatch.setenv("PAAC_ACT_PIPELINE", "1" if pipeline else "0")
    args = make_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="numpy", test_seed=11)
    L, _, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="numpy", use_graph=use_graph)
    assert ro.route == "act_step" and ro.act_pipeline == pipeline
    per_cycle = []
    for _ in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        per_cycle.append([t.cpu().numpy().copy() for t in (ro.actions, ro.values, ro.rewards, ro.masks, ro.y, ro.adv, L.loss_dev)])
    torch.cuda.synchronize()
    state = [t.cpu().numpy().copy() for _, t in L.update_state]
    ro.close()
    return state, per_cycle


@pytest.mark.parametrize("N", [4, 33])        # (33 rows: the 16-wide fc kernel)
def test_device_rollout_equals_the_three_launch_route(monkeypatch, N):
    """DeviceRollout, T = 3, four cycles (both ring parities and the wrap): PAAC_ACT_PIPELINE=0 against the default, graph replay
    and eager -- parameters, RMSProp slots, and every cycle's actions, values, rewards, masks, returns, advantages and loss."""
    want = _device_loop(monkeypatch, N, 3, 4, False, True)
    for use_graph in (True, False):
        got = _device_loop(monkeypatch, N, 3, 4, True, use_graph)
        for a, b in zip(got[0], want[0]):
            assert np.array_equal(a, b)
        for c, (gc, wc) in enumerate(zip(got[1], want[1])):
            for k, (a, b) in enumerate(zip(gc, wc)):
                assert np.array_equal(a, b), "cycle %d, record %d (graph=%s)" % (c, k, use_graph)


def test_launches_of_one_cycle(monkeypatch):
    """One eager cycle at N = 4, T = 3: a tower and an fc launch per forward (T + 1 each), no sampler + env-step launch."""
    from test_learner_gpu import build_learner, make_args
    from paac_amd.paac import DeviceRollout
    monkeypatch.delenv("PAAC_ACT_PIPELINE", raising=False)
    N, T = 4, 3
    args = make_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="numpy", test_seed=11)
    L, _, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="numpy", use_graph=False)
    assert ro.act_pipeline
    L.ctx.prof_enable(True)
    ro.run_cycle()
    ro.synchronize()
    fams = [name for name, _, _ in L.ctx.prof_read()]
    L.ctx.prof_enable(False)
    ro.close()
    assert fams.count("sample_env_step") == 0
    assert fams.count("conv_tower") == T + 1 and fams.count("fc_fwd") == T + 1
