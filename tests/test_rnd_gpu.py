"""-m gpu: --explore_kind rnd (spec and float64 twin: paac_amd/rnd.py; contract: include/paac_hip.h, paac_rnd_bonus).

The device sums on fp32 matrix instructions, the twin in float64: every compared quantity differs by fp32 accumulation error
only, and no bar can be derived.  So the scale is MEASURED ON THE HOST: the twin run in float32 (numpy float32 matmuls) against
the twin in float64 on the same inputs; per quantity, dev = max |float32 - float64| / max |float64|, and the bar is 8 x dev (the
kernel sums in another order than numpy, and a tiled fixed-order sum and a pairwise one can each be off by the same bound in
opposite directions).  Never from the kernel's output.  `reference` computes the bars at run time; the float32 twin's
deviations (the larger of the two calls) were, as dev (bar = 8 x):

rows        raw    bonus  rewards     grad       W1       b1       W2       b2      mom      var        m
1       1.4e-07  1.4e-07  0.0e+00  3.3e-07  1.0e-07  9.2e-08  1.1e-07  6.1e-08  2.6e-07  4.4e-07  2.8e-07
17      2.4e-07  2.0e-07  2.3e-08  1.6e-07  1.1e-07  7.5e-08  1.1e-07  6.1e-08  1.5e-07  3.3e-07  5.7e-08
33      3.2e-07  3.1e-07  8.3e-08  2.2e-07  1.0e-07  8.2e-08  1.1e-07  5.4e-08  1.9e-07  3.1e-07  3.1e-09
160     3.7e-07  3.7e-07  6.7e-08  5.0e-07  1.0e-07  7.7e-08  9.7e-08  5.6e-08  4.7e-07  9.3e-07  1.3e-08
2688    4.4e-07  4.2e-07  6.3e-08  1.8e-06  1.0e-07  8.3e-08  1.1e-07  5.4e-08  1.9e-06  3.4e-06  1.1e-08
"""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from paac_amd import rnd

SEED, BETA, LR, EPS = 3, 0.25, 1e-3, 1e-4          # (eps 1e-4: Adam's g / (sqrt(v) + eps) well-conditioned in every element)
ROWS = [1, 17, 33, 160, 2688]          # a partial tile, a tile boundary, two tiles + 1, the headline shape, more tiles than CUs
PARTS = dict(W1=slice(rnd.W1, rnd.B1), b1=slice(rnd.B1, rnd.W2), W2=slice(rnd.W2, rnd.B2), b2=slice(rnd.B2, rnd.NET))


def twin_calls(twin, stacks_per_call, beta, lr, eps, rewards):
    """-> per call a dict of what the entry leaves behind, from `twin`."""
    out, rewards = [], rewards.copy()
    for x in stacks_per_call:
        raw, bonus, g = twin.bonus(x, beta, lr, rewards, eps=eps)
        q = dict(raw=raw, bonus=bonus, rewards=rewards.copy(), grad=g, mom=twin.mom, var=twin.var, m=np.array([twin.m]))
        q.update({name: twin.predictor[at] for name, at in PARTS.items()})
        out.append({k: np.asarray(v, dtype=np.float64) for k, v in q.items()})
    return out


def bars_of(want, single):
    """Per call and quantity: 8 x (the float32 run's largest deviation relative to the quantity's largest magnitude) x that magnitude."""
    dev = {k: max(np.abs(s[k] - w[k]).max() / np.abs(w[k]).max() for w, s in zip(want, single)) for k in want[0]}
    return [{k: 8.0 * dev[k] * np.abs(w[k]).max() for k in w} for w in want]


@functools.lru_cache(maxsize=None)
def reference(rows):
    """-> (stacks, rewards before, per call the float64 twin's quantities, per call their bars)."""
    rs = np.random.RandomState(rows)
    x, rewards = rs.randint(0, 256, (rows, 84 * 84 * 4)).astype(np.uint8), rs.randn(rows).astype(np.float32)
    want = twin_calls(rnd.Twin(SEED), [x, x], BETA, LR, EPS, rewards)
    return x, rewards, want, bars_of(want, twin_calls(rnd.Twin(SEED, np.float32), [x, x], BETA, LR, EPS, rewards))


def device_calls(rows, captured=False):
    """The two calls on a fresh block -> (per call the same dict from the device, the block)."""
    import torch
    from paac_amd import hip_ops
    dev = torch.device("cuda")
    x, rewards0, _, _ = reference(rows)
    block = hip_ops.rnd_block(dev, SEED, rows)
    states, rewards = torch.from_numpy(x).to(dev), torch.from_numpy(rewards0).to(dev)
    bonus, grad = torch.zeros(rows, device=dev), torch.zeros(rnd.NET, device=dev)
    call = lambda: hip_ops.rnd_bonus(block, states, BETA, LR, rewards, bonus, grad, eps=EPS)
    stream, out = torch.cuda.Stream(), []
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        if captured:
            graph = hip_ops.Graph()
            graph.begin()
            call()
            graph.end()
        for _ in range(2):
            graph.launch() if captured else call()
            stream.synchronize()
            q = dict(raw=block.raw, bonus=bonus, rewards=rewards, grad=grad, mom=block.adam_m, var=block.adam_v, m=block.norm[:1],
                     target=block.target, ticket=block.scratch[:1])
            q.update({name: block.predictor[at] for name, at in PARTS.items()})
            out.append({k: v.cpu().numpy().copy() for k, v in q.items()})
        if captured:
            graph.close()
    return out


@pytest.mark.parametrize("rows", ROWS)
def test_entry_equals_the_twin_over_two_calls(rows):
    _, _, want, bars = reference(rows)
    got = device_calls(rows)
    target = rnd.draw(SEED, rnd.TARGET_STREAM)
    for call in range(2):          # the second call: the stepped weights, the EMA branch, the scratch as the first left it
        errors = {k: np.abs(got[call][k].astype(np.float64) - want[call][k]).max() for k in want[call]}
        print(rows, call, {k: "%.3g / %.3g" % (errors[k], bars[call][k]) for k in errors})
        assert all(errors[k] <= bars[call][k] for k in errors), (call, {k: (errors[k], bars[call][k]) for k in errors if errors[k] > bars[call][k]})
        assert got[call]["target"].tobytes() == target.tobytes() and got[call]["ticket"][0] == 0


@pytest.mark.parametrize("rows", [33, 160])
def test_two_runs_and_a_replayed_graph_give_the_same_bytes(rows):
    first, again, replayed = device_calls(rows), device_calls(rows), device_calls(rows, captured=True)
    for call in range(2):
        for k, v in first[call].items():
            assert v.tobytes() == again[call][k].tobytes() and v.tobytes() == replayed[call][k].tobytes(), (call, k)


def test_refusals_launch_nothing():
    import ctypes
    import torch
    from paac_amd import _lib, hip_ops
    dev = torch.device("cuda")
    block = hip_ops.rnd_block(dev, SEED, 16)
    states = torch.zeros((17, 84 * 84 * 4), dtype=torch.uint8, device=dev)
    rewards, bonus = torch.zeros(16, device=dev), torch.zeros(16, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def raw(message, st=states, rows=16, beta=0.1, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, rw=rewards):
        rc = _lib.load().paac_rnd_bonus(vp(st), rows, vp(block.target), vp(block.predictor), vp(block.adam_m), vp(block.adam_v),
                                        vp(block.norm), vp(block.scratch), beta, lr, b1, b2, eps, vp(rw), vp(bonus), vp(block.raw),
                                        None, hip_ops._stream())
        assert rc < 0 and message in _lib.load().paac_last_error().decode(), (message, _lib.load().paac_last_error())

    raw("null argument", rw=None)
    raw("rows=0", rows=0)
    raw("negative or not finite", beta=-1.0)
    raw("negative or not finite", beta=float("nan"))
    raw("lr", lr=0.0)
    raw("lr", lr=float("inf"))
    raw("outside [0, 1)", b1=1.0)
    raw("outside [0, 1)", b2=-0.1)
    raw("eps", eps=0.0)
    raw("16-byte aligned", st=states.view(-1)[8:])
    assert not bonus.any().item() and not block.norm.any().item() and not block.adam_v.any().item()


def loop_run(use_graph, beta, cycles=3):
    """`cycles` cycles of the device loop on catch, 8 environments -> (predictor, bonus plane, rewards, ep_reward, finished ring,
    per eager cycle (next stacks, rewards, bonus))."""
    from paac_amd.paac import DeviceRollout
    from test_window_stats_gpu import catch_args, seeded_learner
    L, env_creator = seeded_learner(catch_args(["--explore_bonus", beta, "--explore_kind", "rnd"], emulator_counts=8))
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=use_graph)
    assert ro.explore is None and (ro.rnd is not None) == (float(beta) > 0)
    host, seen = lambda t: t.cpu().numpy().copy(), []
    if use_graph:
        ro.run_cycles(cycles)
        ro.synchronize()
    for _ in range(0 if use_graph else cycles):
        ro.run_cycle()
        ro.synchronize()
        first = (ro.parity ^ 1) * ro.T + 1          # the cycle that has just run: the ring slots its steps arrived in
        seen.append((host(ro.states[first:first + ro.T]), host(ro.rewards), host(ro.bonus) if ro.rnd is not None else None))
    on = ro.rnd is not None
    out = (host(ro.rnd.predictor) if on else None, host(ro.bonus) if on else None, host(ro.rewards), host(ro.ep_reward),
           host(ro.finished), seen)
    ro.close()
    L.ctx.close()
    return out


def test_device_loop_eager_captured_and_twin_agree():
    eager, captured, off = loop_run(False, "0.1"), loop_run(True, "0.1"), loop_run(False, "0", cycles=1)
    for a, b in zip(eager[:3], captured[:3]):
        assert a.tobytes() == b.tobytes()
    assert off[0] is None and off[1] is None          # BETA = 0: the rollout holds no block
    stacks = [s for s, _, _ in eager[5]]
    none = np.zeros(stacks[0].shape[0] * stacks[0].shape[1], dtype=np.float32)
    want = twin_calls(rnd.Twin(SEED), stacks, 0.1, 1e-4, rnd.EPS, none)
    bars = bars_of(want, twin_calls(rnd.Twin(SEED, np.float32), stacks, 0.1, 1e-4, rnd.EPS, none))
    for c, (_, rewards, bonus) in enumerate(eager[5]):
        assert np.abs(bonus.reshape(-1) - want[c]["bonus"]).max() <= bars[c]["bonus"], c
        extrinsic = np.rint(rewards - bonus)          # the game's reward is -1, 0 or 1
        assert np.isin(extrinsic, (-1.0, 0.0, 1.0)).all() and np.array_equal(rewards, extrinsic.astype(np.float32) + bonus), c
        if c == 0:          # the same weights and sampler stream as the run without the bonus: the same actions, the same game
            assert np.array_equal(extrinsic, off[5][0][1])
    for name, at in PARTS.items():
        assert np.abs(eager[0][at] - want[-1][name]).max() <= bars[-1][name], name


def test_scores_stay_extrinsic_and_a_run_writes_the_record():
    """Scores: ep_reward and the finished-episode ring after one cycle, bonus on against off (the same weights and sampler
    stream: the same game).  Record: paac_amd.train's loop on catch, 128 environments: one log window of 16 cycles."""
    from test_window_stats_gpu import T, catch_args, seeded_learner
    on, off = loop_run(False, "0.1", cycles=1), loop_run(False, "0", cycles=1)
    assert on[3].tobytes() == off[3].tobytes() and on[4].tobytes() == off[4].tobytes()
    args = catch_args(["--explore_bonus", "0.1", "--explore_kind", "rnd"], emulator_counts=128, max_global_steps=16 * 128 * T)
    learner, _ = seeded_learner(args)
    np.random.seed(9)
    learner.train()
    records = [json.loads(line) for line in open(os.path.join(args.debugging_folder, "metrics.jsonl"))]
    explore = [r for r in records if r["kind"] == "explore"]
    assert len(explore) == 1 and set(explore[0]) == {"kind", "time", "global_step", "explore_kind", "beta", "lr", "bonus_mean",
                                                      "bonus_max", "error_mean", "error_rms_running"}
    assert explore[0]["explore_kind"] == "rnd" and explore[0]["lr"] == 1e-4 and 0 < explore[0]["bonus_mean"] <= explore[0]["bonus_max"]
    assert explore[0]["error_mean"] > 0 and explore[0]["error_rms_running"] > 0
