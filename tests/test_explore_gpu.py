"""-m gpu: --explore_bonus (spec and twin: paac_amd/explore.py; contract: include/paac_hip.h, paac_explore_bonus).  Everything
is an integer or a correctly rounded float32 operation: every comparison is bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from paac_amd import explore

SEED = 3          # (the random_seed train.get_network_and_environment_creator gives a run)


@pytest.mark.parametrize("rows,bits,table_bits", [(1, 1, 4), (16, 17, 4), (17, 64, 20), (160, 32, 20), (2688, 32, 20)])
def test_entry_equals_the_twin_over_two_calls(rows, bits, table_bits):
    import torch
    from paac_amd import hip_ops
    dev = torch.device("cuda")
    rs = np.random.RandomState(rows)
    x = rs.randint(0, 256, (rows, explore.K)).astype(np.uint8)
    # planted, as many as fit: P = 0 everywhere (every bit set), the two extremes of |P|, one row three times (n = 3 in one call)
    planted = [np.full(explore.K, v, dtype=np.uint8) for v in (128, 0, 255)] + 3 * [rs.randint(0, 256, explore.K).astype(np.uint8)]
    for i, row in enumerate(planted[:rows]):
        x[i] = row
    want_rewards = rs.randn(rows).astype(np.float32)
    twin = explore.Twin(SEED, bits, table_bits)
    block = hip_ops.explore_block(dev, SEED, bits, table_bits, rows)
    states, rewards = torch.from_numpy(x).to(dev), torch.from_numpy(want_rewards).to(dev)
    bonus, codes = torch.zeros(rows, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev)
    for call in range(2):          # the second call: the counts persist (n doubles) and the scratch was left clean
        want_codes, want_bonus = twin.bonus(x, 0.25, want_rewards)
        hip_ops.explore_bonus(block, states, 0.25, rewards, bonus, codes)
        assert np.array_equal(codes.cpu().numpy().view(np.uint64), want_codes), call
        assert np.array_equal(block.counts.cpu().numpy(), twin.counts), call
        assert np.array_equal(bonus.cpu().numpy().view(np.uint32), want_bonus.view(np.uint32)), call
        assert np.array_equal(rewards.cpu().numpy().view(np.uint32), want_rewards.view(np.uint32)), call
        assert not block.scratch.any().item(), call
    assert int(want_codes[0]) == (1 << bits) - 1 and twin.counts.sum() == 2 * rows
    if rows >= 6:
        assert want_codes[3] == want_codes[4] == want_codes[5] and (table_bits < 20 or want_bonus[3] == np.float32(0.25) / np.sqrt(np.float32(6)))


def test_refusals_launch_nothing():
    import ctypes
    import torch
    from paac_amd import _lib, hip_ops
    dev = torch.device("cuda")
    block = hip_ops.explore_block(dev, SEED, 32, 4, 16)
    states = torch.zeros((17, explore.K), dtype=torch.uint8, device=dev)
    rewards, bonus = torch.zeros(16, device=dev), torch.zeros(16, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)

    def raw(message, st=states, rows=16, bits=32, table_bits=4, beta=0.1, rw=rewards):
        rc = _lib.load().paac_explore_bonus(vp(st), rows, bits, table_bits, vp(block.signs), vp(block.counts), vp(block.scratch),
                                            beta, vp(rw), vp(bonus), None, hip_ops._stream())
        assert rc < 0 and message in _lib.load().paac_last_error().decode(), (message, _lib.load().paac_last_error())

    raw("null argument", rw=None)
    raw("rows=0", rows=0)
    raw("bits=0", bits=0)
    raw("bits=65", bits=65)
    raw("table_bits=3", table_bits=3)
    raw("table_bits=27", table_bits=27)
    raw("negative or not finite", beta=-1.0)
    raw("negative or not finite", beta=float("inf"))
    raw("negative or not finite", beta=float("nan"))
    raw("16-byte aligned", st=states.view(-1)[8:])
    assert not block.counts.any().item() and not bonus.any().item()


def loop_run(use_graph, beta, cycles=3):
    """`cycles` cycles of the device loop on catch -> (learner state, table, bonus plane, per eager cycle (next stacks, rewards, bonus))."""
    from paac_amd.paac import DeviceRollout
    from test_window_stats_gpu import catch_args, seeded_learner
    L, env_creator = seeded_learner(catch_args(["--explore_bonus", beta], emulator_counts=8))
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=use_graph)
    host, seen = lambda t: t.cpu().numpy().copy(), []
    if use_graph:
        ro.run_cycles(cycles)
        ro.synchronize()
    for _ in range(0 if use_graph else cycles):
        ro.run_cycle()
        ro.synchronize()
        first = (ro.parity ^ 1) * ro.T + 1          # the cycle that has just run: the ring slots its steps arrived in
        seen.append((host(ro.states[first:first + ro.T]), host(ro.rewards), host(ro.bonus) if ro.explore is not None else None))
    out = ([host(t) for _, t in L.update_state], host(ro.explore.counts) if ro.explore is not None else None,
           host(ro.bonus) if ro.explore is not None else None, seen)
    ro.close()
    L.ctx.close()
    return out


def test_device_loop_eager_captured_and_twin_agree():
    eager, captured, off = loop_run(False, "0.1"), loop_run(True, "0.1"), loop_run(False, "0", cycles=1)
    for a, b in zip(eager[0] + [eager[1], eager[2]], captured[0] + [captured[1], captured[2]]):
        assert np.array_equal(a, b)
    assert off[1] is None and off[2] is None          # flag off: the rollout holds no block
    twin = explore.Twin(SEED, 32, 20)
    for c, (stacks, rewards, bonus) in enumerate(eager[3]):
        _, want = twin.bonus(stacks, 0.1)
        assert np.array_equal(bonus.reshape(-1).view(np.uint32), want.view(np.uint32)), c
        extrinsic = np.rint(rewards - bonus)          # the game's reward is -1, 0 or 1 and the bonus at most 0.1
        assert np.isin(extrinsic, (-1.0, 0.0, 1.0)).all() and np.array_equal(rewards, extrinsic.astype(np.float32) + bonus), c
        if c == 0:          # the same weights and sampler stream as the run without the flag: the same actions, the same game
            assert np.array_equal(extrinsic, off[3][0][1])
    assert np.array_equal(eager[1], twin.counts) and twin.counts.sum() == 3 * 5 * 8
