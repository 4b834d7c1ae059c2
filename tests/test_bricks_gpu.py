"""-m gpu: the bricks game on the device (paac_bricks_reset / paac_bricks_step, DeviceRollout with a kind == "bricks" spec)
against its host twin paac_amd/bricks.py."""
import functools
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import bricks
from paac_amd.bricks import FULL_ROW as F, BricksEnvironment

ONE_HOT = np.eye(3)
ACTION_CYCLE = (0, 1, 2, 2, 1)
EVENT_KINDS = ("wall", "left_hit", "right_hit", "miss", "lives_out", "brick", "ceiling", "step_cap")
SHAPES = [(3, 5, 520), (33, 0, 120)]          # (N, env_offset, steps) of the kernel-against-twin runs


def step_twins(twins, actions):
    """runners.step_emulators for a list of twins -> (observations, rewards, masks)."""
    obs, rewards, overs = [], [], []
    for env, a in zip(twins, actions):
        o, r, t = env.next(ONE_HOT[int(a)])
        if t:
            o = env.get_initial_state()
        obs.append(o)
        rewards.append(r)
        overs.append(t)
    return np.stack(obs), np.asarray(rewards, dtype=np.float32), 1.0 - np.asarray(overs, dtype=np.float32)


def drained(fin):
    """The device ring of finished episodes -> (count, sorted [(reward, length)])."""
    host = fin.cpu().numpy()
    count = int(host[0])
    assert count <= 4096
    return count, sorted(zip(host[2:2 + 4096].view(np.float32)[:count].tolist(), host[2 + 4096:2 + 4096 + count].tolist()))


def events_of(state, a):
    """The rule branches the step of `state` under action a takes (the spec's order of tests, restated for counting only)."""
    bx, by, dx, dy, px, lives, steps = state[:7]
    px = max(px - 1, 0) if a == 1 else (min(px + 1, 12) if a == 2 else px)
    found = []
    nx = bx + dx
    if nx < 0 or nx > 13:
        found.append("wall")
        nx = bx
    ny = by + dy
    if ny < 0:
        found.append("ceiling")
    elif 2 <= ny <= 4 and (state[8 + ny - 2] >> nx) & 1:
        found.append("brick")
    elif ny == 13:
        if nx in (px, px + 1):
            found.append("left_hit" if nx == px else "right_hit")
        else:
            found.append("miss")
            if lives == 1:
                found.append("lives_out")
    if steps == bricks.MAX_STEPS - 1:
        found.append("step_cap")
    return found


@functools.lru_cache(maxsize=None)
def scripted_run(N, env_offset, steps, seed=3):
    """The actions of a kernel-against-twin run -- environment e plays track_action when e % 3 == 0, else ACTION_CYCLE -- and the
    count of every rule branch they lead the twins through -> (int32 [steps, N], {kind: count}).  States only: no rendering."""
    states = [bricks.start_state(seed, env_offset + e, 0) for e in range(N)]
    actions, seen = np.zeros((steps, N), dtype=np.int32), dict.fromkeys(EVENT_KINDS, 0)
    for step in range(steps):
        for e in range(N):
            a = bricks.track_action(states[e]) if e % 3 == 0 else ACTION_CYCLE[(step + e) % 5]
            actions[step, e] = a
            for kind in events_of(states[e], a):
                seen[kind] += 1
            states[e] = bricks.step_state(seed, env_offset + e, states[e], a)[0]
    return actions, seen


class Buffers(object):
    """What one paac_bricks_step launch of N environments reads and writes."""

    def __init__(self, N, dev="cuda"):
        from paac_amd import hip_ops
        W = hip_ops.BRICKS_STATE_WORDS
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, W), dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.state2 = torch.zeros((N, W), dtype=torch.int32, device=dev)
        self.actions = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r = (torch.zeros(N, device=dev) for _ in range(3))
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)

    def step(self, seed, env_offset, a, second=False, single_life=False):
        from paac_amd import hip_ops
        self.actions.copy_(torch.from_numpy(np.asarray(a, dtype=np.int32)))
        hip_ops.bricks_step(seed, env_offset, self.actions, self.states[0], self.states[1], self.stacks[0], self.stacks[1],
                            self.rew, self.msk, self.ep_r, self.ep_l, self.fin, stack_out2=self.stack2 if second else None,
                            state_out2=self.state2 if second else None, single_life=single_life)


@pytest.mark.parametrize("N,env_offset,steps", SHAPES)
def test_kernel_matches_twin_bit_for_bit(N, env_offset, steps):
    from paac_amd import hip_ops
    seed = 3
    b = Buffers(N)
    twins = [BricksEnvironment(env_offset + e, seed=seed) for e in range(N)]
    want_obs = np.stack([env.get_initial_state() for env in twins])
    hip_ops.bricks_reset(seed, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.stacks[0].cpu().numpy(), want_obs)
    assert np.array_equal(b.states[0].cpu().numpy(), np.stack([env.state_words() for env in twins]))
    want_ep_r, want_ep_l, want_fin = np.zeros(N, np.float32), np.zeros(N, np.int32), []
    script, seen = scripted_run(N, env_offset, steps)
    for step in range(steps):
        a = script[step]
        assert a[0] == bricks.track_action(twins[0].state)
        second = step == 7
        b.step(seed, env_offset, a, second=second)
        want_obs, want_rew, want_msk = step_twins(twins, a)
        want_ep_r += want_rew
        want_ep_l += 1
        for e in np.nonzero(want_msk == 0.0)[0]:
            want_fin.append((float(want_ep_r[e]), int(want_ep_l[e])))
            want_ep_r[e], want_ep_l[e] = 0.0, 0
        assert np.array_equal(b.stacks[1].cpu().numpy(), want_obs), "step %d: stacks" % step
        assert np.array_equal(b.states[1].cpu().numpy(), np.stack([env.state_words() for env in twins])), "step %d: states" % step
        assert np.array_equal(b.rew.cpu().numpy(), want_rew) and np.array_equal(b.msk.cpu().numpy(), want_msk), "step %d" % step
        assert np.array_equal(b.ep_r.cpu().numpy(), want_ep_r) and np.array_equal(b.ep_l.cpu().numpy(), want_ep_l), "step %d" % step
        assert drained(b.fin) == (len(want_fin), sorted(want_fin)), "step %d: finished ring" % step
        if second:
            assert torch.equal(b.stack2, b.stacks[1]) and torch.equal(b.state2, b.states[1])
        b.stacks.reverse()
        b.states.reverse()
    print("N = %d, %d steps: %s; %d episodes" % (N, steps, seen, len(want_fin)))
    assert seen["brick"] == int(sum(r for r, _ in want_fin) + want_ep_r.sum())
    assert len(want_fin) >= N and min(l for _, l in want_fin) >= 24
    if steps > bricks.MAX_STEPS:
        # the tracking environment never loses a life: its first episode ends at the step cap
        assert seen["step_cap"] >= 1 and max(l for _, l in want_fin) == bricks.MAX_STEPS


def test_the_two_shapes_reach_every_event_kind():
    """From the twins' side: every rule branch a run can reach occurred in the two runs above (a later change of their inputs
    cannot quietly stop covering one)."""
    counts = [scripted_run(*shape)[1] for shape in SHAPES]
    print(counts)
    for kind in EVENT_KINDS:
        assert sum(seen[kind] for seen in counts) >= 1, kind


def S(bx, by, dx, dy, px, lives=3, steps=10, k=0, rows=(F, F, F)):
    return (bx, by, dx, dy, px, lives, steps, k) + tuple(rows)


# valid hand-written records: the branches no short run reaches first, then one or two of every other branch
CRAFTED = [
    S(5, 5, 1, -1, 6, rows=(0, 0, 1 << 6)),               # the last brick goes: the field stays empty ...
    S(5, 12, 1, 1, 6, rows=(0, 0, 0)),                    # ... until the paddle is hit: refill (a = 2: a miss, no refill)
    S(7, 12, -1, 1, 5, rows=(0, 0, 0), k=3),              # refill on the right half
    S(5, 12, 1, 1, 6, rows=(0, 1 << 13, 0)),              # one brick left: a hit refills nothing
    S(5, 5, 1, -1, 9, steps=499),                         # a reward on the capping step
    S(5, 8, 1, 1, 9, steps=499, k=7),                     # the cap alone
    S(5, 12, 1, 1, 6, steps=499),                         # the cap with a paddle hit / with a miss
    S(5, 8, 1, 1, 9, steps=498),                          # one step short of the cap
    S(5, 12, 1, 1, 9),                                    # a miss: serve 1 (single_life: terminal)
    S(5, 12, 1, 1, 9, lives=2, rows=(5, 6, 7)),           # serve 2
    S(5, 12, 1, 1, 9, lives=1, k=4),                      # lives out
    S(5, 12, 1, 1, 7),                                    # a = 1 turns the miss into a left-half hit
    S(5, 12, 1, 1, 4),                                    # a = 2 turns the miss into a right-half hit
    S(13, 12, 1, 1, 12),                                  # wall in row 12, paddle at its right end
    S(0, 12, -1, 1, 0),                                   # ... and at its left end
    S(0, 8, -1, 1, 0), S(13, 8, 1, -1, 12),               # walls; the paddle clamps
    S(5, 0, 1, -1, 5, rows=(0, 0, 0)), S(13, 0, 1, -1, 5, rows=(0, 0, 0)),      # ceiling; ceiling and wall
    S(0, 5, -1, -1, 9), S(2, 1, 1, 1, 9), S(6, 4, 1, -1, 9, rows=(F, F, F & ~(1 << 6))),      # bricks: wall, from above, inside
    S(6, 4, 1, -1, 9, rows=(0, 0, 0)), S(6, 3, -1, 1, 9, rows=(F, F & ~(1 << 6), F & ~(3 << 5))),      # cleared cells
]


@pytest.mark.parametrize("single_life", [False, True])
def test_crafted_records_step_like_the_twin(single_life):
    from paac_amd import hip_ops
    seed, env_offset, N = 3, 2, len(CRAFTED)
    b = Buffers(N)
    records = np.array([list(s) + [0] for s in CRAFTED], dtype=np.int32)
    history = np.random.RandomState(4).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    outcomes = set()
    for a in range(3):
        b.states[0].copy_(torch.from_numpy(records))
        b.stacks[0].copy_(torch.from_numpy(history))
        b.ep_r.fill_(2.0)
        b.ep_l.fill_(40)
        b.fin.zero_()
        b.step(seed, env_offset, [a] * N, single_life=single_life)
        got_states, got_stacks = b.states[1].cpu().numpy(), b.stacks[1].cpu().numpy()
        got_rew, got_msk = b.rew.cpu().numpy(), b.msk.cpu().numpy()
        want_fin = []
        for e, s in enumerate(CRAFTED):
            state, r, t = bricks.step_state(seed, env_offset + e, s, a, single_life)
            assert tuple(got_states[e]) == state + (0,), (e, a, s)
            assert (got_rew[e], got_msk[e]) == (r, 0.0 if t else 1.0), (e, a, s)
            want = np.zeros((84, 84, 4), dtype=np.uint8)
            if not t:
                want[..., :3] = history[e][..., 1:]
            want[..., 3] = bricks.plane(state)
            assert np.array_equal(got_stacks[e], want), (e, a, s)
            if t:
                want_fin.append((2.0 + r, 41))
            outcomes.add((e, a, r, t, state[8:] == (F, F, F) and s[8:] != (F, F, F) and not t))
        assert drained(b.fin) == (len(want_fin), sorted(want_fin))
        assert np.array_equal(b.ep_r.cpu().numpy() == 0.0, got_msk == 0.0) and np.array_equal(b.ep_l.cpu().numpy() == 0, got_msk == 0.0)
    # the branches this test is for did occur
    assert (1, 0, 0.0, False, True) in outcomes and (2, 0, 0.0, False, True) in outcomes          # refills
    assert (1, 2, 0.0, single_life, False) in outcomes and (3, 0, 0.0, False, False) in outcomes  # ... and none
    assert (4, 0, 1.0, True, False) in outcomes and (5, 1, 0.0, True, False) in outcomes          # the cap, with and without reward
    assert (8, 0, 0.0, single_life, False) in outcomes and (10, 0, 0.0, True, False) in outcomes  # a miss; lives out


def test_last_brick_then_paddle_hit_refills_the_field():
    """A field with one brick left, played on by the tracking policy: the strike, the empty field, the paddle hit, 42 bricks."""
    seed, env_offset = 3, 9
    b = Buffers(1)
    twin = BricksEnvironment(env_offset, seed=seed)
    twin.state = S(5, 5, 1, -1, 5, steps=0, rows=(0, 0, 1 << 6))
    b.states[0].copy_(torch.from_numpy(twin.state_words()[None]))
    b.stacks[0].copy_(torch.from_numpy(twin.get_initial_state()[None]))
    fields = []
    for step in range(12):
        a = [bricks.track_action(twin.state)]
        b.step(seed, env_offset, a)
        want_obs, want_rew, want_msk = step_twins([twin], a)
        assert np.array_equal(b.states[1].cpu().numpy()[0], twin.state_words()) and np.array_equal(b.stacks[1].cpu().numpy(), want_obs)
        assert np.array_equal(b.rew.cpu().numpy(), want_rew) and np.array_equal(b.msk.cpu().numpy(), want_msk)
        fields.append(twin.state[8:])
        b.stacks.reverse()
        b.states.reverse()
    assert fields[0] == (0, 0, 0) and fields[-1] != (0, 0, 0) and (F, F, F) in fields and twin.state[5] == 3


def test_step_in_place_and_bad_shapes_are_refused():
    from paac_amd import _lib, hip_ops
    N, W = 2, hip_ops.BRICKS_STATE_WORDS
    assert W == bricks.STATE_WORDS == 12
    stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    stack_b = torch.zeros_like(stack)
    state = torch.zeros((N, W), dtype=torch.int32, device="cuda")
    state_b = torch.zeros_like(state)
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    f, i = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    hip_ops.bricks_reset(1, 0, state, stack)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.bricks_step(1, 0, actions, state, state, stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.bricks_step(1, 0, actions, state, state_b, stack, stack, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.bricks_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, state_out2=state)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.bricks_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, stack_out2=stack)
    with pytest.raises(ValueError):
        hip_ops.bricks_step(1, 0, actions, state, state_b[:, :8].contiguous(), stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.bricks_step(1, 0, actions, state, state_b, stack, stack_b[:1], f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.bricks_reset(1, 0, state_b[:1], stack)
    with pytest.raises(ValueError):          # a catch record is no bricks record
        hip_ops.bricks_reset(1, 0, torch.zeros((N, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"), stack)
    torch.cuda.synchronize()


def make_args(**kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "bricks"])
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_test_")
    args.emulator_workers = 0
    args.max_global_steps = 1 << 40
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def build_learner(args, params_seed=0):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(params_seed))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


@pytest.mark.parametrize("sampler,single_life", [("numpy", False), ("philox", False), ("philox", True)])
def test_device_loop_eager_captured_and_batched_agree_and_replay_through_the_twins(sampler, single_life):
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 7          # odd T: the ring's wrap-around slot is exercised
    outs, records = [], []
    for mode in ("eager", "captured", "batched"):
        learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler=sampler,
                                          single_life_episodes=single_life))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        spec = learner.environment_creator.device_env_spec
        assert spec == dict(kind="bricks", seed=3, single_life=single_life)
        ro = DeviceRollout(learner, spec, sampler=sampler, use_graph=mode != "eager")
        assert not ro.catch and ro.stateful and tuple(ro.env_state.shape) == (2 * T + 1, N, 12)
        if mode == "batched":
            ro.run_cycles(cycles)           # 4 cycles in one graph launch, then 3 single ones
        else:
            for _ in range(cycles):
                ro.run_cycle()
                if mode == "eager":
                    ro.synchronize()
                    records.append((ro.actions.cpu().numpy().copy(), ro.rewards.cpu().numpy().copy(),
                                    ro.masks.cpu().numpy().copy(), ro.rollout_states().cpu().numpy().copy()))
        ro.synchronize()
        outs.append(dict(params=learner.network.get_parameters(), stacks=ro.states.cpu().numpy().copy(),
                         states=ro.env_state.cpu().numpy().copy(), actions=ro.actions.cpu().numpy().copy(),
                         rewards=ro.rewards.cpu().numpy().copy(), masks=ro.masks.cpu().numpy().copy(),
                         step=int(ro.global_step_dev.item()), finished=ro.finished_episodes()))
        ro.close()
    for other in outs[1:]:
        assert other["step"] == outs[0]["step"] == cycles * N * T
        for k in ("stacks", "states", "actions", "rewards", "masks"):
            assert np.array_equal(outs[0][k], other[k]), k
        for k, v in outs[0]["params"].items():
            assert np.array_equal(v, other["params"][k]), k
        assert outs[0]["finished"][0] == other["finished"][0] and sorted(outs[0]["finished"][1]) == sorted(other["finished"][1])
    # the whole run through the host twins on the recorded actions: every observation trained on, every reward and mask
    twins = [BricksEnvironment(e, seed=3, single_life=single_life) for e in range(N)]
    obs = np.stack([env.get_initial_state() for env in twins])
    episodes, totals, lengths = [], np.zeros(N), np.zeros(N, dtype=np.int64)
    for c, (actions, rewards, masks, trained_on) in enumerate(records):
        assert actions.min() >= 0 and actions.max() <= 2
        for t in range(T):
            assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "cycle %d step %d" % (c, t)
            obs, want_rew, want_msk = step_twins(twins, actions[t])
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], want_msk), "cycle %d step %d" % (c, t)
            totals += want_rew
            lengths += 1
            for e in np.nonzero(want_msk == 0.0)[0]:
                episodes.append((float(totals[e]), int(lengths[e])))
                totals[e], lengths[e] = 0.0, 0
    assert np.array_equal(outs[0]["rewards"], records[-1][1]) and np.array_equal(outs[0]["actions"], records[-1][0])
    # the slot the next cycle starts from holds the twins' present: observations and state records
    last = (cycles & 1) * T
    assert np.array_equal(outs[0]["stacks"][last], obs)
    assert np.array_equal(outs[0]["states"][last], np.stack([env.state_words() for env in twins]))
    print("%s, single_life %s: %d episodes in %d steps: %s" % (sampler, single_life, len(episodes), cycles * T, episodes))
    assert outs[0]["finished"][0] == len(episodes) and sorted(outs[0]["finished"][1]) == sorted(episodes)
    # 35 steps: an episode lasts 24 steps at the least, 8 with single lives (a serve falls for 8 steps)
    assert len(episodes) >= 1 and all(l >= (8 if single_life else 24) for _, l in episodes)


LEARN_STEPS = 2 * 696320      # twice the smallest step count at which the default flags cleared the bar (DESIGN.md has the curve)


def test_it_learns():
    """The device loop with the default flags (NIPS trunk, RMSProp, lr 0.0224, 32 environments, t_max 5), weights seeded, philox
    sampler, environment seed 3: the mean return of the last 1000 finished episodes must exceed 1.0.  Over 64,000 episodes the
    uniform random policy scores 0.253 (std 0.530: a 1000-episode mean has a standard error of 0.017, the bar is four times the
    score and 44 standard errors above it) and always-stay 0.289 (std 0.982, standard error 0.031: 23 standard errors).
    Measured on the MI355X: first above the bar at 696,320 steps (checked every 20,480); the test trains twice as long, where
    the mean was 22.0."""
    from paac_amd.paac import DeviceRollout
    N, T = 32, 5
    learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, arch="NIPS"))
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=True)
    ro.run_cycles(LEARN_STEPS // (N * T))
    ro.synchronize()
    count, episodes = ro.finished_episodes()
    assert int(ro.global_step_dev.item()) == LEARN_STEPS and count > 4096 and len(episodes) == 4096
    mean = float(np.mean([r for r, _ in episodes[-1000:]]))
    print("bricks after %d steps: mean return of the last 1000 of %d episodes %+.3f" % (LEARN_STEPS, count, mean))
    ro.close()
    assert mean > 1.0


def test_host_plugin_loop_matches_device_loop():
    """The host loop stepping BricksEnvironment plugins == the device loop on the same np.random sampler stream."""
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 3
    feeds = []
    host = build_learner(make_args(emulator_counts=N, max_local_steps=T, max_global_steps=cycles * N * T, sampler="numpy",
                                   host_environments=True, record_feeds=True, feed_callback=feeds.append))
    np.random.seed(7)
    host.train()
    assert len(feeds) == cycles
    devl = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler="numpy"))
    np.random.seed(7)
    devl.global_step = devl.init_network()
    ro = DeviceRollout(devl, devl.environment_creator.device_env_spec, sampler="numpy", use_graph=True)
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        assert np.array_equal(ro.rollout_states().cpu().numpy(), feeds[c]["states"]), "cycle %d" % c
        assert np.array_equal(ro.actions.view(-1).cpu().numpy(), feeds[c]["actions"]), "cycle %d" % c
        assert np.array_equal(ro.rewards.cpu().numpy(), feeds[c]["rewards"]), "cycle %d" % c
        assert np.array_equal(ro.masks.cpu().numpy(), feeds[c]["masks"]), "cycle %d" % c
        assert np.allclose(ro.y.cpu().numpy(), feeds[c]["y"], atol=1e-5)
    gh, gd = host.network.get_parameters(), devl.network.get_parameters()
    for k in gh:
        assert np.abs(gh[k] - gd[k]).max() < 1e-5, k
    ro.close()
