"""-m gpu: the rally game on the device (paac_rally_reset / paac_rally_step, DeviceRollout with a kind == "rally" spec,
paac_eval_step with game "rally") against its host twin paac_amd/rally.py."""
import functools
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import evaluation, rally
from paac_amd.rally import RallyEnvironment

ONE_HOT = np.eye(6)
ACTION_CYCLE = (0, 2, 4, 1, 3, 5, 3)          # all six actions; a net drift of one cell to the left per round
EVENT_KINDS = ("wall", "agent_left", "agent_right", "opponent_left", "opponent_right", "agent_miss", "opponent_miss",
               "opponent_moves_left", "opponent_moves_right", "lazy_stay", "agent_wins", "opponent_wins", "step_cap")
SHAPES = [(5, 7, 160), (3, 0, 1010)]          # (N, env_offset, steps) of the kernel-against-twin runs
SEED = 3


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


def events_of(seed, env, state, a):
    """The rule branches the step of `state` under action a takes (the spec's order of tests, restated for counting only)."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = state
    px = min(px + 1, 12) if a in (2, 4) else (max(px - 1, 0) if a in (3, 5) else px)
    found = []
    if dy < 0 and by <= rally.REACT_ROW:
        if rally.opponent_moves(seed, env, state):
            tx = rally.entry_column(bx, dx, by)[0]
            if tx < ox:
                found.append("opponent_moves_left")
                ox -= 1
            elif tx > ox + 1:
                found.append("opponent_moves_right")
                ox += 1
        else:
            found.append("lazy_stay")
    nx = bx + dx
    if nx < 0 or nx > 13:
        found.append("wall")
        nx = bx
    ny = by + dy
    if ny == 13:
        if nx in (px, px + 1):
            found.append("agent_left" if nx == px else "agent_right")
        else:
            found.append("agent_miss")
            if theirs == rally.POINTS - 1:
                found.append("opponent_wins")
    elif ny == 0:
        if nx in (ox, ox + 1):
            found.append("opponent_left" if nx == ox else "opponent_right")
        else:
            found.append("opponent_miss")
            if mine == rally.POINTS - 1:
                found.append("agent_wins")
    if steps == rally.MAX_STEPS - 1:
        found.append("step_cap")
    return found


def scripted_action(state, e, step):
    """Environment e plays return_action when e % 3 == 0, aim_action when e % 3 == 1, else ACTION_CYCLE."""
    if e % 3 == 0:
        return rally.return_action(state)
    if e % 3 == 1:
        return rally.aim_action(state)
    return ACTION_CYCLE[(step + e) % len(ACTION_CYCLE)]


@functools.lru_cache(maxsize=None)
def scripted_run(N, env_offset, steps, seed=SEED):
    """The actions of a kernel-against-twin run and the count of every rule branch they lead the twins through ->
    (int32 [steps, N], {kind: count}).  States only: no rendering."""
    states = [rally.start_state(seed, env_offset + e, 0) for e in range(N)]
    actions, seen = np.zeros((steps, N), dtype=np.int32), dict.fromkeys(EVENT_KINDS, 0)
    for step in range(steps):
        for e in range(N):
            a = scripted_action(states[e], e, step)
            actions[step, e] = a
            for kind in events_of(seed, env_offset + e, states[e], a):
                seen[kind] += 1
            states[e] = rally.step_state(seed, env_offset + e, states[e], a)[0]
    return actions, seen


class Buffers(object):
    """What one paac_rally_step launch of N environments reads and writes."""

    def __init__(self, N, dev="cuda"):
        from paac_amd import hip_ops
        W = hip_ops.RALLY_STATE_WORDS
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, W), dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.state2 = torch.zeros((N, W), dtype=torch.int32, device=dev)
        self.actions = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r = (torch.zeros(N, device=dev) for _ in range(3))
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)

    def step(self, seed, env_offset, a, second=False):
        from paac_amd import hip_ops
        self.actions.copy_(torch.from_numpy(np.asarray(a, dtype=np.int32)))
        hip_ops.rally_step(seed, env_offset, self.actions, self.states[0], self.states[1], self.stacks[0], self.stacks[1],
                           self.rew, self.msk, self.ep_r, self.ep_l, self.fin, stack_out2=self.stack2 if second else None,
                           state_out2=self.state2 if second else None)


@pytest.mark.parametrize("N,env_offset,steps", SHAPES)
def test_kernel_matches_twin_bit_for_bit(N, env_offset, steps):
    from paac_amd import hip_ops
    b = Buffers(N)
    twins = [RallyEnvironment(env_offset + e, seed=SEED) for e in range(N)]
    want_obs = np.stack([env.get_initial_state() for env in twins])
    hip_ops.rally_reset(SEED, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.stacks[0].cpu().numpy(), want_obs)
    assert np.array_equal(b.states[0].cpu().numpy(), np.stack([env.state_words() for env in twins]))
    want_ep_r, want_ep_l, want_fin = np.zeros(N, np.float32), np.zeros(N, np.int32), []
    script, seen = scripted_run(N, env_offset, steps)
    for step in range(steps):
        a = script[step]
        assert a[0] == rally.return_action(twins[0].state) and a[1] == rally.aim_action(twins[1].state)
        second = step == 7
        b.step(SEED, env_offset, a, second=second)
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
    print("N = %d, %d steps: %s; episodes %s" % (N, steps, seen, want_fin))
    assert seen["opponent_miss"] - seen["agent_miss"] == int(sum(r for r, _ in want_fin) + want_ep_r.sum())
    assert len(want_fin) >= 1 and min(l for _, l in want_fin) >= 35
    if steps > rally.MAX_STEPS:
        # the returning environment draws its first episode out to the step cap
        assert seen["step_cap"] >= 1 and max(l for _, l in want_fin) == rally.MAX_STEPS


def test_the_two_shapes_reach_every_event_kind():
    """From the twins' side: every rule branch a run can reach occurred in the two runs above (a later change of their inputs
    cannot quietly stop covering one)."""
    counts = [scripted_run(*shape)[1] for shape in SHAPES]
    print(counts)
    for kind in EVENT_KINDS:
        assert sum(seen[kind] for seen in counts) >= 1, kind
    assert {a for shape in SHAPES for a in scripted_run(*shape)[0].reshape(-1).tolist()} == set(range(6))


def S(bx, by, dx, dy, px, ox, mine=0, theirs=0, steps=10, k=0):
    return (bx, by, dx, dy, px, ox, mine, theirs, steps, k)


# valid hand-written records: the branches a short run reaches rarely or never, then one or two of every other branch
CRAFTED = [
    S(5, 1, 1, -1, 9, 0, mine=4, theirs=3, k=2),          # the agent's fifth point
    S(5, 12, 1, 1, 7, 3, mine=2, theirs=4, k=5),          # the opponent's fifth point (a = 3 / 5 turn it into a return)
    S(5, 12, 1, 1, 9, 3, mine=4, theirs=4, steps=999),    # the fifth point on the capping step
    S(5, 12, 1, 1, 9, 3, steps=999),                      # a point against on the capping step
    S(5, 1, 1, -1, 9, 0, steps=999, k=7),                 # a point for on the capping step
    S(5, 8, 1, 1, 9, 3, steps=999),                       # the cap alone
    S(5, 12, 1, 1, 6, 3, steps=999),                      # the cap with a return
    S(5, 8, 1, 1, 9, 3, steps=998),                       # one step short of the cap
    S(5, 12, 1, 1, 9, 3, mine=1, theirs=2),               # a point against: serve 4 towards the agent
    S(5, 1, 1, -1, 9, 0, mine=3, theirs=1, steps=9),      # a point for: serve 5 towards the opponent
    S(5, 12, 1, 1, 7, 3),                                 # a = 3 / 5 turn the miss into a left-cell return
    S(5, 12, 1, 1, 4, 3),                                 # a = 2 / 4 turn the miss into a right-cell return
    S(13, 12, 1, 1, 12, 3), S(0, 12, -1, 1, 0, 3),        # a wall in row 12, the paddle at either end (it clamps)
    S(13, 1, 1, -1, 9, 12), S(0, 1, -1, -1, 9, 0),        # ... and in row 1
    S(5, 1, 1, -1, 9, 7), S(5, 1, 1, -1, 9, 4),           # the opponent steps under the ball
    S(5, 1, 1, -1, 9, 7),                                 # ... but not on a lazy step
    S(5, 5, 1, -1, 9, 0), S(5, 5, 1, -1, 9, 12), S(5, 6, 1, -1, 9, 0), S(5, 3, 1, 1, 9, 0),      # REACT_ROW, above it, flying down
    S(1, 3, -1, -1, 9, 2), S(12, 4, 1, -1, 9, 12), S(12, 4, 1, -1, 9, 9),      # the look-ahead bounces off a wall
    S(0, 8, -1, 1, 0, 12), S(13, 8, 1, -1, 12, 0),        # walls in the middle
]
LAZY_RECORDS = (18,)                                       # the opponent's laziness hangs on (environment, episode, steps):
ACTIVE_RECORDS = (16, 17, 19, 20, 23, 24, 25)              # these records get the first steps value from 10 on that has it


def lazy(env, k, steps):
    from paac_amd.synthetic import lowbias32_int, synth_key
    return lowbias32_int(synth_key(SEED, env, k) ^ (0xA11E1000 + steps)) % 4 == 0


for _e in LAZY_RECORDS + ACTIVE_RECORDS:
    _s = CRAFTED[_e]
    CRAFTED[_e] = _s[:8] + (next(t for t in range(10, 990) if lazy(_e, _s[9], t) == (_e in LAZY_RECORDS)),) + _s[9:]


def test_crafted_records_step_like_the_twin():
    seed, env_offset, N = SEED, 0, len(CRAFTED)
    b = Buffers(N)
    records = np.array([list(s) + [0, 0] for s in CRAFTED], dtype=np.int32)
    history = np.random.RandomState(4).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    outcomes = set()
    for a in range(6):
        b.states[0].copy_(torch.from_numpy(records))
        b.stacks[0].copy_(torch.from_numpy(history))
        b.ep_r.fill_(2.0)
        b.ep_l.fill_(40)
        b.fin.zero_()
        b.step(seed, env_offset, [a] * N)
        got_states, got_stacks = b.states[1].cpu().numpy(), b.stacks[1].cpu().numpy()
        got_rew, got_msk = b.rew.cpu().numpy(), b.msk.cpu().numpy()
        want_fin = []
        for e, s in enumerate(CRAFTED):
            state, r, t = rally.step_state(seed, env_offset + e, s, a)
            assert tuple(got_states[e]) == state + (0, 0), (e, a, s)
            assert (got_rew[e], got_msk[e]) == (r, 0.0 if t else 1.0), (e, a, s)
            want = np.zeros((84, 84, 4), dtype=np.uint8)
            if not t:
                want[..., :3] = history[e][..., 1:]
            want[..., 3] = rally.plane(state)
            assert np.array_equal(got_stacks[e], want), (e, a, s)
            if t:
                want_fin.append((2.0 + r, 41))
            outcomes.add((e, a, r, t))
        assert drained(b.fin) == (len(want_fin), sorted(want_fin))
        assert np.array_equal(b.ep_r.cpu().numpy() == 0.0, got_msk == 0.0) and np.array_equal(b.ep_l.cpu().numpy() == 0, got_msk == 0.0)
    # the branches this test is for did occur
    assert (0, 0, 1.0, True) in outcomes and (1, 0, -1.0, True) in outcomes and (1, 3, 0.0, False) in outcomes      # by points
    assert (2, 1, -1.0, True) in outcomes and (3, 0, -1.0, True) in outcomes and (4, 0, 1.0, True) in outcomes      # cap and point
    assert (5, 0, 0.0, True) in outcomes and (6, 0, 0.0, True) in outcomes and (7, 0, 0.0, False) in outcomes       # the cap alone
    assert (8, 0, -1.0, False) in outcomes and (9, 0, 1.0, False) in outcomes                                       # serves
    assert (10, 0, -1.0, False) in outcomes and (10, 5, 0.0, False) in outcomes and (11, 4, 0.0, False) in outcomes
    assert (16, 0, 0.0, False) in outcomes and (18, 0, 1.0, False) in outcomes                                      # active / lazy


def test_step_in_place_and_bad_shapes_are_refused():
    from paac_amd import _lib, hip_ops
    N, W = 2, hip_ops.RALLY_STATE_WORDS
    assert W == rally.STATE_WORDS == 12
    stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    stack_b = torch.zeros_like(stack)
    state = torch.zeros((N, W), dtype=torch.int32, device="cuda")
    state_b = torch.zeros_like(state)
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    f, i = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    hip_ops.rally_reset(1, 0, state, stack)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.rally_step(1, 0, actions, state, state, stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.rally_step(1, 0, actions, state, state_b, stack, stack, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.rally_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, state_out2=state)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.rally_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, stack_out2=stack)
    with pytest.raises(ValueError):
        hip_ops.rally_step(1, 0, actions, state, state_b[:, :8].contiguous(), stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.rally_step(1, 0, actions, state, state_b, stack, stack_b[:1], f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.rally_reset(1, 0, state_b[:1], stack)
    with pytest.raises(ValueError):          # a 4-word catch record is no rally record
        hip_ops.rally_reset(1, 0, torch.zeros((N, 4), dtype=torch.int32, device="cuda"), stack)
    with pytest.raises(ValueError):
        hip_ops.rally_reset(1, 0, torch.zeros((N, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"), stack)
    torch.cuda.synchronize()
    assert not state_b.any() and not stack_b.any()          # nothing was launched


def make_args(**kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "rally"])
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


@pytest.mark.parametrize("sampler", ["numpy", "philox"])
def test_device_loop_eager_captured_and_batched_agree_and_replay_through_the_twins(sampler):
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 7          # odd T: the ring's wrap-around slot is exercised
    outs, records = [], []
    for mode in ("eager", "captured", "batched"):
        learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler=sampler))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        spec = learner.environment_creator.device_env_spec
        assert spec == dict(kind="rally", seed=3) and learner.num_actions == 6
        ro = DeviceRollout(learner, spec, sampler=sampler, use_graph=mode != "eager")
        assert not ro.catch and ro.stateful and tuple(ro.env_state.shape) == (2 * T + 1, N, 12) and ro.A == 6
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
    twins = [RallyEnvironment(e, seed=3) for e in range(N)]
    obs = np.stack([env.get_initial_state() for env in twins])
    episodes, totals, lengths = [], np.zeros(N), np.zeros(N, dtype=np.int64)
    played = set()
    for c, (actions, rewards, masks, trained_on) in enumerate(records):
        assert actions.min() >= 0 and actions.max() <= 5
        played.update(actions.reshape(-1).tolist())
        for t in range(T):
            assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "cycle %d step %d" % (c, t)
            obs, want_rew, want_msk = step_twins(twins, actions[t])
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], want_msk), "cycle %d step %d" % (c, t)
            totals += want_rew
            lengths += 1
            for e in np.nonzero(want_msk == 0.0)[0]:
                episodes.append((float(totals[e]), int(lengths[e])))
                totals[e], lengths[e] = 0.0, 0
    assert len(played) >= 4, played
    assert np.array_equal(outs[0]["rewards"], records[-1][1]) and np.array_equal(outs[0]["actions"], records[-1][0])
    # the slot the next cycle starts from holds the twins' present: observations and state records
    last = (cycles & 1) * T
    assert np.array_equal(outs[0]["stacks"][last], obs)
    assert np.array_equal(outs[0]["states"][last], np.stack([env.state_words() for env in twins]))
    print("%s: actions %s, points so far %s, %d episodes in %d steps: %s" % (sampler, sorted(played), totals, len(episodes),
                                                                            cycles * T, episodes))
    assert outs[0]["finished"][0] == len(episodes) and sorted(outs[0]["finished"][1]) == sorted(episodes)
    # 35 steps: the shortest episode (five serves nobody returns, seven steps each) ends on the last of them at the earliest
    assert all(l >= 35 for _, l in episodes)


LEARN_STEPS = 2 * 737280      # twice the smallest step count at which the default flags cleared the bar (DESIGN.md has the curve)


def test_it_learns():
    """The device loop with the default flags (NIPS trunk, RMSProp, lr 0.0224, 32 environments, t_max 5), weights seeded, philox
    sampler, environment seed 3: the mean return of the last 1000 finished episodes must exceed -3.0.  Over 1024 episodes the
    uniform random policy scores -4.508 (std 1.062: a 1000-episode mean has a standard error of 0.034, the bar is 45 standard
    errors above it) and always-NOOP -3.912 (std 1.670, standard error 0.053: 17 standard errors).  Measured on the MI355X:
    first above the bar at 737,280 steps (checked every 20,480); the test trains twice as long, where the mean was -0.85."""
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
    print("rally after %d steps: mean return of the last 1000 of %d episodes %+.3f" % (LEARN_STEPS, count, mean))
    ro.close()
    assert mean > -3.0


def test_host_plugin_loop_matches_device_loop():
    """The host loop stepping RallyEnvironment plugins == the device loop on the same np.random sampler stream."""
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


EVAL_SEED = (0x5EED << 32) + 11           # the evaluation's seed: a non-zero high word
EVAL_STEPS = 300                          # the hand-given bound: well under the 1000 (+ noops) steps a whole evaluation may take


@pytest.fixture(scope="module")
def acting_network():
    from paac_amd import hip_ops, train
    args = make_args(arch="NIPS")
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    network = network_creator()
    network.initialize(np.random.RandomState(0))
    ctx = hip_ops.Context(network.arch_id, 6, max_batch=8)
    yield network, ctx, env_creator
    ctx.close()


@pytest.mark.parametrize("greedy,noops", [(True, 0), (True, 3), (False, 0), (False, 3)])
def test_eval_step_matches_the_replay_on_the_twins(acting_network, greedy, noops):
    """paac_eval_step with game "rally" behind the acting forward of a seeded network, 8 environments, EVAL_STEPS steps by hand:
    scores and lengths are replay_on_twins' on the recorded actions, and an environment still playing at the bound keeps
    done == 0 on both sides."""
    from paac_amd import hip_ops
    network, ctx, env_creator = acting_network
    N, env_offset, dev = 8, 0, "cuda"
    assert hip_ops.EVAL_GAMES["rally"] == (2, 12)
    stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
    states = [torch.zeros((N, 12), dtype=torch.int32, device=dev) for _ in range(2)]
    probs = torch.zeros((N, 6), dtype=torch.float32, device=dev)
    actions = torch.zeros((EVAL_STEPS, N), dtype=torch.int32, device=dev)
    score = torch.zeros(N, dtype=torch.float32, device=dev)
    length, done = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
    alive = torch.full((1,), N, dtype=torch.int32, device=dev)
    hip_ops.rally_reset(SEED, env_offset, states[0], stacks[0])
    for t in range(EVAL_STEPS):
        a, b = t & 1, (t & 1) ^ 1
        ctx.forward(network.params, stacks[a], probs=probs)
        hip_ops.eval_step("rally", probs, greedy, EVAL_SEED, noops, None, t, SEED, env_offset, states[a], states[b], stacks[a],
                          stacks[b], actions[t], score, length, done, alive)
    trace = actions.cpu().numpy()
    noops_e = evaluation.eval_noops(EVAL_SEED, env_offset + np.arange(N), noops)
    assert trace.min() >= 0 and trace.max() <= 5
    for e in range(N):
        assert not trace[:noops_e[e], e].any()
    # the twins on the recorded actions, one step at a time: records, observations, and the accounts with their done flags
    twins = [env_creator.create_environment(env_offset + e) for e in range(N)]
    for env in twins:
        env.get_initial_state()
    rewards, terminals = np.zeros((EVAL_STEPS, N), dtype=np.float32), np.zeros((EVAL_STEPS, N), dtype=bool)
    for t in range(EVAL_STEPS):
        rewards[t], terminals[t] = evaluation.step_twins(twins, trace[t])
    final = EVAL_STEPS & 1
    assert np.array_equal(states[final].cpu().numpy(), np.stack([env.state_words() for env in twins]))
    assert np.array_equal(stacks[final].cpu().numpy(), np.stack([env.stack for env in twins]))
    want_score, want_length, want_done = evaluation.account(rewards, terminals, noops_e)
    got = (score.cpu().numpy(), length.cpu().numpy(), done.cpu().numpy())
    print("greedy %s, noops %s: scores %s lengths %s done %s" % (greedy, noops_e, got[0], got[1], got[2]))
    assert np.array_equal(got[0], want_score) and np.array_equal(got[1], want_length) and np.array_equal(got[2], want_done)
    assert int(alive.item()) == N - int(want_done.sum())
    replayed = evaluation.replay_on_twins(env_creator, trace, noops_e, env_offset=env_offset)
    assert np.array_equal(got[0], replayed[0]) and np.array_equal(got[1], replayed[1])
    assert np.array_equal(got[1][got[2] == 0], EVAL_STEPS - noops_e[got[2] == 0])          # still playing: every step was scored
    assert (got[1][got[2] == 1] >= 35 - noops).all()          # five unreturned serves of seven steps, less the no-ops among them
    if not greedy:
        assert len(set(trace[noops:].reshape(-1).tolist())) >= 4 and got[2].sum() >= 1
