"""CPU: the rally game's specification (paac_amd/rally.py) and its wiring into the command line, the environment factory
and the evaluation harness."""
import json
import os

import numpy as np
import pytest

from paac_amd import environment_creator, evaluation, rally, train
from paac_amd.rally import RallyEnvironment
from paac_amd.synthetic import lowbias32_int, synth_key

ONE_HOT = np.eye(6)
SEED = 3
ACTIVE, LAZY_STEP = 10, 9          # steps values of (seed 3, environment 0, episode 0) on which the opponent may / may not move


def S(bx, by, dx, dy, px, ox, mine=0, theirs=0, steps=ACTIVE, k=0):
    return (bx, by, dx, dy, px, ox, mine, theirs, steps, k)


def step(state, a, env=0):
    return rally.step_state(SEED, env, state, a)


def served(env, k, s):
    """(bx, dx) of serve s of episode k, from the spec's formula."""
    w = lowbias32_int(synth_key(SEED, env, k) ^ (0xA11E0002 + 16 * s))
    return (w >> 1) % 14, (1 if w & 1 else -1)


def lazy(env, k, steps):
    return lowbias32_int(synth_key(SEED, env, k) ^ (0xA11E1000 + steps)) % 4 == 0


def test_constants():
    assert (rally.POINTS, rally.MAX_STEPS, rally.REACT_ROW, rally.LAZY, rally.NUM_ACTIONS) == (5, 1000, 5, 4, 6)
    assert rally.STATE_WORDS == 12 and (rally.BALL, rally.PADDLE, rally.OPPONENT) == (255, 128, 64)
    assert not lazy(0, 0, ACTIVE) and lazy(0, 0, LAZY_STEP)


@pytest.mark.parametrize("g,k,want", [(0, 0, (5, 6, -1, 1, 12, 3)), (1, 0, (3, 6, -1, 1, 8, 0)), (2, 0, (4, 6, 1, 1, 7, 4)),
                                      (0, 1, (8, 6, -1, 1, 0, 5))])
def test_anchor_start_states(g, k, want):
    state = rally.start_state(SEED, g, k)
    assert state == want + (0, 0, 0, k)
    h = synth_key(SEED, g, k)
    assert (state[4], state[5]) == (lowbias32_int(h ^ 0xA11E0001) % 13, lowbias32_int(h ^ 0xA11E0003) % 13)
    assert (state[0], state[2]) == served(g, k, 0)
    if k == 0:
        assert RallyEnvironment(g, seed=SEED).state == state


def test_agent_paddle_moves_and_clamps_at_both_walls():
    mid = lambda px, a: step(S(6, 8, 1, 1, px, 3), a)[0][4]
    assert mid(0, 3) == 0 and mid(1, 3) == 0 and mid(12, 2) == 12 and mid(11, 2) == 12
    assert mid(0, 5) == 0 and mid(12, 4) == 12
    assert mid(6, 0) == 6 and mid(6, 1) == 6 and mid(6, 2) == 7 and mid(6, 3) == 5 and mid(6, 4) == 7 and mid(6, 5) == 5
    assert mid(0, 2) == 1 and mid(12, 3) == 11


def test_action_aliases():
    rs = np.random.RandomState(2)
    states = [S(5, 12, 1, 1, 7, 3), S(5, 12, 1, 1, 4, 3), S(5, 1, 1, -1, 9, 0), S(0, 8, -1, 1, 0, 12)]
    for g in range(4):
        state = rally.start_state(SEED, g, 0)
        for _ in range(60):
            states.append(state)
            state = step(state, rs.randint(6), env=g)[0]
    for state in states:
        assert step(state, 1) == step(state, 0) and step(state, 4) == step(state, 2) and step(state, 5) == step(state, 3)
    assert step(states[0], 2) != step(states[0], 0) != step(states[0], 3)


def test_wall_hit_keeps_the_column():
    assert step(S(0, 8, -1, 1, 5, 3), 0) == (S(0, 9, 1, 1, 5, 3, steps=11), 0.0, False)
    assert step(S(13, 8, 1, -1, 5, 3), 0) == (S(13, 7, -1, -1, 5, 3, steps=11), 0.0, False)
    assert step(S(1, 8, -1, 1, 5, 3), 0) == (S(0, 9, -1, 1, 5, 3, steps=11), 0.0, False)          # reaching the wall is no hit
    assert step(S(12, 8, 1, 1, 5, 3), 0) == (S(13, 9, 1, 1, 5, 3, steps=11), 0.0, False)


def test_agent_returns_with_the_left_cell_and_the_right_cell():
    assert step(S(5, 12, 1, 1, 6, 3), 0) == (S(6, 12, -1, -1, 6, 3, steps=11), 0.0, False)          # left cell: up and left
    assert step(S(5, 12, 1, 1, 5, 3), 0) == (S(6, 12, 1, -1, 5, 3, steps=11), 0.0, False)           # right cell: up and right
    assert step(S(7, 12, -1, 1, 5, 3), 0) == (S(6, 12, 1, -1, 5, 3, steps=11), 0.0, False)
    # the paddle moves before the ball lands
    assert step(S(5, 12, 1, 1, 7, 3), 3) == (S(6, 12, -1, -1, 6, 3, steps=11), 0.0, False)
    assert step(S(5, 12, 1, 1, 4, 3), 2) == (S(6, 12, 1, -1, 5, 3, steps=11), 0.0, False)
    assert step(S(5, 12, 1, 1, 6, 3), 3) == (S(6, 12, 1, -1, 5, 3, steps=11), 0.0, False)           # left cell becomes right cell
    # a wall hit in row 12: the ball comes down in its own column
    assert step(S(13, 12, 1, 1, 12, 3), 0) == (S(13, 12, 1, -1, 12, 3, steps=11), 0.0, False)
    assert step(S(0, 12, -1, 1, 0, 3), 0) == (S(0, 12, -1, -1, 0, 3, steps=11), 0.0, False)


def test_opponent_returns_with_the_left_cell_and_the_right_cell():
    # the ball enters row 0 in column 6; an opponent that covers it does not move, lazy or not
    for steps in (ACTIVE, LAZY_STEP):
        assert step(S(5, 1, 1, -1, 9, 6, steps=steps), 0) == (S(6, 1, -1, 1, 9, 6, steps=steps + 1), 0.0, False)
        assert step(S(5, 1, 1, -1, 9, 5, steps=steps), 0) == (S(6, 1, 1, 1, 9, 5, steps=steps + 1), 0.0, False)
        assert step(S(7, 1, -1, -1, 9, 5, steps=steps), 0) == (S(6, 1, 1, 1, 9, 5, steps=steps + 1), 0.0, False)
    # the opponent moves before the ball arrives: one cell off becomes a return on an active step, a point on a lazy one
    assert step(S(5, 1, 1, -1, 9, 7), 0) == (S(6, 1, -1, 1, 9, 6, steps=11), 0.0, False)
    assert step(S(5, 1, 1, -1, 9, 4), 0) == (S(6, 1, 1, 1, 9, 5, steps=11), 0.0, False)
    assert step(S(5, 1, 1, -1, 9, 7, steps=LAZY_STEP), 0)[1:] == (1.0, False)
    # at the walls
    assert step(S(13, 1, 1, -1, 9, 12), 0) == (S(13, 1, 1, 1, 9, 12, steps=11), 0.0, False)
    assert step(S(0, 1, -1, -1, 9, 0), 0) == (S(0, 1, -1, 1, 9, 0, steps=11), 0.0, False)


def test_agent_miss_is_minus_one_and_the_serve_comes_to_the_agent():
    for env in range(4):
        state, r, t = step(S(5, 12, 1, 1, 9, 3, mine=1, theirs=2, k=2), 2, env=env)
        bx, dx = served(env, 2, 4)
        assert (state, r, t) == (S(bx, 6, dx, 1, 10, 3, mine=1, theirs=3, steps=11, k=2), -1.0, False)
    assert step(S(5, 12, 1, 1, 7, 3), 0)[1] == -1.0 and step(S(5, 12, 1, 1, 4, 3), 0)[1] == -1.0        # one cell off, either side
    assert step(S(5, 12, 1, 1, 6, 3), 2)[1] == -1.0 and step(S(5, 12, 1, 1, 5, 3), 3)[1] == -1.0        # moving away misses


def test_opponent_miss_is_plus_one_and_the_serve_goes_to_the_opponent():
    for env in range(4):
        state, r, t = step(S(5, 1, 1, -1, 9, 0, mine=2, k=2, steps=LAZY_STEP), 0, env=env)
        bx, dx = served(env, 2, 3)
        ox = 0 if lazy(env, 2, LAZY_STEP) else 1            # it may take a step towards the ball; the paddles stay otherwise
        assert (state, r, t) == (S(bx, 7, dx, -1, 9, ox, mine=3, steps=LAZY_STEP + 1, k=2), 1.0, False)


def test_serve_hash_differs_per_serve_and_per_episode():
    serves = {tuple(served(env, k, s) for s in range(3)) for env in range(8) for k in range(8)}
    assert len(serves) > 32
    assert {served(env, 0, s)[1] for env in range(4) for s in range(9)} == {-1, 1}
    assert len({served(0, 0, s)[0] for s in range(9)}) > 3
    start = rally.start_state(SEED, 5, 3)
    for s in range(9):
        bx, dx = served(5, 3, s)
        assert rally.serve(SEED, 5, start, s, True) == (bx, 6, dx, 1) + start[4:]
        assert rally.serve(SEED, 5, start, s, False) == (bx, 7, dx, -1) + start[4:]


def test_opponent_moves_only_near_with_the_ball_flying_up_and_never_on_a_lazy_step():
    ox_after = lambda state: step(state, 0)[0][5]
    # the ball at (5, by) flying up and right enters row 0 in column 5 + by
    assert ox_after(S(5, 5, 1, -1, 9, 0)) == 1 and ox_after(S(5, 5, 1, -1, 9, 12)) == 11          # row 5 is near
    assert ox_after(S(5, 6, 1, -1, 9, 0)) == 0 and ox_after(S(5, 6, 1, -1, 9, 12)) == 12          # row 6 is not
    assert ox_after(S(5, 3, 1, 1, 9, 0)) == 0 and ox_after(S(5, 3, 1, 1, 9, 12)) == 12            # the ball flies down
    assert ox_after(S(5, 5, 1, -1, 9, 0, steps=LAZY_STEP)) == 0 and ox_after(S(5, 5, 1, -1, 9, 12, steps=LAZY_STEP)) == 12
    assert ox_after(S(5, 3, 1, -1, 9, 0)) == 1 and ox_after(S(5, 2, -1, -1, 9, 12)) == 11
    # it stays when either of its cells is the entry column (8 here), and moves one cell at a time otherwise
    assert ox_after(S(5, 3, 1, -1, 9, 8)) == 8 and ox_after(S(5, 3, 1, -1, 9, 7)) == 7
    assert ox_after(S(5, 3, 1, -1, 9, 6)) == 7 and ox_after(S(5, 3, 1, -1, 9, 9)) == 8 and ox_after(S(5, 3, 1, -1, 9, 2)) == 3
    # about one step in four is lazy
    count = sum(lazy(0, 0, t) for t in range(1000))
    assert 200 < count < 300
    assert rally.opponent_moves(SEED, 0, S(5, 5, 1, -1, 9, 0)) and not rally.opponent_moves(SEED, 0, S(5, 5, 1, -1, 9, 0, steps=LAZY_STEP))


def test_opponent_aims_at_the_entry_column_after_a_wall_bounce():
    # (1, 3) flying up and left: column 0, the wall (the ball keeps column 0), column 1 -- not 2 (a mirror), not 0 (a clip)
    assert rally.entry_column(1, -1, 3) == (1, 1)
    assert step(S(1, 3, -1, -1, 9, 2), 0)[0][5] == 1 and step(S(1, 3, -1, -1, 9, 1), 0)[0][5] == 1
    assert step(S(1, 3, -1, -1, 9, 0), 0)[0][5] == 0
    # (12, 4) flying up and right: 13, wall, 12, 11
    assert rally.entry_column(12, 1, 4) == (11, -1)
    assert step(S(12, 4, 1, -1, 9, 12), 0)[0][5] == 11 and step(S(12, 4, 1, -1, 9, 11), 0)[0][5] == 11
    assert step(S(12, 4, 1, -1, 9, 10), 0)[0][5] == 10 and step(S(12, 4, 1, -1, 9, 9), 0)[0][5] == 10


def test_fifth_point_at_either_end_is_terminal_and_starts_the_next_episode():
    nxt = rally.start_state(SEED, 6, 4)
    assert nxt[6:] == (0, 0, 0, 4)
    assert step(S(5, 1, 1, -1, 9, 0, mine=4, theirs=2, k=3), 0, env=6) == (nxt, 1.0, True)
    assert step(S(5, 12, 1, 1, 9, 3, mine=1, theirs=4, k=3), 0, env=6) == (nxt, -1.0, True)
    assert step(S(5, 12, 1, 1, 9, 3, mine=4, theirs=4, k=3), 0, env=6) == (nxt, -1.0, True)
    # the fourth point is not, and a return with four points on the board is not
    assert step(S(5, 1, 1, -1, 9, 0, mine=3, theirs=4, k=3), 0, env=6)[1:] == (1.0, False)
    assert step(S(5, 12, 1, 1, 9, 3, mine=4, theirs=3, k=3), 0, env=6)[1:] == (-1.0, False)
    assert step(S(5, 12, 1, 1, 6, 3, mine=4, theirs=4, k=3), 0, env=6)[1:] == (0.0, False)


def test_step_cap_alone_and_together_with_a_reward():
    nxt = rally.start_state(SEED, 1, 1)
    assert step(S(5, 8, 1, 1, 9, 3, steps=998), 0, env=1) == (S(6, 9, 1, 1, 9, 3, steps=999), 0.0, False)
    assert step(S(5, 8, 1, 1, 9, 3, steps=999), 0, env=1) == (nxt, 0.0, True)
    assert step(S(5, 12, 1, 1, 6, 3, steps=999), 0, env=1) == (nxt, 0.0, True)              # a return on the capping step
    assert step(S(5, 12, 1, 1, 9, 3, steps=999), 0, env=1) == (nxt, -1.0, True)             # a point against
    assert step(S(5, 1, 1, -1, 9, 0, steps=999), 0, env=1) == (nxt, 1.0, True)              # a point for
    assert step(S(5, 1, 1, -1, 9, 0, mine=4, steps=999), 0, env=1) == (nxt, 1.0, True)      # ... the fifth


def test_ball_stays_in_rows_1_to_12_and_the_state_in_range():
    rs = np.random.RandomState(5)
    points = [0, 0]
    for env in range(4):
        state = rally.start_state(SEED, env, 0)
        for n in range(3000):
            # half of the time a reference policy, so that rallies get long and the ball reaches both ends
            a = rally.aim_action(state) if rs.rand() < 0.5 else rs.randint(6)
            before = state
            state, r, t = step(state, a, env=env)
            bx, by, dx, dy, px, ox, mine, theirs, steps, k = state
            assert 0 <= bx <= 13 and 1 <= by <= 12 and dx in (-1, 1) and dy in (-1, 1) and 0 <= px <= 12 and 0 <= ox <= 12
            assert 0 <= mine < 5 and 0 <= theirs < 5 and 0 <= steps < 1000 and r in (-1.0, 0.0, 1.0)
            assert abs(px - before[4]) <= 1 and abs(ox - before[5]) <= 1 or t
            assert k == before[9] + int(t)
            if r and not t:
                assert (mine + theirs) == before[6] + before[7] + 1 and (by, dy) == ((6, 1) if r < 0 else (7, -1))
            points[r > 0] += r != 0
    assert points[0] > 20 and points[1] > 20


def brute_plane(state):
    bx, by, px, ox = state[0], state[1], state[4], state[5]
    want = np.zeros((84, 84), dtype=np.uint8)
    for y in range(84):
        for x in range(84):
            cy, cx = y // 6, x // 6
            if (cy, cx) == (by, bx):
                want[y, x] = 255
            elif cy == 13 and cx in (px, px + 1):
                want[y, x] = 128
            elif cy == 0 and cx in (ox, ox + 1):
                want[y, x] = 64
    return want


def test_plane_values_and_cell_boundaries():
    p = rally.plane(S(0, 1, 1, 1, 12, 0))
    assert p.shape == (84, 84) and p.dtype == np.uint8
    assert np.all(p[6:12, 0:6] == 255) and p[6, 6] == 0 and p[12, 0] == 0 and p[11, 5] == 255
    assert np.all(p[0:6, 0:12] == 64) and p[5, 11] == 64 and p[5, 12] == 0 and p[0, 12] == 0          # the opponent at ox = 0
    assert np.all(p[78:84, 72:84] == 128) and p[77, 72] == 0 and p[78, 71] == 0                         # the agent at px = 12
    assert sorted(np.unique(p)) == [0, 64, 128, 255]
    assert int((p == 255).sum()) == 36 and int((p == 128).sum()) == 72 and int((p == 64).sum()) == 72
    p = rally.plane(S(13, 12, 1, 1, 0, 12))
    assert np.all(p[72:78, 78:84] == 255) and p[71, 78] == 0 and p[72, 77] == 0
    assert np.all(p[0:6, 72:84] == 64) and p[0, 71] == 0 and np.all(p[78:84, 0:12] == 128) and p[78, 12] == 0
    for state in (S(0, 1, 1, 1, 12, 0), S(3, 12, -1, 1, 3, 3), S(13, 7, 1, 1, 7, 5), S(6, 1, 1, -1, 0, 6),
                  rally.start_state(SEED, 0, 0)):
        assert np.array_equal(rally.plane(state), brute_plane(state))


def test_stack_shifts_one_channel_per_step_and_restarts_after_a_terminal():
    env = RallyEnvironment(0, seed=SEED)          # (5, 6, -1, 1, 12, 3): the ball passes the paddle on step 7
    obs = env.get_initial_state()
    assert obs.shape == (84, 84, 4) and obs.dtype == np.uint8
    assert obs[..., :3].max() == 0 and np.array_equal(obs[..., 3], rally.plane(env.state))
    planes = [obs[..., 3]]
    for n in range(6):
        new, r, t = env.next(ONE_HOT[0])
        assert (r, t) == (0.0, False) and env.state[8] == n + 1
        planes.append(rally.plane(env.state))
        assert np.array_equal(new[..., 3], planes[-1])
        for c in range(3):
            assert np.array_equal(new[..., c], obs[..., c + 1])
        obs = new
    assert np.array_equal(obs[..., 0], planes[-4]) and not np.array_equal(planes[-1], planes[-2])
    new, r, t = env.next(ONE_HOT[0])
    assert (r, t) == (-1.0, False) and env.state[:4] == served(0, 0, 1)[:1] + (6,) + served(0, 0, 1)[1:] + (1,)
    assert np.array_equal(new[..., :3], obs[..., 1:])              # a point alone keeps the history
    env.state = env.state[:7] + (4,) + env.state[8:]               # four points against: the next one ends the episode
    while True:
        _, r, t = env.next(ONE_HOT[0])
        if r:
            break
    assert (r, t) == (-1.0, True) and env.k == 1 and env.state == rally.start_state(SEED, 0, 1)
    obs = env.get_initial_state()              # what the runner shows after a terminal: never the terminal position
    assert obs[..., :3].max() == 0 and np.array_equal(obs[..., 3], rally.plane(rally.start_state(SEED, 0, 1)))
    again = env.get_initial_state()            # asking twice starts no further episode
    assert np.array_equal(obs, again) and env.k == 1


def play(policy, episodes=16, envs=64):
    """-> (returns, lengths) [envs, episodes] of the first `episodes` episodes of environments 0..envs-1 under policy(state)."""
    returns, lengths = [], []
    for g in range(envs):
        state, total, n, done = rally.start_state(SEED, g, 0), 0.0, 0, 0
        while done < episodes:
            state, r, t = rally.step_state(SEED, g, state, policy(state))
            total += r
            n += 1
            if t:
                returns.append(total)
                lengths.append(n)
                total, n, done = 0.0, 0, done + 1
    return np.asarray(returns).reshape(envs, episodes), np.asarray(lengths).reshape(envs, episodes)


# the module docstring's scores: sum of the 1024 returns, sum of the 64 first-episode returns, episodes at the step cap,
# shortest and longest episode
def test_uniform_random_policy_score():
    rs = np.random.RandomState(0)
    returns, lengths = play(lambda state: rs.randint(6))
    assert (returns.sum(), returns[:, 0].sum()) == (-4616.0, -282.0)
    assert (lengths.min(), lengths.max(), int((lengths == 1000).sum())) == (35, 203, 0)
    assert abs(returns.std() - 1.062) < 1e-3 and abs(lengths.mean() - 60.5) < 0.05


def test_always_noop_policy_score():
    returns, lengths = play(lambda state: 0)
    assert (returns.sum(), returns[:, 0].sum()) == (-4006.0, -262.0)
    assert (lengths.min(), lengths.max(), int((lengths == 1000).sum())) == (35, 1000, 233)
    assert abs(returns.std() - 1.670) < 1e-3 and abs(lengths.mean() - 266.1) < 0.05


def test_return_action_score():
    returns, lengths = play(rally.return_action)
    assert (returns.sum(), returns[:, 0].sum()) == (397.0, 42.0)
    assert int((lengths == 1000).sum()) == 1015 and abs(lengths.mean() - 991.7) < 0.05 and abs(returns.std() - 1.093) < 1e-3


def test_aim_action_score():
    returns, lengths = play(rally.aim_action)
    assert (returns.sum(), returns[:, 0].sum()) == (4179.0, 243.0)
    assert int((lengths == 1000).sum()) == 313 and abs(lengths.mean() - 693.3) < 0.05 and abs(returns.std() - 1.428) < 1e-3


def test_reference_policies_read_the_landing_column():
    # (5, 10) flying down and right lands in column 8 with dx = +1
    assert rally.entry_column(5, 1, 3) == (8, 1)
    ret = lambda px: rally.return_action(S(5, 10, 1, 1, px, 3))
    assert ret(0) == 2 and ret(6) == 2 and ret(7) == 0 and ret(8) == 0 and ret(9) == 3
    aim = lambda px, dx=1, bx=5: rally.aim_action(S(bx, 10, dx, 1, px, 3))
    assert aim(6) == 2 and aim(7) == 0 and aim(8) == 3                    # the right cell under column 8
    assert aim(1, dx=-1) == 2 and aim(2, dx=-1) == 0 and aim(3, dx=-1) == 3          # column 2 with dx = -1: the left cell
    assert rally.entry_column(12, 1, 3) == (12, -1) and aim(11, bx=12) == 2 and aim(12, bx=12) == 0          # after a wall bounce
    assert aim(1, dx=-1, bx=2) == 3 and aim(0, dx=-1, bx=2) == 0           # (2, 10): 1, 0, wall: column 0 with dx = +1, clamped
    # both stay while the ball flies up
    assert rally.return_action(S(5, 10, 1, -1, 0, 3)) == 0 and rally.aim_action(S(5, 10, 1, -1, 0, 3)) == 0


def test_call_pattern_of_the_plugin_surface():
    env = RallyEnvironment(2, seed=5)
    assert list(env.get_legal_actions()) == [0, 1, 2, 3, 4, 5] and list(env.get_noop()) == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert env.num_actions == 6
    words = env.state_words()
    assert words.dtype == np.int32 and words.shape == (rally.STATE_WORDS,) == (12,) and list(words) == list(env.state) + [0, 0]
    px = env.state[4]
    env.get_initial_state()
    obs, r, t = env.next(env.get_noop())
    assert env.state[4] == px and env.state[8] == 1 and obs.shape == (84, 84, 4) and (r, t) == (0.0, False)


def test_emulator_rally_parses_and_gives_six_actions():
    args = train.get_arg_parser().parse_args("--emulator rally -g breakout".split())
    assert args.emulator == "rally"
    creator = environment_creator.EnvironmentCreator(args)
    assert creator.num_actions == 6                      # -g is ignored (breakout has 4)
    network_creator, creator = train.get_network_and_environment_creator(args)
    assert args.num_actions == 6
    env = creator.create_environment(2)
    assert isinstance(env, RallyEnvironment) and env.actor_id == 2 and env.seed == args.random_seed == 3
    assert env.state == rally.start_state(3, 2, 0)
    assert creator.device_env_spec == dict(kind="rally", seed=3)
    assert "rally" in train.get_arg_parser().format_help()


def test_single_life_episodes_does_not_apply():
    args = train.get_arg_parser().parse_args("--emulator rally --single_life_episodes true".split())
    _, creator = train.get_network_and_environment_creator(args)
    assert creator.device_env_spec == dict(kind="rally", seed=3)
    assert creator.create_environment(0).state == rally.start_state(3, 0, 0)


def test_emulator_rally_refuses_raw_frames():
    args = train.get_arg_parser().parse_args("--emulator rally --synthetic_raw_frames true".split())
    with pytest.raises(ValueError, match="raw"):
        environment_creator.EnvironmentCreator(args)


def test_other_emulators_keep_their_specs():
    from paac_amd.bricks import BricksEnvironment
    from paac_amd.catch import CatchEnvironment
    from paac_amd.synthetic import terminal_threshold
    args = train.get_arg_parser().parse_args("--emulator catch --single_life_episodes true".split())
    _, creator = train.get_network_and_environment_creator(args)
    assert creator.device_env_spec == dict(kind="catch", seed=3) and isinstance(creator.create_environment(0), CatchEnvironment)
    assert creator.num_actions == 3
    args = train.get_arg_parser().parse_args("--emulator bricks --single_life_episodes true".split())
    _, creator = train.get_network_and_environment_creator(args)
    assert creator.device_env_spec == dict(kind="bricks", seed=3, single_life=True) and creator.num_actions == 3
    assert isinstance(creator.create_environment(0), BricksEnvironment)
    args = train.get_arg_parser().parse_args("-g breakout".split())
    _, creator = train.get_network_and_environment_creator(args)
    assert creator.device_env_spec == dict(kind="synthetic", seed=3, terminal_threshold=terminal_threshold(0.01),
                                           raw_frames=False)
    assert creator.num_actions == 4


def test_evaluation_settings_restore_rally_environments(tmp_path):
    from paac_amd import logger_utils, test as test_cli
    args = train.get_arg_parser().parse_args("--emulator rally".split())
    logger_utils.save_args(args, str(tmp_path))
    assert json.load(open(os.path.join(str(tmp_path), "args.json")))["emulator"] == "rally"
    settings = test_cli.restore_settings(test_cli.get_arg_parser().parse_args(["-f", str(tmp_path)]))
    assert settings.emulator == "rally"
    _, creator = train.get_network_and_environment_creator(settings, random_seed=11)
    env = creator.create_environment(1)
    assert isinstance(env, RallyEnvironment) and env.seed == 11 and creator.num_actions == 6
    assert creator.device_env_spec == dict(kind="rally", seed=11)


def test_evaluation_accepts_rally_and_bounds_it():
    from paac_amd.paac import STATEFUL_KINDS
    assert STATEFUL_KINDS["rally"]["max_episode_steps"] == 1000 == rally.MAX_STEPS
    assert STATEFUL_KINDS["rally"]["words"] == rally.STATE_WORDS and STATEFUL_KINDS["rally"]["spec_kwargs"] == ()
    assert evaluation.max_steps_of("rally", 30) == 1030 and evaluation.max_steps_of("rally", 0) == 1000
    assert evaluation.check_env_spec(dict(kind="rally", seed=3)) == "rally"
    with pytest.raises(ValueError, match=r"--emulator catch\|bricks\|rally"):
        evaluation.check_env_spec(dict(kind="synthetic", seed=3))
    args = train.get_arg_parser().parse_args("--emulator rally --eval_every 160".split())
    assert evaluation.check_train_flags(args) is True
    args = train.get_arg_parser().parse_args("--emulator synthetic --eval_every 160".split())
    with pytest.raises(ValueError, match=r"catch\|bricks\|rally"):
        evaluation.check_train_flags(args)
    args = train.get_arg_parser().parse_args("--emulator rally --eval_every 160 --host_environments true".split())
    with pytest.raises(ValueError, match="host_environments"):
        evaluation.check_train_flags(args)


def test_replay_on_twins_scores_a_rally_trace():
    """evaluation.replay_on_twins on RallyEnvironment twins: always-NOOP traces reproduce play()'s first episodes."""
    args = train.get_arg_parser().parse_args("--emulator rally".split())
    _, creator = train.get_network_and_environment_creator(args)
    steps = 120
    score, length = evaluation.replay_on_twins(creator, np.zeros((steps, 4), dtype=np.int32), 0)
    returns, lengths = play(lambda state: 0, episodes=1, envs=4)
    for e in range(4):
        if lengths[e, 0] <= steps:
            assert (score[e], length[e]) == (returns[e, 0], lengths[e, 0])
        else:
            assert length[e] == steps
    assert (lengths[:, 0] <= steps).any()
