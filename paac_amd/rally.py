"""Rally: a two-paddle game with an opponent, resident on the GPU.  A ball flies between the agent's paddle in the bottom row and
a scripted opponent's in the top row; a ball that passes a paddle is a point for the other side, first to five.

This is the SPEC of the rally environment family; the same numbers are produced
  * on the host by `RallyEnvironment` (a BaseEnvironment plugin, numpy and pure Python), and
  * on the device by paac_rally_reset / paac_rally_step (csrc/rally_dev.h, csrc/games.hip), N envs per launch.
Catch (catch.py) is a 13-step bandit and bricks (bricks.py) a long game with lives; both have three actions, no adversary and no
negative reward.  This game has an opponent that plays back, rewards of both signs, the six actions of ALE Pong's minimal set
(aliases included) and episodes of up to 1000 steps.  Call pattern as BricksEnvironment's: get_initial_state() /
next(one_hot) -> (obs, reward, terminal).

Spec (all hashing reuses lowbias32 and h = synth_key(seed, g, k) of synthetic.py unchanged; g = the global environment
env_offset + e, k = the episode index):
  board          14 x 14 cells of 6 x 6 pixels = 84 x 84; columns and rows 0..13, row 0 at the top
  paddles        the agent's in row 13 on cells px, px + 1; the opponent's in row 0 on cells ox, ox + 1; px, ox in 0..12
  ball           cell (bx, by), velocity dx in {-1, +1}, dy in {-1, +1}; it only ever occupies rows 1..12
  constants      POINTS = 5, MAX_STEPS = 1000, REACT_ROW = 5, LAZY = 4, A = 6 actions: 0 NOOP, 1 FIRE (= NOOP), 2 RIGHT, 3 LEFT,
                 4 RIGHTFIRE (= RIGHT), 5 LEFTFIRE (= LEFT)
  state          per environment, int32: (bx, by, dx, dy, px, ox, mine, theirs, steps, k); mine / theirs = the points of the
                 agent / the opponent, steps = the steps taken in the current episode, k = the number of episodes this
                 environment has started before the current one; the device record is these 10 words and two words of padding
                 (STATE_WORDS = 12: three 16-byte parts)
  episode start  px = lowbias32(h ^ 0xA11E0001) % 13, ox = lowbias32(h ^ 0xA11E0003) % 13, mine = theirs = steps = 0, then serve
                 number 0 towards the agent
  serve s        (s = the points played so far in the episode) w = lowbias32(h ^ (0xA11E0002 + 16 * s)):
                   bx = (w >> 1) % 14, dx = +1 if w & 1 else -1; towards the agent dy = +1, by = 6; towards the opponent
                   dy = -1, by = 7.  After a point the serve goes towards the side that conceded it; the paddles stay.
  step(a)        in this order:
                   1. agent: a in (2, 4): px = min(px + 1, 12); a in (3, 5): px = max(px - 1, 0)
                   2. opponent: it moves only if dy < 0 and by <= REACT_ROW and lowbias32(h ^ (0xA11E1000 + steps)) % LAZY != 0
                      (steps before this step's increment).  tx = the column in which the ball would enter row 0: the x rule
                      of 3. run forward `by` times from (bx, dx).  tx < ox: ox -= 1; tx > ox + 1: ox += 1
                   3. nx = bx + dx; if nx < 0 or nx > 13: dx = -dx, nx = bx (bricks' wall rule: the ball keeps its column)
                   4. ny = by + dy;
                        ny == 13 and nx in (px, px + 1): dy = -1, dx = -1 on the left cell and +1 on the right one, ny = by
                        ny == 13 otherwise: theirs += 1, reward -1
                        ny == 0: the same against ox with dy = +1; a miss gives mine += 1, reward +1
                        else the ball moves to (nx, ny)
                   5. steps += 1; terminal if mine == POINTS or theirs == POINTS or steps == MAX_STEPS
                   6. a terminal step starts episode k + 1 at once; a non-terminal step that scored a point is followed by
                      serve mine + theirs
                 truncated: the step is terminal ONLY because steps == MAX_STEPS -- neither side reached POINTS on it.  A step
                 that is both the fifth point and at the cap is not truncated (--bootstrap_truncated reads this)
  plane(state)   a pixel in cell (cy, cx) = 255 if (cy, cx) == (by, bx), else 128 if cy == 13 and cx in (px, px + 1), else 64
                 if cy == 0 and cx in (ox, ox + 1), else 0
  observation    bricks' rule: the previous stack shifted by one channel with the new plane as channel 3; at construction and
                 after a terminal step it is [0, 0, 0, plane of the new start state] -- the terminal position is never shown
  bookkeeping    as bricks': reward clipped to [-1, 1] (a no-op here), mask = 0 on terminal, ep_reward / ep_len totals, the
                 finished-episode ring
--single_life_episodes (there are no lives), -g, --synthetic_terminal_p and --random_start do not apply.

Anchors, seed 3, (g, k) -> (bx, by, dx, dy, px, ox): (0, 0) -> (5, 6, -1, 1, 12, 3); (1, 0) -> (3, 6, -1, 1, 8, 0);
(2, 0) -> (4, 6, 1, 1, 7, 4); (0, 1) -> (8, 6, -1, 1, 0, 5).
Scores, seed 3, environments 0..63, the first 16 episodes of each (1024 episodes; uniform random drawn with
RandomState(0).randint(6), environment after environment), and in brackets the mean over the first episode of each (64 episodes):
  uniform random   mean return -4.5078 (sum -4616), std 1.062, lengths 35 to 203, mean 60.5                       [-4.4063]
  always NOOP      mean return -3.9121 (sum -4006), std 1.670, lengths 35 to 1000, mean 266.1, 233 at the step cap  [-4.0938]
  return_action    mean return +0.3877 (sum +397), std 1.093, mean length 991.7, 1015 episodes at the step cap      [+0.6563]
  aim_action       mean return +4.0811 (sum +4179), std 1.428, mean length 693.3, 313 episodes at the step cap      [+3.7969]
Chance, then "return the ball" (the opponent returns nearly everything it can reach: a draw at the step cap), then "aim it".
"""
import numpy as np

from .environment import BaseEnvironment
from .synthetic import lowbias32_int, synth_key

CELLS = 14                 # board cells per side
CELL = 6                   # pixels per cell side
NUM_ACTIONS = 6
POINTS = 5
MAX_STEPS = 1000
REACT_ROW = 5              # the opponent reacts to a ball flying up in rows 1..REACT_ROW
LAZY = 4                   # ... except on one step in LAZY
NOOP, FIRE, RIGHT, LEFT, RIGHTFIRE, LEFTFIRE = range(6)
BALL, PADDLE, OPPONENT = 255, 128, 64  # pixel values
STATE_WORDS = 12           # int32 words of a device state record: the 10 state words, then padding


def serve(seed, env, state, s, towards_agent):
    """The state with the ball served for the s-th time in its episode; the paddles stay where they are."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = state
    w = lowbias32_int(synth_key(seed, env, k) ^ (0xA11E0002 + 16 * s))
    bx, dx = (w >> 1) % CELLS, (1 if w & 1 else -1)
    by, dy = (6, 1) if towards_agent else (7, -1)
    return (bx, by, dx, dy, px, ox, mine, theirs, steps, k)


def start_state(seed, env, k):
    """-> the state episode k of global environment env starts from."""
    h = synth_key(seed, env, k)
    px = lowbias32_int(h ^ 0xA11E0001) % (CELLS - 1)
    ox = lowbias32_int(h ^ 0xA11E0003) % (CELLS - 1)
    return serve(seed, env, (0, 0, 0, 0, px, ox, 0, 0, 0, k), 0, True)


def entry_column(bx, dx, n):
    """The x rule of a step run forward n times from column bx with sideways direction dx -> (column, dx on arrival)."""
    for _ in range(n):
        nx = bx + dx
        if nx < 0 or nx > CELLS - 1:
            dx = -dx
            nx = bx
        bx = nx
    return bx, dx


def opponent_moves(seed, env, state):
    """Whether the opponent reacts on the step `state` is about to take (the ball flies up, is near, and the step is not lazy)."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = state
    return dy < 0 and by <= REACT_ROW and lowbias32_int(synth_key(seed, env, k) ^ (0xA11E1000 + steps)) % LAZY != 0


def step_state(seed, env, state, a):
    """One step of `state` under action a -> (state, reward, terminal).  The state returned is the one the next step starts
    from: after a terminal step that is the start state of episode k + 1 (the device record's rule)."""
    return step_state_truncated(seed, env, state, a)[:3]


def step_state_truncated(seed, env, state, a):
    """step_state with the reason of a terminal step -> (state, reward, terminal, truncated): truncated = the step is terminal
    only because steps reached MAX_STEPS (neither side reached POINTS on it).  The cap is a time limit, not a property of the
    state: --bootstrap_truncated bootstraps the return there."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = state
    if a in (RIGHT, RIGHTFIRE):
        px = min(px + 1, CELLS - 2)
    elif a in (LEFT, LEFTFIRE):
        px = max(px - 1, 0)
    if opponent_moves(seed, env, state):
        tx = entry_column(bx, dx, by)[0]
        if tx < ox:
            ox -= 1
        elif tx > ox + 1:
            ox += 1
    nx = bx + dx
    if nx < 0 or nx > CELLS - 1:
        dx = -dx
        nx = bx
    ny = by + dy
    reward = 0.0
    if ny == CELLS - 1:
        if nx == px or nx == px + 1:
            dy, dx, ny = -1, (-1 if nx == px else 1), by
        else:
            theirs += 1
            reward = -1.0
    elif ny == 0:
        if nx == ox or nx == ox + 1:
            dy, dx, ny = 1, (-1 if nx == ox else 1), by
        else:
            mine += 1
            reward = 1.0
    steps += 1
    decided = mine == POINTS or theirs == POINTS
    if decided or steps == MAX_STEPS:
        return start_state(seed, env, k + 1), reward, True, not decided
    state = (nx, ny, dx, dy, px, ox, mine, theirs, steps, k)
    if reward != 0.0:
        state = serve(seed, env, state, mine + theirs, reward < 0.0)
    return state, reward, False, False


def plane(state):
    bx, by, px, ox = state[0], state[1], state[4], state[5]
    out = np.zeros((84, 84), dtype=np.uint8)
    out[:CELL, ox * CELL:(ox + 2) * CELL] = OPPONENT
    out[(CELLS - 1) * CELL:, px * CELL:(px + 2) * CELL] = PADDLE
    out[by * CELL:(by + 1) * CELL, bx * CELL:(bx + 1) * CELL] = BALL
    return out


def _towards(px, target):
    return LEFT if target < px else (RIGHT if target > px else NOOP)


def return_action(state):
    """Reference policy: stay while the ball flies up, otherwise move the paddle under the column the ball comes down in."""
    bx, by, dx, dy, px = state[:5]
    if dy < 0:
        return NOOP
    tx = entry_column(bx, dx, CELLS - 1 - by)[0]
    return LEFT if tx < px else (RIGHT if tx > px + 1 else NOOP)


def aim_action(state):
    """Reference policy: as return_action, but the ball is met with the left cell when it arrives with dx < 0 and with the right
    cell otherwise -- it keeps its sideways direction and outruns the opponent."""
    bx, by, dx, dy, px = state[:5]
    if dy < 0:
        return NOOP
    tx, arriving = entry_column(bx, dx, CELLS - 1 - by)
    return _towards(px, min(max(tx if arriving < 0 else tx - 1, 0), CELLS - 2))


class RallyEnvironment(BaseEnvironment):
    def __init__(self, actor_id, seed=0):
        self.actor_id = int(actor_id)
        self.num_actions = NUM_ACTIONS
        self.seed = int(seed)
        self.state = start_state(self.seed, self.actor_id, 0)
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.last_step_truncated = False       # the last next() ended its episode at the step cap alone (runners.py reads it)

    @property
    def k(self):
        return self.state[9]

    def state_words(self):
        """The device twin's state record of this environment (int32 [STATE_WORDS])."""
        return np.array(list(self.state) + [0] * (STATE_WORDS - len(self.state)), dtype=np.int32)

    def get_initial_state(self):
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack)

    def next(self, action):
        a = int(np.argmax(action))
        self.state, reward, terminal, self.last_step_truncated = step_state_truncated(self.seed, self.actor_id, self.state, a)
        self.stack[..., :3] = self.stack[..., 1:]
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack), reward, terminal

    def get_legal_actions(self):
        return np.arange(self.num_actions)

    def get_noop(self):
        return [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
