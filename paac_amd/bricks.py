"""Bricks: a brick-wall game with lives, resident on the GPU.  A ball bounces between a paddle and three rows of bricks, +1
for every brick struck; a ball that passes the paddle costs one of three lives.

This is the SPEC of the bricks environment family; the same numbers are produced
  * on the host by `BricksEnvironment` (a BaseEnvironment plugin, numpy and pure Python), and
  * on the device by paac_bricks_reset / paac_bricks_step (csrc/bricks_dev.h, csrc/games.hip), N envs per launch.
Catch (catch.py) is a 13-step bandit: one reward, fixed length, no lives.  This game has a long horizon with dense delayed
reward, episodes of variable length, lives (what --single_life_episodes refers to), a field that changes the observation,
and a ball whose direction cannot be read from one plane -- the frame history is needed.  Call pattern as CatchEnvironment's:
get_initial_state() / next(one_hot) -> (obs, reward, terminal).

Spec (all hashing reuses lowbias32 and key = synth_key(seed, env, id) of synthetic.py unchanged):
  board          14 x 14 cells of 6 x 6 pixels = 84 x 84; columns and rows 0..13, row 0 at the top
  bricks         board rows 2, 3, 4 in all 14 columns (42 bricks), held as three 14-bit masks rows[0..2]: bit c of rows[r] is
                 the brick at board row 2 + r, column c; a full row is 0x3FFF
  paddle         in row 13, two cells wide: columns px and px + 1, px in 0..12
  ball           cell (bx, by), velocity dx in {-1, +1}, dy in {-1, +1}
  constants      LIVES = 3, MAX_STEPS = 500, A = 3 actions: 0 stay, 1 left, 2 right
  state          per environment, int32: (bx, by, dx, dy, px, lives, steps, k, rows[0], rows[1], rows[2]); steps = the steps
                 taken in the current episode, k = the number of episodes this environment has started before the current
                 one; the device record is these 11 words and one word of padding (STATE_WORDS = 12: three 16-byte parts)
  episode start  global environment g = env_offset + e, episode index k, h = synth_key(seed, g, k):
                   px = lowbias32(h ^ 0xB41C0001) % 13, lives = 3, steps = 0, all rows full, then serve number 0
  serve s        (s = 0 at episode start; after a lost life s = LIVES - lives, the life already taken)
                   bx = px, by = 5, dy = +1, dx = +1 if lowbias32(h ^ (0xB41C0002 + 16 * s)) & 1 else -1, h of the current
                   episode -- the ball is served over the paddle's left cell, so every serve can be returned
  step(a)        in this order:
                   1. paddle: a == 1: px = max(px - 1, 0); a == 2: px = min(px + 1, 12)
                   2. nx = bx + dx; if nx < 0 or nx > 13: dx = -dx, nx = bx (the ball keeps its column on a wall hit: that
                      breaks the checkerboard parity of a diagonal ball)
                   3. ny = by + dy; exactly one of, tested in this order:
                        ceiling     ny < 0: dy = +1, ny = by
                        brick       2 <= ny <= 4 and bit nx of rows[ny - 2] set: the bit is cleared, reward 1.0, dy = -dy and
                                    the ball stays where it was (nx = bx, ny = by): it never occupies a brick's cell
                        paddle row  ny == 13: nx == px: dy = -1, dx = -1, ny = by; nx == px + 1: dy = -1, dx = +1, ny = by;
                                    on either hit, all 42 bricks return if all three masks are zero.  Otherwise a miss:
                                    lives -= 1; if lives == 0, or the environment is a single_life one, the step is
                                    terminal, else the ball is served again (serve LIVES - lives, over the paddle where it
                                    stands now).  A miss has no reward.
                        else        the ball moves to (nx, ny)
                   4. steps += 1; steps == MAX_STEPS: the step is terminal whatever else happened
                   5. on a terminal step the environment starts episode k + 1 at once (catch's rule)
                 truncated: the step is terminal ONLY because of rule 4 -- it did not also lose the last life (or, in a
                 single_life environment, any life).  A step that is both a real ending and at the cap is not truncated.
                 The cap is a time limit, not a property of the state: --bootstrap_truncated bootstraps the return there
                 at most 1.0 of reward per step
  plane(state)   a pixel in cell (cy, cx) = 255 if (cy, cx) == (by, bx), else 128 if cy == 13 and cx in (px, px + 1), else 64
                 if 2 <= cy <= 4 and the brick is present, else 0
  observation    catch's rule: the previous stack shifted by one channel with the new plane as channel 3; at construction and
                 after a terminal step it is [0, 0, 0, plane of the new start state] -- the terminal position is never shown
  bookkeeping    as catch's: reward clipped to [-1, 1] (a no-op here), mask = 0 on terminal, ep_reward / ep_len totals, the
                 finished-episode ring

Anchors, seed 3, (g, k) -> (bx, by, dx, dy, px): (0, 0) -> (9, 5, -1, 1, 9); (1, 0) -> (2, 5, 1, 1, 2);
(2, 0) -> (9, 5, 1, 1, 9); (0, 1) -> (3, 5, 1, 1, 3).
Scores, seed 3, environments 0..63, the first episodes of each (64,000 episodes; track_action 512):
  uniform random               mean return 0.253, std 0.530, lengths 24 to 126, mean 28.1
  always stay                  mean return 0.289, std 0.982, lengths 24 to 114, mean 28.4
  track_action                 mean return 29.59, std 0.49, every episode 500 steps (no life is ever lost)
  uniform random, single_life  mean return 0.087, std 0.310, lengths 8 to 74, mean 9.4
"""
import numpy as np

from .environment import BaseEnvironment
from .synthetic import lowbias32_int, synth_key

CELLS = 14                 # board cells per side
CELL = 6                   # pixels per cell side
NUM_ACTIONS = 3
LIVES = 3
MAX_STEPS = 500
BRICK_ROW0, BRICK_ROWS = 2, 3          # the bricks' first board row, and how many rows of them
FULL_ROW = 0x3FFF
SERVE_ROW = 5
BALL, PADDLE, BRICK = 255, 128, 64     # pixel values
STATE_WORDS = 12           # int32 words of a device state record: the 11 state words, then padding


def serve(seed, env, state, s):
    """The state with the ball served for the s-th time in its episode, over the paddle where it stands."""
    bx, by, dx, dy, px, lives, steps, k, r0, r1, r2 = state
    h = synth_key(seed, env, k)
    dx = 1 if lowbias32_int(h ^ (0xB41C0002 + 16 * s)) & 1 else -1
    return (px, SERVE_ROW, dx, 1, px, lives, steps, k, r0, r1, r2)


def start_state(seed, env, k):
    """-> the state episode k of global environment env starts from."""
    px = lowbias32_int(synth_key(seed, env, k) ^ 0xB41C0001) % (CELLS - 1)
    return serve(seed, env, (0, 0, 0, 0, px, LIVES, 0, k, FULL_ROW, FULL_ROW, FULL_ROW), 0)


def step_state(seed, env, state, a, single_life=False):
    """One step of `state` under action a -> (state, reward, terminal).  The state returned is the one the next step starts
    from: after a terminal step that is the start state of episode k + 1 (the device record's rule)."""
    return step_state_truncated(seed, env, state, a, single_life)[:3]


def step_state_truncated(seed, env, state, a, single_life=False):
    """step_state with the reason of a terminal step -> (state, reward, terminal, truncated): truncated = the step is terminal
    only because steps reached MAX_STEPS."""
    bx, by, dx, dy, px, lives, steps, k, r0, r1, r2 = state
    rows = [r0, r1, r2]
    if a == 1:
        px = max(px - 1, 0)
    elif a == 2:
        px = min(px + 1, CELLS - 2)
    nx = bx + dx
    if nx < 0 or nx > CELLS - 1:
        dx = -dx
        nx = bx
    ny = by + dy
    reward, terminal, lost = 0.0, False, False
    if ny < 0:
        dy, ny = 1, by
    elif BRICK_ROW0 <= ny < BRICK_ROW0 + BRICK_ROWS and (rows[ny - BRICK_ROW0] >> nx) & 1:
        rows[ny - BRICK_ROW0] &= ~(1 << nx)
        reward = 1.0
        dy = -dy
        nx, ny = bx, by
    elif ny == CELLS - 1:
        if nx == px or nx == px + 1:
            dy, dx, ny = -1, (-1 if nx == px else 1), by
            if rows == [0, 0, 0]:
                rows = [FULL_ROW] * BRICK_ROWS
        else:
            lives -= 1
            lost = True
            terminal = lives == 0 or bool(single_life)
    steps += 1
    truncated = not terminal and steps == MAX_STEPS
    terminal = terminal or steps == MAX_STEPS
    if terminal:
        return start_state(seed, env, k + 1), reward, True, truncated
    state = (nx, ny, dx, dy, px, lives, steps, k, rows[0], rows[1], rows[2])
    if lost:
        state = serve(seed, env, state, LIVES - lives)
    return state, reward, False, False


def plane(state):
    bx, by, px = state[0], state[1], state[4]
    out = np.zeros((84, 84), dtype=np.uint8)
    for r in range(BRICK_ROWS):
        for c in range(CELLS):
            if (state[8 + r] >> c) & 1:
                out[(BRICK_ROW0 + r) * CELL:(BRICK_ROW0 + r + 1) * CELL, c * CELL:(c + 1) * CELL] = BRICK
    out[(CELLS - 1) * CELL:, px * CELL:(px + 2) * CELL] = PADDLE
    out[by * CELL:(by + 1) * CELL, bx * CELL:(bx + 1) * CELL] = BALL
    return out


def landing_column(state):
    """The column in which the ball of `state` reaches row 13 when it is run forward by the rules with no paddle."""
    bx, by, dx, dy = state[:4]
    rows = list(state[8:11])
    while True:
        nx = bx + dx
        if nx < 0 or nx > CELLS - 1:
            dx = -dx
            nx = bx
        ny = by + dy
        if ny < 0:
            dy, ny = 1, by
        elif BRICK_ROW0 <= ny < BRICK_ROW0 + BRICK_ROWS and (rows[ny - BRICK_ROW0] >> nx) & 1:
            rows[ny - BRICK_ROW0] &= ~(1 << nx)
            dy = -dy
            nx, ny = bx, by
        elif ny == CELLS - 1:
            return nx
        bx, by = nx, ny


def track_action(state):
    """Reference policy: move the paddle towards the column the ball will come down in; stay when the paddle covers it."""
    target, px = landing_column(state), state[4]
    return 1 if target < px else (2 if target > px + 1 else 0)


class BricksEnvironment(BaseEnvironment):
    def __init__(self, actor_id, seed=0, single_life=False):
        self.actor_id = int(actor_id)
        self.num_actions = NUM_ACTIONS
        self.seed = int(seed)
        self.single_life = bool(single_life)
        self.state = start_state(self.seed, self.actor_id, 0)
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.last_step_truncated = False       # the last next() ended its episode at the step cap alone (runners.py reads it)

    @property
    def k(self):
        return self.state[7]

    def state_words(self):
        """The device twin's state record of this environment (int32 [STATE_WORDS])."""
        return np.array(list(self.state) + [0] * (STATE_WORDS - len(self.state)), dtype=np.int32)

    def get_initial_state(self):
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack)

    def next(self, action):
        a = int(np.argmax(action))
        self.state, reward, terminal, self.last_step_truncated = step_state_truncated(self.seed, self.actor_id, self.state, a,
                                                                                      self.single_life)
        self.stack[..., :3] = self.stack[..., 1:]
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack), reward, terminal

    def get_legal_actions(self):
        return np.arange(self.num_actions)

    def get_noop(self):
        return [1.0, 0.0, 0.0]
