"""Catch: a learnable game resident on the GPU.  A ball falls, a paddle moves, +1 for a catch and -1 for a miss.

This is the SPEC of the catch environment family; the same numbers are produced
  * on the host by `CatchEnvironment` (a BaseEnvironment plugin, numpy and pure Python), and
  * on the device by paac_catch_reset / paac_catch_step (csrc/catch_dev.h, csrc/games.hip), N envs per launch.
The synthetic family (synthetic.py) measures the hot path, but its reward is a hash: there is nothing to learn.  This one
is stateful and action-dependent, is rendered into the same 84x84x4 uint8 observations and is small enough to be learned in
seconds at the device loop's speed.  Call pattern as SyntheticEnvironment's: get_initial_state() / next(one_hot) ->
(obs, reward, terminal).

Spec (all hashing reuses lowbias32 and key = synth_key(seed, env, id) of synthetic.py unchanged):
  board          14 x 14 cells of 6 x 6 pixels = 84 x 84
  state          per environment, int32: ball column bx in 0..13, ball row by in 0..13, drift dx in {-1, 0, 1}, paddle
                 column px in 0..13 (the paddle lives in row 13), episode index k = the number of episodes this
                 environment has started before the current one
  actions        A = 3: 0 stay, 1 left, 2 right
  episode start  global environment g = env_offset + e, episode index k, h = synth_key(seed, g, k):
                   bx = lowbias32(h ^ 0xC47C0001) % 14
                   px = lowbias32(h ^ 0xC47C0002) % 14
                   dx = lowbias32(h ^ 0xC47C0003) % 3 - 1
                   by = lowbias32(h ^ 0xC47C0004) % 13 if k == 0 else 0
                 (the start row is staggered only in an environment's very first episode, so that environments do not all
                 terminate on the same step)
  step(a)        in this order:
                   1. paddle: a == 1: px = max(px - 1, 0); a == 2: px = min(px + 1, 13)
                   2. ball:   nx = bx + dx; if nx < 0 or nx > 13: dx = -dx, nx = bx + dx; then bx = nx, by += 1
                   3. by == 13: terminal, reward +1.0 if bx == px else -1.0, and the environment starts episode k + 1
                      at once; otherwise reward 0.0, not terminal
                 every episode with k >= 1 lasts exactly 13 steps and can always be won (13 moves cover 13 columns)
  plane(state)   pixel (y, x) = 255 if (y // 6, x // 6) == (by, bx), else 128 if (y // 6, x // 6) == (13, px), else 0
  observation    the synthetic family's rule: the previous stack shifted by one channel with the new plane as channel 3;
                 at construction and after a terminal step it is [0, 0, 0, plane of the new start state] -- the terminal
                 position itself is never shown (the runner calls get_initial_state())
  bookkeeping    as the synthetic family's: reward clipped to [-1, 1] (a no-op here), mask = 0 on terminal, ep_reward /
                 ep_len totals, the finished-episode ring

Anchors, seed 3, (g, k) -> (bx, by, dx, px): (0, 0) -> (1, 12, 0, 8); (1, 0) -> (1, 3, -1, 3); (2, 0) -> (10, 7, 1, 11);
(3, 0) -> (4, 8, 0, 2); (0, 1) -> (4, 0, -1, 0); (1, 1) -> (1, 0, -1, 12).
Mean return over seed 3, 64 environments, episodes 1..79: uniform random -0.862, always stay -0.854, moving towards the
ball's final column +1.000.
"""
import numpy as np

from .environment import BaseEnvironment
from .synthetic import lowbias32_int, synth_key

CELLS = 14                 # board cells per side
CELL = 6                   # pixels per cell side
NUM_ACTIONS = 3
BALL, PADDLE = 255, 128    # pixel values
STATE_WORDS = 8            # int32 words of a device state record: bx, by, dx, px, k, then padding


def start_state(seed, env, k):
    """-> (bx, by, dx, px) of episode k of global environment env."""
    h = synth_key(seed, env, k)
    bx = lowbias32_int(h ^ 0xC47C0001) % CELLS
    px = lowbias32_int(h ^ 0xC47C0002) % CELLS
    dx = lowbias32_int(h ^ 0xC47C0003) % 3 - 1
    by = lowbias32_int(h ^ 0xC47C0004) % (CELLS - 1) if k == 0 else 0
    return bx, by, dx, px


def step_state(state, a):
    """One step of (bx, by, dx, px) under action a -> (state, reward, terminal); the state returned on a terminal step is the
    terminal position (the caller starts the next episode)."""
    bx, by, dx, px = state
    if a == 1:
        px = max(px - 1, 0)
    elif a == 2:
        px = min(px + 1, CELLS - 1)
    nx = bx + dx
    if nx < 0 or nx > CELLS - 1:
        dx = -dx
        nx = bx + dx
    bx, by = nx, by + 1
    if by == CELLS - 1:
        return (bx, by, dx, px), (1.0 if bx == px else -1.0), True
    return (bx, by, dx, px), 0.0, False


def plane(state):
    bx, by, dx, px = state
    out = np.zeros((84, 84), dtype=np.uint8)
    out[(CELLS - 1) * CELL:, px * CELL:(px + 1) * CELL] = PADDLE
    out[by * CELL:(by + 1) * CELL, bx * CELL:(bx + 1) * CELL] = BALL
    return out


class CatchEnvironment(BaseEnvironment):
    def __init__(self, actor_id, seed=0):
        self.actor_id = int(actor_id)
        self.num_actions = NUM_ACTIONS
        self.seed = int(seed)
        self.k = 0
        self.state = start_state(self.seed, self.actor_id, 0)
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)

    def state_words(self):
        """The device twin's state record of this environment (int32 [STATE_WORDS])."""
        return np.array(list(self.state) + [self.k] + [0] * (STATE_WORDS - 5), dtype=np.int32)

    def get_initial_state(self):
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack)

    def next(self, action):
        a = int(np.argmax(action))
        self.state, reward, terminal = step_state(self.state, a)
        if terminal:
            self.k += 1
            self.state = start_state(self.seed, self.actor_id, self.k)
        self.stack[..., :3] = self.stack[..., 1:]
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack), reward, terminal

    def get_legal_actions(self):
        return np.arange(self.num_actions)

    def get_noop(self):
        return [1.0, 0.0, 0.0]
