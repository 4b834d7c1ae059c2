"""Duel: rally played against the learner itself.  N rows = N / 2 boards of the rally board (rally.py); the same network plays both
paddles, each row seeing the board from its own side.  To the learner it is a device game with N rows and 6 actions.

This is the SPEC of the duel environment family; the same numbers are produced
  * on the host by the reference functions below and the numpy batch twin `DuelBoards`, and
  * on the device by paac_duel_reset / paac_duel_step (csrc/duel_dev.h, csrc/games.hip), N rows per launch.
There is no BaseEnvironment plugin: the host loop steps environments one by one in worker processes, and a row here needs its
partner's action.  `--emulator duel` runs on the device loop only; what `paac_amd.test` steps on the host for a duel run is
rally.RallyEnvironment -- the scripted opponent is the yardstick a duel policy is scored against.

Spec (board, constants, hashes, serves, pixels and bookkeeping are rally's, unchanged):
  rows           HALF = N // 2.  Row e < HALF is the bottom player of board b = e; row e >= HALF the top player of board
                 b = e - HALF.  The partner of row e is (e + HALF) % N.  The board's hash key uses g = env_offset + b (rally:
                 env_offset + e)
  board state    rally's 10 words (bx, by, dx, dy, px, ox, mine, theirs, steps, k) in the BOTTOM player's frame: px / mine are
                 the bottom player's, ox / theirs the top player's
  mirror(s)      (bx, 13 - by, dx, -dy, ox, px, theirs, mine, steps, k): the board as the other player sees it.  An involution;
                 a vertical flip only -- columns are not flipped, LEFT / RIGHT mean the same for both players
  start_board    (seed, g, k): k even: rally.start_state(seed, g, k); k odd: the same state with serve 0 re-dealt towards the
                 top player.  Who receives first alternates from episode to episode
  step_board     (seed, g, s, a_bottom, a_top) -> (s', reward_bottom, terminal, truncated): rally.step_state_truncated with its
                 rule 2, the scripted opponent, replaced by a second paddle move: a_top in (2, 4): ox = min(ox + 1, 12); a_top in
                 (3, 5): ox = max(ox - 1, 0).  Rules 1 and 3..6, POINTS, MAX_STEPS, the serves and the truncation rule are
                 rally's; a terminal step returns start_board(seed, g, k + 1)
  row records    12 int32, rally's layout: a bottom row holds the board state, a top row mirror(board state)
  a row's step   un-mirror the record if the row is top; step_board with (actions[bottom row], actions[top row]); re-mirror if
                 the row is top.  reward = reward_bottom for bottom, 0 - reward_bottom for top (a zero reward is +0.0 on both
                 rows); terminal and truncated are the same for both.  Both rows of a board compute the same board step; no row
                 writes anything another row reads.  Invariant: record[b + HALF] == mirror(record[b]) after reset and after
                 every step
  plane          rally.plane(the row's own record): own paddle 128 in the bottom row, the other's 64 in the top row, ball 255.
                 A top row's plane is the bottom row's flipped vertically with 128 and 64 exchanged: a network trained here is
                 directly a rally agent.  History push and the fresh stack after a terminal step are rally's
  bookkeeping    rally's, per row: ep_reward, ep_len and the finished ring get both players' episodes -- the mean logged return
                 is 0 by construction; --eval_every scores the policy against rally's scripted opponent instead
-g, --single_life_episodes, --synthetic_terminal_p and --random_start do not apply.

Anchors, seed 3, (g, k) -> (bx, by, dx, dy, px, ox): (0, 0) -> (5, 6, -1, 1, 12, 3); (1, 0) -> (3, 6, -1, 1, 8, 0);
(0, 1) -> (8, 7, -1, -1, 0, 5).
With a_top = scripted_top_action(seed, g, s), step_board is rally's step: same reward, terminal and truncated flags, the same
state after a non-terminal step (tests/test_duel.py).
"""
import numpy as np

from . import rally
from .rally import CELLS, LEFT, LEFTFIRE, MAX_STEPS, NOOP, POINTS, RIGHT, RIGHTFIRE

NUM_ACTIONS = rally.NUM_ACTIONS
STATE_WORDS = rally.STATE_WORDS


def mirror(s):
    """The board state as the other player sees it."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = s
    return (bx, CELLS - 1 - by, dx, -dy, ox, px, theirs, mine, steps, k)


def start_board(seed, g, k):
    """-> the state episode k of board g starts from (the bottom player's frame)."""
    state = rally.start_state(seed, g, k)
    return state if k % 2 == 0 else rally.serve(seed, g, state, 0, False)


def step_board(seed, g, s, a_bottom, a_top):
    """One step of board state s under the two players' actions -> (state, reward_bottom, terminal, truncated).  The state
    returned is the one the next step starts from: after a terminal step the start state of episode k + 1."""
    bx, by, dx, dy, px, ox, mine, theirs, steps, k = s
    if a_bottom in (RIGHT, RIGHTFIRE):
        px = min(px + 1, CELLS - 2)
    elif a_bottom in (LEFT, LEFTFIRE):
        px = max(px - 1, 0)
    if a_top in (RIGHT, RIGHTFIRE):
        ox = min(ox + 1, CELLS - 2)
    elif a_top in (LEFT, LEFTFIRE):
        ox = max(ox - 1, 0)
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
        return start_board(seed, g, k + 1), reward, True, not decided
    state = (nx, ny, dx, dy, px, ox, mine, theirs, steps, k)
    if reward != 0.0:
        state = rally.serve(seed, g, state, mine + theirs, reward < 0.0)
    return state, reward, False, False


def scripted_top_action(seed, g, s):
    """Rally's scripted opponent expressed as the top player's action on board state s: NOOP, LEFT or RIGHT."""
    if not rally.opponent_moves(seed, g, s):
        return NOOP
    bx, by, dx, ox = s[0], s[1], s[2], s[5]
    tx = rally.entry_column(bx, dx, by)[0]
    return LEFT if tx < ox else (RIGHT if tx > ox + 1 else NOOP)


def step_row(seed, g, record, top, a_own, a_partner):
    """One step of a ROW: `record` is the row's own 10-word state (mirrored if the row is top), a_own its action, a_partner
    the other player's -> (record, reward, terminal, truncated) in the row's own frame."""
    board = mirror(record) if top else record
    a_bottom, a_top = (a_partner, a_own) if top else (a_own, a_partner)
    board, reward, terminal, truncated = step_board(seed, g, board, a_bottom, a_top)
    if top:
        return mirror(board), 0 - reward, terminal, truncated
    return board, reward, terminal, truncated


class DuelBoards(object):
    """The numpy batch twin of paac_duel_reset / paac_duel_step: n_rows rows = n_rows // 2 boards.  Every row is stepped on
    its own from its own record and the two actions, as a workgroup of the kernel does.
    reset() -> (records int32 [N, STATE_WORDS], stacks uint8 [N, 84, 84, 4]);
    step(actions [N]) -> (records, stacks, rewards float32 [N], terminals bool [N], truncated bool [N])."""

    def __init__(self, n_rows, seed, env_offset=0):
        if int(n_rows) < 2 or int(n_rows) % 2:
            raise ValueError("DuelBoards: %r rows: expected an even number >= 2 (two rows per board)" % (n_rows,))
        self.n_rows, self.half = int(n_rows), int(n_rows) // 2
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.rows = None
        self.stacks = None

    def _top(self, e):
        return e >= self.half

    def _key(self, e):
        return self.env_offset + (e - self.half if self._top(e) else e)

    def records(self):
        out = np.zeros((self.n_rows, STATE_WORDS), dtype=np.int32)
        out[:, :10] = np.asarray(self.rows, dtype=np.int32)
        return out

    def reset(self):
        self.rows = []
        for e in range(self.n_rows):
            board = start_board(self.seed, self._key(e), 0)
            self.rows.append(mirror(board) if self._top(e) else board)
        self.stacks = np.zeros((self.n_rows, 84, 84, 4), dtype=np.uint8)
        for e, row in enumerate(self.rows):
            self.stacks[e, ..., 3] = rally.plane(row)
        return self.records(), self.stacks.copy()

    def step(self, actions):
        actions = [int(a) for a in np.asarray(actions).reshape(-1)]
        if len(actions) != self.n_rows:
            raise ValueError("DuelBoards.step: %d actions for %d rows" % (len(actions), self.n_rows))
        rewards = np.zeros(self.n_rows, dtype=np.float32)
        terminals, truncated = np.zeros(self.n_rows, dtype=bool), np.zeros(self.n_rows, dtype=bool)
        rows = []
        for e, row in enumerate(self.rows):
            partner = (e + self.half) % self.n_rows
            row, rewards[e], terminals[e], truncated[e] = step_row(self.seed, self._key(e), row, self._top(e), actions[e],
                                                                   actions[partner])
            rows.append(row)
            if terminals[e]:
                self.stacks[e] = 0
            else:
                self.stacks[e, ..., :3] = self.stacks[e, ..., 1:]
            self.stacks[e, ..., 3] = rally.plane(row)
        self.rows = rows
        return self.records(), self.stacks.copy(), rewards, terminals, truncated
