"""Head-to-head matches: two policies play duel boards (paac_amd/duel.py) against each other, scored on the GPU.

This is the SPEC of a match, as evaluation.py is the spec of an evaluation; the same numbers are produced
  * on the host by the plain-numpy functions below (`match_actions`, `replay_match`, with evaluation.eval_noops / account and
    duel.DuelBoards), and
  * on the device by paac_match_step (csrc/games.hip; include/paac_hip.h has the contract), one step of N rows = N / 2 boards
    per launch, driven by `DeviceMatch`.

Spec
  rows         a match of n boards is 2n rows in duel's layout: row b < n is the bottom player of board b, row b + n the top
               player, each seeing the board from its own side.  The board key is g = env_offset + b
  no-ops       noops_g = evaluation.eval_noops(seed, g, noops), keyed by the BOARD: both rows play action 0 while t < noops_g
  action       evaluation.eval_action's two rules, unchanged, on the row's own probabilities; counter (g, t lo, t hi, stream),
               key the match's seed.  A bottom row draws from EVAL_STREAM_ACTION -- the bottom rows' actions are exactly
               evaluation.eval_action(probs[:n], seed, t, g, greedy) -- and a top row from MATCH_STREAM_TOP: the two players of
               a board never share a random word, and nothing depends on n or on the chunking
  game         duel.step_row / DuelBoards, seeded by the game seed
  accounting   evaluation.account per row with the row's own reward: score[b + n] == -score[b]; length and done are equal for
               both rows of a board
  bound        max_steps = noops + 1000 (duel's longest episode)
  sides        fixed by the board index, so that side and serve asymmetry cancel: X is the bottom player on boards
               [0, ceil(count / 2)) and the top player on the rest; swap_sides reverses this
"""
import numpy as np

from . import duel
from .evaluation import MAX_CHUNK, DeviceDriver, account, eval_action, eval_noops, philox_word0

MATCH_STREAM_TOP = 0x45560003          # csrc/games.hip: kMatchStreamTop
MATCH_KINDS = ("rally", "duel")        # the runs whose agents play this board: 6 actions, the same planes
MAX_EPISODE_STEPS = duel.MAX_STEPS


def sampled_on_stream(probs_f32, seed, step, board_ids, stream):
    """-> int32 [n]: evaluation.eval_action's sampling rule on probs_f32 [n, A] -- the inverse CDF over float32 running sums,
    the first hit keeping the action -- with u from Philox word 0 of counter (g, step lo, step hi, stream), key `seed`.  The
    top players' rule of a match, and the ghosts' of a pooled duel step (paac_amd/duel_pool.py) on its own stream."""
    p = np.asarray(probs_f32, dtype=np.float32)
    n, A = p.shape
    u = (philox_word0(seed, step, board_ids, stream) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    acts = np.full(n, A - 1, dtype=np.int32)
    chosen = np.zeros(n, dtype=bool)
    c = np.zeros(n, dtype=np.float32)
    for j in range(A - 1):                                   # eval_action's running sums
        c = (c + p[:, j]).astype(np.float32)
        hit = (~chosen) & (u < c)
        acts[hit] = j
        chosen |= hit
    return acts


def match_actions(probs_f32, seed, step, board_ids, greedy):
    """-> int32 [2n]: the action of every row of probs_f32 [2n, A] at step `step` (past the boards' no-ops); board_ids [n] are
    the boards' keys g, rows [0, n) their bottom players and rows [n, 2n) their top players."""
    p = np.asarray(probs_f32, dtype=np.float32)
    board_ids = np.asarray(board_ids)
    n = board_ids.shape[0]
    if p.ndim != 2 or p.shape[0] != 2 * n:
        raise ValueError("match_actions: probs %s for %d boards: expected [%d, A]" % (p.shape, n, 2 * n))
    bottom = eval_action(p[:n], seed, step, board_ids, greedy)
    if greedy:
        return np.concatenate([bottom, np.argmax(p[n:], axis=1).astype(np.int32)])
    return np.concatenate([bottom, sampled_on_stream(p[n:], seed, step, board_ids, MATCH_STREAM_TOP)])


def replay_match(game_seed, env_offset, actions_trace, noops):
    """Steps DuelBoards through a recorded [steps, 2n] action trace under the accounting rule (the no-op wherever t < noops_b,
    whatever the trace holds) -> (scores float32 [2n], lengths int32 [2n]).  noops: the per-board counts [n] (or one for all)."""
    trace = np.asarray(actions_trace)
    steps, rows = trace.shape
    n = rows // 2
    noops = np.tile(np.broadcast_to(np.asarray(noops, dtype=np.int64), (n,)), 2)
    boards = duel.DuelBoards(rows, seed=game_seed, env_offset=env_offset)
    boards.reset()
    rewards, terminals = np.zeros((steps, rows), dtype=np.float32), np.zeros((steps, rows), dtype=bool)
    for t in range(steps):
        _, _, rewards[t], terminals[t], _ = boards.step(np.where(t < noops, 0, trace[t]))
    score, length, _ = account(rewards, terminals, noops)
    return score, length


def x_is_bottom(count, swap_sides=False):
    """-> bool [count]: the boards on which player X is the bottom player."""
    count = int(count)
    first = np.arange(count) < (count + 1) // 2
    return ~first if swap_sides else first


def legs(count, chunk, swap_sides=False):
    """The chunks a match of `count` boards is played in -> [(env_offset, boards, X is bottom), ...]: two legs, one per side
    of X, each in chunks of at most `chunk` boards; board b is board b in any chunking."""
    count, chunk = int(count), int(chunk)
    half = (count + 1) // 2
    out = []
    for lo, hi, bottom in ((0, half, not swap_sides), (half, count, bool(swap_sides))):
        for off in range(lo, hi, chunk):
            out.append((off, min(chunk, hi - off), bottom))
    return out


def check_train_flags(args):
    """Start-up refusals of --eval_match (train.py) -> on?; a Namespace from before the flag: off."""
    boards = getattr(args, "eval_match", 0)
    if isinstance(boards, bool) or int(boards) != boards or not 0 <= int(boards) <= 4096:
        raise ValueError("--eval_match %r: expected a number of boards in [0, 4096] (0 = off)" % (boards,))
    if int(boards) == 0:
        return False
    if int(getattr(args, "eval_every", 0)) <= 0:
        raise ValueError("--eval_match %d plays its boards at the evaluations: it needs --eval_every STEPS" % int(boards))
    if getattr(args, "emulator", "synthetic") != "duel":
        raise ValueError("--eval_match plays the live weights against an earlier copy of themselves on the duel board: it needs "
                         "--emulator duel (got '%s')" % getattr(args, "emulator", "synthetic"))
    return True


class DeviceMatch(DeviceDriver):
    """Plays `count` duel boards, one scored episode each, between player X (params_x through ctx_x) and player Y -- nothing
    crosses to the host but one int32 per block of steps.

    params_*: flat float32 parameter tensors, read at every run().  ctx_*: a hip_ops.Context of that player's geometry that
    the match may use freely (its acting forwards only); the same unmanaged context may serve both players when their
    geometries agree -- its forwards repack what they are handed.  seed: the match's own (no-ops and sampled actions);
    game_seed: the boards'.  Each leg (a side of X) is played in chunks of at most min(ctx.max_batch, MAX_CHUNK) boards,
    env_offset advancing.  steps_per_launch: steps per block (made even: the ping-pong closes), one hipGraph per (chunk size,
    offset, leg) when use_graph; record=True runs eagerly and keeps the action trace.

    run(): X's scores and lengths; the trace's column b is the bottom player of board b, column count + b its top player."""

    rows_per_board = 2

    def __init__(self, params_x, ctx_x, params_y, ctx_y, count, noops=30, greedy=False, seed=0, game_seed=0, steps_per_launch=16,
                 record=False, use_graph=True, stream=None, swap_sides=False):
        from . import hip_ops
        super(DeviceMatch, self).__init__(hip_ops, count, noops, seed, greedy, steps_per_launch, record, use_graph)
        for who, params, ctx in (("X", params_x, ctx_x), ("Y", params_y, ctx_y)):
            if ctx.num_actions != duel.NUM_ACTIONS:
                raise ValueError("player %s: a context of %d actions; the duel board has %d" % (who, ctx.num_actions, duel.NUM_ACTIONS))
            if params.numel() != ctx.layout["total"]:
                raise ValueError("player %s: %d parameters; the context's geometry has %d" % (who, params.numel(), ctx.layout["total"]))
        self.players = ((params_x, ctx_x), (params_y, ctx_y))
        self.game_seed, self.swap_sides = int(game_seed), bool(swap_sides)
        self.max_steps = self.noops + MAX_EPISODE_STEPS
        self._allocate(min(self.count, ctx_x.max_batch, ctx_y.max_batch, MAX_CHUNK), duel.STATE_WORDS, duel.NUM_ACTIONS,
                       params_x.device, stream)

    def _chunks(self):
        return [(n, env_offset, x_bottom) for env_offset, n, x_bottom in legs(self.count, self.chunk, self.swap_sides)]

    def _reset(self, n, env_offset, x_bottom):
        self.hip_ops.duel_reset(self.game_seed, env_offset, self.states[0][:2 * n], self.stacks[0][:2 * n])

    def _block(self, n, env_offset, x_bottom):
        """`block` x [the bottom player's forward, the top player's forward, one match step] on n boards, then the counter."""
        ops = self.hip_ops
        (pb, cb), (pt, ct) = self.players if x_bottom else self.players[::-1]
        for j in range(self.block):
            a, b = j & 1, (j & 1) ^ 1
            cb.forward(pb, self.stacks[a][:n], probs=self.probs[:n])
            ct.forward(pt, self.stacks[a][n:2 * n], probs=self.probs[n:2 * n])
            ops.match_step(self.probs[:2 * n], self.greedy, self.seed, self.noops, self.step, j, self.game_seed, env_offset,
                           self.states[a][:2 * n], self.states[b][:2 * n], self.stacks[a][:2 * n], self.stacks[b][:2 * n],
                           self.actions[j][:2 * n], self.score[:2 * n], self.length[:2 * n], self.done[:2 * n], self.alive)
        ops.counter_add(self.step, self.block)

    def _scored_rows(self, n, env_offset, x_bottom):
        return slice(0, n) if x_bottom else slice(n, 2 * n)

    def _place_trace(self, full, trace, n, env_offset, x_bottom):
        full[:len(trace), env_offset:env_offset + n] = trace[:, :n]
        full[:len(trace), self.count + env_offset:self.count + env_offset + n] = trace[:, n:]

    def summary(self, scores, lengths, seconds):
        """evaluator.summary's fields, of X's scores, plus the fractions of boards X won, drew and lost."""
        scores = np.asarray(scores)
        return dict(count=self.count, greedy=self.greedy, mean=float(np.mean(scores)), min=float(np.min(scores)),
                    max=float(np.max(scores)), std=float(np.std(scores)), mean_length=float(np.mean(lengths)),
                    seconds=float(seconds), wins=float(np.mean(scores > 0)), draws=float(np.mean(scores == 0)),
                    losses=float(np.mean(scores < 0)))
