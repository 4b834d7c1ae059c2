"""Duel against a pool of past selves: `--emulator duel --duel_pool K` trains every row against a frozen earlier copy of the
policy instead of against the live weights (fictitious self-play: pure mirror play always meets its own newest habits).

This is the SPEC of the pooled step and of the pool's schedule; the same numbers are produced
  * on the host by the plain-numpy functions and the twin `PooledBoards` below (on top of duel.py, match.py and
    evaluation.philox_word0), and
  * on the device by paac_duel_ghost_reset / paac_duel_ghost_step (csrc/games.hip: ghost_step_kernel; include/paac_hip.h has
    the contract), N boards per launch, driven by paac.DeviceRollout with the tensors of `DevicePool`.

Spec
  rows         -ec rows are -ec BOARDS.  Learner row b is the bottom player of board b (a duel row always sees itself at the
               bottom, and the first serve alternates per episode: no asymmetry); the top player of board b is a GHOST, a row
               of the frozen opponent, with an observation stack of its own -- what duel's top rows see -- and no rollout
               records.  The update sees N = -ec rows exactly as a rally run does
  step         one pooled step of N boards is duel.DuelBoards(2N, seed, env_offset).step(concat(a_learner, a_ghost)): rows
               [0, N) give the learner's records, observations, rewards, terminals and truncation flags, rows [N, 2N) the
               ghosts' observations.  Reset is DuelBoards(2N).reset(), split the same way.  The board key is g = env_offset + b
  ghost action always sampled: evaluation.eval_action's inverse-CDF rule on the ghost's own probability row, the float32
               running sums of match.match_actions' top rule (match.sampled_on_stream: one body), on the Philox counter
               {g, t lo, t hi, GHOST_STREAM}, key --sampler_seed; t = the rollout's device tick plus the step's offset in the
               cycle.  The learner's action is whatever the run's sampler (philox or numpy) wrote, as in any run
  pool         up to K frozen copies of the weights in slots [0, K), each tagged with the global step it was taken at.  It
               starts with one member, the weights the run started or resumed from, in slot (start // STEPS) % K -- slot 0
               for a fresh run -- which is also the first opponent
  events       event j = 1, 2, ... happens at the first chunk boundary of the training loop at or after global step
               j * STEPS (the loop caps its chunk with an until_pool as it does with until_eval: `event_step`); a boundary that
               has passed several multiples at once runs the one event of the largest j.  At an event
                 1. the live weights are written to slot j % K (the pool grows until every slot is taken);
                 2. the next opponent is drawn with u = (philox_word0(random_seed, j, 0, POOL_STREAM_LATEST) >> 8) / 2^24:
                    u < P: the slot just written; otherwise the occupied slot of index philox_word0(random_seed, j, 0,
                    POOL_STREAM_SLOT) % size, counted in slot order (a fresh run's occupied slots are [0, size): the slot
                    itself)
  not saved    the pool is not checkpointed: a resumed run starts a fresh pool from the restored weights
The defaults (STEPS = 102400, P = 0.5) are design choices, not measured optima.
"""
import math

import numpy as np

from . import duel
from .evaluation import philox_word0
from .match import sampled_on_stream

GHOST_STREAM = 0x44500001              # csrc/games.hip: kGhostStream
POOL_STREAM_LATEST = 0x44500002        # the schedule's two streams (host only)
POOL_STREAM_SLOT = 0x44500003
MAX_POOL = 16


def ghost_actions(probs_f32, sampler_seed, tick, board_ids):
    """-> int32 [n]: the ghosts' actions on their probability rows probs_f32 [n, A] at device tick `tick`; board_ids [n] are
    the boards' keys g."""
    p = np.asarray(probs_f32, dtype=np.float32)
    board_ids = np.asarray(board_ids)
    if p.ndim != 2 or p.shape[0] != board_ids.shape[0]:
        raise ValueError("ghost_actions: probs %s for %d boards" % (p.shape, board_ids.shape[0]))
    return sampled_on_stream(p, sampler_seed, tick, board_ids, GHOST_STREAM)


class PooledBoards(object):
    """The numpy twin of paac_duel_ghost_reset / paac_duel_ghost_step: n boards = DuelBoards(2n), split.
    reset() -> (records int32 [n, STATE_WORDS], stacks uint8 [n, 84, 84, 4], ghost_stacks uint8 [n, 84, 84, 4]);
    step(a_learner [n], a_ghost [n]) -> (records, stacks, ghost_stacks, rewards float32 [n], terminals bool [n],
    truncated bool [n]) -- the records, rewards and flags are the learner's (bottom) rows'."""

    def __init__(self, n_boards, seed, env_offset=0):
        if int(n_boards) < 1:
            raise ValueError("PooledBoards: %r boards: expected at least 1" % (n_boards,))
        self.n = int(n_boards)
        self.boards = duel.DuelBoards(2 * self.n, seed, env_offset)

    def reset(self):
        records, stacks = self.boards.reset()
        return records[:self.n], stacks[:self.n], stacks[self.n:]

    def step(self, a_learner, a_ghost):
        a_learner, a_ghost = np.asarray(a_learner).reshape(-1), np.asarray(a_ghost).reshape(-1)
        if a_learner.shape[0] != self.n or a_ghost.shape[0] != self.n:
            raise ValueError("PooledBoards.step: %d + %d actions for %d boards" % (a_learner.shape[0], a_ghost.shape[0], self.n))
        records, stacks, rewards, terminals, truncated = self.boards.step(np.concatenate([a_learner, a_ghost]))
        n = self.n
        return records[:n], stacks[:n], stacks[n:], rewards[:n], terminals[:n], truncated[:n]


# -- the pool's schedule: pure functions ---------------------------------------------------------------------------------------
def event_step(start, steps_per_cycle, j, every):
    """The global step event j happens at in a run that starts at `start` and advances by steps_per_cycle per cycle: the first
    cycle boundary at or after j * every -- exactly j * every when the boundaries hit it.  (Chunks end there: until_pool.)"""
    start, spc = int(start), int(steps_per_cycle)
    return start + max(0, -(-(int(j) * int(every) - start) // spc)) * spc


def until_pool(next_event, global_step, steps_per_cycle):
    """Cycles from global_step to the first boundary at or after next_event (at least 1): the loop's chunk is capped by it."""
    return max(1, -(-(int(next_event) - int(global_step)) // int(steps_per_cycle)))


def draw_opponent(random_seed, j, latest_p, slot, occupied):
    """Event j has written `slot`; `occupied`: the occupied slots in slot order (slot among them) -> (opponent slot, latest?)."""
    u = float(philox_word0(random_seed, j, 0, POOL_STREAM_LATEST) >> np.uint32(8)) / 16777216.0
    if u < float(latest_p):
        return int(slot), True
    return int(occupied[int(philox_word0(random_seed, j, 0, POOL_STREAM_SLOT)) % len(occupied)]), False


class PoolSchedule(object):
    """Which slot holds what and who plays next -- host integers only; DevicePool moves the weights accordingly.
    tags[slot]: the global step the slot's weights were taken at (None: empty)."""

    def __init__(self, K, every, latest_p, random_seed, start_step=0):
        self.K, self.every, self.latest_p, self.random_seed = int(K), int(every), float(latest_p), int(random_seed)
        j0 = int(start_step) // self.every
        self.tags = [None] * self.K
        self.tags[j0 % self.K] = int(start_step)
        self.opponent_slot = j0 % self.K
        self.next_event = (j0 + 1) * self.every

    @property
    def size(self):
        return sum(t is not None for t in self.tags)

    def due(self, global_step):
        return int(global_step) >= self.next_event

    def event(self, global_step):
        """The event at a boundary with due(global_step) -> the `duel_pool` record (metrics.jsonl)."""
        global_step = int(global_step)
        j = global_step // self.every
        slot = j % self.K
        self.tags[slot] = global_step
        occupied = [s for s, t in enumerate(self.tags) if t is not None]
        self.opponent_slot, latest = draw_opponent(self.random_seed, j, self.latest_p, slot, occupied)
        self.next_event = (j + 1) * self.every
        return dict(global_step=global_step, event=j, slot=slot, size=len(occupied), opponent_slot=self.opponent_slot,
                    opponent_global_step=self.tags[self.opponent_slot], latest=bool(latest))


def schedule(start, steps_per_cycle, max_global_steps, K, every, latest_p, random_seed):
    """The `duel_pool` records of a whole run, as the training loop writes them (the chunking enters through event_step
    alone: every chunk ends at a cycle boundary, and until_pool ends one at the first boundary at or after each multiple)."""
    sched = PoolSchedule(K, every, latest_p, random_seed, start)
    spc = int(steps_per_cycle)
    end = int(start) + max(0, -(-(int(max_global_steps) - int(start)) // spc)) * spc
    out = []
    while True:
        at = event_step(start, spc, sched.next_event // sched.every, sched.every)
        if at > end:
            return out
        out.append(sched.event(at))


def check_train_flags(args, world=1):
    """Start-up refusals of --duel_pool / --duel_pool_every / --duel_pool_latest_p (train.py), before the GPU is touched -> K
    (0: off); a Namespace from before the flags: off.  K = 0 ignores the other two flags."""
    K = getattr(args, "duel_pool", 0)
    if isinstance(K, bool) or not isinstance(K, (int, float, np.integer, np.floating)) or int(K) != K or not 0 <= int(K) <= MAX_POOL:
        raise ValueError("--duel_pool %r: expected an integer in [0, %d] (0 = off): the frozen copies of the weights the pool "
                         "holds" % (K, MAX_POOL))
    K = int(K)
    if K == 0:
        return 0
    every = getattr(args, "duel_pool_every", 102400)
    if isinstance(every, bool) or int(every) != every or int(every) <= 0:
        raise ValueError("--duel_pool_every %r: expected a positive number of global steps between pool events" % (every,))
    p = getattr(args, "duel_pool_latest_p", 0.5)
    if isinstance(p, bool) or not math.isfinite(float(p)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError("--duel_pool_latest_p %r: expected a probability in [0, 1]" % (p,))
    if getattr(args, "emulator", "synthetic") != "duel":
        raise ValueError("--duel_pool %d plays duel boards against frozen copies of the learner: it needs --emulator duel (got "
                         "'%s')" % (K, getattr(args, "emulator", "synthetic")))
    if int(world) > 1:
        raise ValueError("--duel_pool %d with %d data-parallel ranks: the pool is rank-local and would work unchanged, but it is "
                         "not built into the data-parallel loop yet: run --duel_pool on one GPU" % (K, int(world)))
    return K


class DevicePool(object):
    """The pool's device side: the pool tensor [K, total], the opponent's parameter tensor -- a fixed address, the captured
    cycles read it -- and a second context of the run's architecture for the ghost forwards, in MANAGED mode: its packed
    weights are refreshed once per opponent change (pack_weights), so a ghost forward inside a cycle carries no repack launch.
    The ghost forward runs on this context alone: the learner's context, its kept-forward state included, is never touched."""

    def __init__(self, params, arch_id, num_actions, n_boards, K, every, latest_p, random_seed, start_step, device_index=0):
        import torch
        from . import hip_ops
        self.schedule = PoolSchedule(K, every, latest_p, random_seed, start_step)
        self.pool = torch.zeros((int(K), params.numel()), dtype=torch.float32, device=params.device)
        self.pool[self.schedule.opponent_slot].copy_(params)
        self.opponent = params.clone()
        self.ctx = hip_ops.Context(arch_id, num_actions, max_batch=int(n_boards), device_index=device_index)
        self.ctx.set_managed_weights(True)
        self.ctx.pack_weights(self.opponent)

    def set_opponent(self, params):
        """Overwrites the opponent's weights in place (on the current stream) and repacks them."""
        self.opponent.copy_(params)
        self.ctx.pack_weights(self.opponent)

    def event(self, global_step, live_params):
        """A pool event on the current stream: the live weights into their slot, the drawn slot into the opponent tensor, the
        repack.  Device-to-device copies and one launch: no host synchronisation.  -> the `duel_pool` record."""
        record = self.schedule.event(global_step)
        self.pool[record["slot"]].copy_(live_params)
        self.set_opponent(self.pool[record["opponent_slot"]])
        return record

    def close(self):
        self.ctx.close()
