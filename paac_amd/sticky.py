"""Sticky actions for the device games (--sticky_action_p P; Machado et al., arXiv 1709.06009): at every step, with probability
P, the environment executes the action it executed on its previous step instead of the one the agent chose.

This is the SPEC of the rule, as evaluation.py is the spec of an evaluation; the same numbers are produced
  * on the host by the plain-numpy functions below (`sticks`, `apply`) and by `StickyEnvironment`, a wrapper of any host twin, and
  * on the device by the sticky forms of game_step_kernel and eval_step_kernel (csrc/games.hip; include/paac_hip.h has the
    contract: paac_sticky, paac_game_step_sticky, paac_duel_step_sticky, paac_eval_step_sticky).

Spec
  draw         u = the 24 high bits of word 0 of philox4x32-10 on counter (g, step lo, step hi, stream), key (seed lo, seed hi),
               times 2^-24, as a float32; the step STICKS iff u < float32(P).  P = 0 never sticks.
  training     stream STICKY_STREAM, seed = the environment seed (env_spec["seed"]), g = env_offset + e -- for duel per ROW,
               g = env_offset + row: the two players of a board stick independently -- and step = the number of game steps
               environment g has taken in this run: *tick + t in the device loop, the wrapper's own count of next() calls in
               the host loop
  evaluation   stream EVAL_STREAM_STICKY, seed = the evaluation's seed, step = the evaluation step t, no-op steps included
  streams      neither constant is a stream in use: 0 (the rollout sampler), 0x504D0000 + epoch (the minibatch shuffles),
               0x45560001..3 (evaluation actions, no-ops, the match's top player), 0x44500001 and 0x44500003 (the duel pool)
  executed     executed = prev if the step sticks else chosen; prev = the action EXECUTED on the environment's previous step,
               0 (every game's no-op) at the first step of a run and at the first step after a terminal step.  During an
               evaluation's no-op steps chosen = 0, so executed = 0
  learner      only the CHOSEN action goes into the rollout's `actions` plane: the agent is not told, as in ALE.  Returns,
               update, samplers and the finished-episode ring are untouched, so the flag works with every update option
  left out     the ghost step of --duel_pool and the match step of --eval_match / --versus have no sticky form: the flag is
               refused beside them (check_flags)
"""
import logging
import math

import numpy as np

from .environment import BaseEnvironment
from .evaluation import philox_word0

STICKY_STREAM = 0x53544B01             # csrc/games.hip: kStickyStream
EVAL_STREAM_STICKY = 0x45560004        # csrc/games.hip: kEvalStreamSticky


def sticks(p, seed, step, env_ids, stream):
    """-> bool per environment: whether the step `step` of environments `env_ids` sticks."""
    u = (philox_word0(seed, step, env_ids, stream) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u < np.float32(p)


def apply(chosen, prev, step, env_ids, p, seed, stream):
    """One step of the rule on int32 [N] arrays -> (executed, new_prev): executed = prev where the draw sticks, else chosen;
    new_prev = executed (the caller zeroes it where the step turned out terminal)."""
    chosen, prev = np.asarray(chosen, dtype=np.int32), np.asarray(prev, dtype=np.int32)
    executed = np.where(sticks(p, seed, step, env_ids, stream), prev, chosen).astype(np.int32)
    return executed, executed.copy()


def check_p(p, what="sticky_action_p"):
    """P as a float in [0, 1), or a ValueError."""
    try:
        value = float(p)
    except (TypeError, ValueError):
        raise ValueError("%s %r: expected a probability in [0, 1)" % (what, p))
    if isinstance(p, bool) or not math.isfinite(value) or not 0.0 <= value < 1.0:
        raise ValueError("%s %r: expected a finite probability in [0, 1)" % (what, p))
    return value


def flag_of(args):
    """args.sticky_action_p; a Namespace without the field (an args.json from before the flag): 0."""
    return float(getattr(args, "sticky_action_p", 0.0) or 0.0)


def check_flags(args, versus=None):
    """Start-up refusals of --sticky_action_p (train.py, test.py) -> P.  versus: paac_amd.test's --versus folder."""
    p = check_p(getattr(args, "sticky_action_p", 0.0) or 0.0)
    if p > 0.0:
        if int(getattr(args, "duel_pool", 0) or 0) > 0:
            raise ValueError("--sticky_action_p %g cannot be combined with --duel_pool: the pooled (ghost) step has no sticky form"
                             % p)
        if int(getattr(args, "eval_match", 0) or 0) > 0:
            raise ValueError("--sticky_action_p %g cannot be combined with --eval_match: the match step has no sticky form" % p)
        if versus is not None:
            raise ValueError("--sticky_action_p %g cannot be combined with --versus: the match step has no sticky form" % p)
        if getattr(args, "emulator", "synthetic") == "synthetic":
            logging.info("--sticky_action_p %g is without effect for --emulator synthetic: the synthetic reward is a hash of the "
                         "step, not of what the environment executes", p)
    return p


class StickyEnvironment(BaseEnvironment):
    """Any host twin under the rule: environment `g` of a run keyed by (seed, stream).  next() replaces the one-hot action by
    the previously executed one where the draw sticks; the step of a draw is this wrapper's own count of next() calls."""

    def __init__(self, env, p, seed, g, stream=STICKY_STREAM):
        self.env = env
        # (names of their own: the twin's `seed`, `state`, `actor_id` ... stay reachable through the wrapper)
        self.sticky_p, self.sticky_seed, self.sticky_g, self.sticky_stream = check_p(p), int(seed), int(g), int(stream)
        self.prev = 0
        self.sticky_steps = 0                     # next() calls so far: the draw's step
        self.last_executed = 0             # (what the last next() executed: read by the tests)

    @property
    def num_actions(self):
        return self.env.num_actions

    # (last_step_truncated goes through __getattr__ below: a twin without it -- catch -- stays without it, which is what
    # --bootstrap_truncated asks the host environments)
    @property
    def on_new_frame(self):
        return self.env.on_new_frame

    @on_new_frame.setter
    def on_new_frame(self, hook):
        self.env.on_new_frame = hook

    def __getattr__(self, name):
        # (only what the wrapper does not define itself: the twin's own fields -- state, actor_id, seed of the game ...)
        if name == "env":
            raise AttributeError(name)
        return getattr(self.env, name)

    def state_words(self):
        return self.env.state_words()

    def get_initial_state(self):
        self.prev = 0
        return self.env.get_initial_state()

    def next(self, action):
        chosen = int(np.argmax(action))
        stuck = bool(sticks(self.sticky_p, self.sticky_seed, self.sticky_steps, np.array([self.sticky_g]), self.sticky_stream)[0])
        executed = self.prev if stuck else chosen
        self.sticky_steps += 1
        self.last_executed = executed
        if executed != chosen:
            action = np.zeros(len(action), dtype=np.asarray(action).dtype)
            action[executed] = 1
        observation, reward, terminal = self.env.next(action)
        self.prev = 0 if terminal else executed
        return observation, reward, terminal

    def get_legal_actions(self):
        return self.env.get_legal_actions()

    def get_noop(self):
        return self.env.get_noop()
