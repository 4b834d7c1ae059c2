"""PAAC learner (mirrors reference paac.py:13-187).

`PAACLearner(network_creator, environment_creator, args)`, `.train()`, `.cleanup()` and the static
`choose_next_actions(network, num_actions, states, session)` keep the reference's signatures.

train() has two executions of the SAME cycle (paac.py:99-183):
  * device-resident (environments with a device twin): T x [policy forward -> sample -> env step] ->
    bootstrap forward -> n-step returns -> forward/backward -> (RCCL all-reduce) -> clip + RMSProp, every
    stage a HIP kernel, the whole cycle replayed as a hipGraph; nothing crosses PCIe per step.
  * host environments (any BaseEnvironment plugin): the reference's loop, with session.run replaced by
    kernel launches and the numpy sampler/return maths by their HIP twins; actions are bit-identical to
    the reference's numpy sampler on the same np.random seed (paac_sample_mt).
"""
import functools
import logging
import os
import time

import numpy as np
import torch

from . import hip_ops, logger_utils, parallel, sticky, window_stats
from .actor_learner import ActorLearner
from .runners import TRUNCATED_ATTRIBUTE, EmulatorRunner, RawEmulatorRunner, Runners


# Device environments that carry a state record from step to step, by env_spec["kind"]: int32 words of a record and the reset
# and step wrappers (one argument list, catch's) from hip_ops.DEVICE_GAMES, the keys of the spec the step wrapper takes as
# keyword arguments, the longest episode of the game in steps (what bounds an evaluation: paac_amd/evaluation.py), and whether
# that length is a step cap the game can be cut off at (--bootstrap_truncated: the step then records a truncation plane) or
# the game's own rule (catch).  step_sticky: the step under --sticky_action_p (paac_amd/sticky.py) -- p, the tick (pointer and
# offset) and the two planes of previous actions in front of step's list, prev_out2 among its keywords.
def _stateful_kind(kind, spec_kwargs, max_episode_steps, truncates):
    return dict(words=hip_ops.DEVICE_GAMES[kind]["words"], reset=functools.partial(hip_ops.game_reset, kind),
                step=functools.partial(hip_ops.game_step, kind), spec_kwargs=spec_kwargs, max_episode_steps=max_episode_steps,
                truncates=truncates, step_sticky=functools.partial(hip_ops.game_step_sticky, kind))


STATEFUL_KINDS = {
    "catch": _stateful_kind("catch", (), 13, False),
    "bricks": _stateful_kind("bricks", ("single_life",), 500, True),
    "rally": _stateful_kind("rally", (), 1000, True),
}

# The paired kinds (hip_ops.PAIRED_GAMES, paac_amd/duel.py): the same fields -- to the rollout a paired game is a stateful game
# with N rows -- and eval_kind, the kind of STATEFUL_KINDS a run of this kind is evaluated as (duel has no evaluation of its
# own: its policy is scored as a rally agent, against the scripted opponent).  N must be even: two rows per board.
PAIRED_KINDS = {
    "duel": dict(words=hip_ops.PAIRED_GAMES["duel"]["words"], reset=hip_ops.duel_reset, step=hip_ops.duel_step, spec_kwargs=(),
                 max_episode_steps=1000, truncates=True, eval_kind="rally", step_sticky=hip_ops.duel_step_sticky),
}


# The user's game (paac_amd/user_game.py: --emulator user --device_game): _stateful_kind's fields under the kind "user", filled by
# user_game.load() from the specification module.  A table of its own, consulted after the two above.
USER_KINDS = {}


def register_user_kind(spec_kwargs, max_episode_steps, truncates):
    """-> the USER_KINDS entry of the user game hip_ops.USER_GAMES holds."""
    USER_KINDS["user"] = dict(words=hip_ops.USER_GAMES["user"]["words"], reset=hip_ops.user_game_reset, step=hip_ops.user_game_step,
                              spec_kwargs=tuple(spec_kwargs), max_episode_steps=int(max_episode_steps), truncates=bool(truncates),
                              step_sticky=functools.partial(hip_ops.game_step_sticky, "user"))
    return USER_KINDS["user"]


def stateful_kind(kind):
    """The entry of a non-paired game that carries a state record: STATEFUL_KINDS, then USER_KINDS; None for any other kind."""
    return STATEFUL_KINDS.get(kind) or USER_KINDS.get(kind)


def device_kind(env_spec):
    """The STATEFUL_KINDS, PAIRED_KINDS or USER_KINDS entry of a device env spec; None for the synthetic environments (or no
    spec)."""
    kind = (env_spec or {}).get("kind", "synthetic")
    return STATEFUL_KINDS.get(kind) or PAIRED_KINDS.get(kind) or USER_KINDS.get(kind)


def eval_env_spec(env_spec, **changes):
    """The env spec a run on `env_spec` is evaluated on: the spec itself with `changes` (the evaluation's seed, bricks'
    single_life off), or, for a paired kind, its eval_kind with the seed alone -- a duel run is scored on rally."""
    kind = None if env_spec is None else env_spec.get("kind", "synthetic")
    if kind in PAIRED_KINDS:
        return dict(kind=PAIRED_KINDS[kind]["eval_kind"], seed=changes.get("seed", env_spec["seed"]))
    return dict(env_spec, **changes) if env_spec is not None else None


class DeviceRollout(object):
    """Device-resident rollout/update cycle for N local environments x T steps."""
    truncs = None      # --bootstrap_truncated: the [T, N] truncation plane, allocated by __init__ only where it applies
    pool = None        # --duel_pool: the duel_pool.DevicePool, created by __init__ only with the pool on
    act_pipeline = False   # the small act_step route as two launches per step (act_step_pipe), set by __init__ only where it applies
    prev = None        # --sticky_action_p: the ring of previously executed actions, allocated by __init__ only with P > 0 and a game
    sticky_p = 0.0
    window_f = window_i = None   # --window_stats: the accumulator block (paac_amd/window_stats.py), allocated by __init__ only with the flag on

    def __init__(self, learner, env_spec, sampler="philox", sampler_seed=42, env_offset=0, use_graph=True,
                 total_envs=None):
        L = learner
        self.L = L
        dev = L.torch_device
        N, T, A = L.emulator_counts, L.max_local_steps, L.num_actions
        self.N, self.T, self.A = N, T, A
        self.total_envs = total_envs if total_envs is not None else N * L._world()
        self.env_spec = env_spec
        self.env_offset = int(env_offset)
        self.sampler = sampler
        self.sampler_seed = int(sampler_seed)
        self.use_graph = use_graph
        # Observation buffer of 2T+1 slots: even cycles use slots 0..T, odd cycles T..2T, so the last observation of
        # an even cycle IS the first of the odd one, and the T+1 observations of a cycle are contiguous (one
        # forward at batch N*(T+1) serves the update and the bootstrap); the last environment step of an odd cycle
        # writes its new stacks to slot 2T AND to slot 0 (stack_out2).  Two captured graphs alternate.
        self.states = torch.zeros((2 * T + 1, N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.parity = 0
        self.actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.values = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.masks = torch.zeros((T, N), dtype=torch.float32, device=dev)
        self.probs = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self.y = torch.zeros((T * N,), dtype=torch.float32, device=dev)
        self.adv = torch.zeros((T * N,), dtype=torch.float32, device=dev)
        self.ep_reward = torch.zeros((N,), dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.finished = torch.zeros((hip_ops.FINISHED_RING_BYTES // 4,), dtype=torch.int32, device=dev)
        self.tick = torch.zeros((1,), dtype=torch.int64, device=dev)          # env steps taken (per env)
        self.global_step_dev = torch.full((1,), int(L.global_step), dtype=torch.int64, device=dev)
        # the per-cycle bookkeeping (global_step, lr, frame counter) of whichever launch computes the cycle's returns
        self.cycle_tick = dict(global_step_dev=self.global_step_dev, increment=self.total_envs * T, initial_lr=L.initial_lr,
                               lr_annealing_steps=L.lr_annealing_steps, lr_out_dev=L.lr_dev, tick_dev=self.tick, tick_inc=T)
        self.raw = None
        # a stateful kind (STATEFUL_KINDS: catch, bricks, rally): the environments carry state from step to step -- a ring of state
        # records beside the observation ring, slot for slot (a step reads slot t and writes slot t + 1: nothing is updated in
        # place, and the wrap-around second output goes to slot 0 of both)
        # (a paired kind -- PAIRED_KINDS: duel -- is one more of them here: N rows, two per board, the same call)
        self.stateful = device_kind(env_spec)
        if env_spec.get("kind") in PAIRED_KINDS and N % 2:
            raise ValueError("-ec / --emulator_counts %d: --emulator %s plays two rows per board and needs an even number of "
                             "environments per rank" % (N, env_spec["kind"]))
        self.catch = env_spec.get("kind", "synthetic") == "catch"       # (read by the games' device-loop tests only)
        self.env_state = None
        if self.stateful:
            self.env_state = torch.zeros((2 * T + 1, N, self.stateful["words"]), dtype=torch.int32, device=dev)
            self.env_step_kwargs = {k: env_spec[k] for k in self.stateful["spec_kwargs"]}
        # --sticky_action_p P (env_spec["sticky_p"], paac_amd/sticky.py): a ring of the actions the environments executed, beside
        # env_state slot for slot -- a step reads slot t and writes slot t + 1, the wrap-around second output goes to slot 0 --
        # and the step goes through the game's sticky entry with the tick the sampler gets.  Zeroed: a run starts from the
        # no-op.  Shard-local: the draw's key carries env_offset.  P = 0 (or no game): no ring, the entries of always
        if self.stateful and float(env_spec.get("sticky_p", 0.0) or 0.0) > 0.0:
            if int(env_spec.get("pool", 0) or 0) > 0:
                raise ValueError("--sticky_action_p cannot be combined with --duel_pool: the pooled (ghost) step has no sticky form")
            self.sticky_p = float(env_spec["sticky_p"])
            self.prev = torch.zeros((2 * T + 1, N), dtype=torch.int32, device=dev)
        # --bootstrap_truncated: the truncation plane beside rewards and masks -- step t writes row t, whatever computes the
        # cycle's returns reads it.  Only with the flag on and a game that has a step cap: otherwise no plane exists, the step
        # goes through the game's own entry and every returns launch is the one it always was.  Shard-local, like the masks.
        if getattr(L, "bootstrap_truncated", False) and self.stateful and self.stateful["truncates"]:
            self.truncs = torch.zeros((T, N), dtype=torch.float32, device=dev)
        # --duel_pool K (env_spec["pool"], paac_amd/duel_pool.py): the N rows are N boards, each learner row at the bottom and a
        # ghost row of a frozen opponent at the top.  The ghosts have an observation ring of their own, slot for slot like
        # self.states (wrap output included), their probabilities and the actions they took (the plane a rollout is replayed
        # from on the twin), and the pool its tensors and a context of its own.  Off: none of this exists
        if env_spec.get("kind") == "duel" and int(env_spec.get("pool", 0) or 0) > 0:
            from . import duel_pool
            largs = getattr(L, "args", None)
            self.ghost_states = torch.zeros((2 * T + 1, N, 84, 84, 4), dtype=torch.uint8, device=dev)
            self.ghost_probs = torch.zeros((N, A), dtype=torch.float32, device=dev)
            self.ghost_actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
            self.pool = duel_pool.DevicePool(L.network.params, L.network.arch_id, A, N, int(env_spec["pool"]),
                                             int(getattr(largs, "duel_pool_every", 102400)),
                                             float(getattr(largs, "duel_pool_latest_p", 0.5)),
                                             int(getattr(largs, "random_seed", env_spec["seed"])), int(L.global_step),
                                             device_index=dev.index or 0)
        # --window_stats: the block one fold per cycle adds to, behind the cycle's last optimizer step (_update).  Off: no block,
        # no launch, the same graphs
        if getattr(L, "window_stats", False):
            if parallel.collectives_active():
                raise ValueError(window_stats.DATA_PARALLEL_REFUSAL)
            self.window_f, self.window_i = hip_ops.window_block(dev)
        # lets the large shards' sampler spread its walk over several workgroups (hip_ops.sample_mt_synth_step)
        self.walk_scratch = hip_ops.walk_scratch(N, A, dev) if N * (A - 1) <= hip_ops.FUSED_SAMPLE_MAX_DRAWS else None
        if env_spec.get("raw_frames"):
            self.raw = torch.zeros((N, 2, hip_ops.RAW_H, hip_ops.RAW_W), dtype=torch.uint8, device=dev)
        if sampler == "numpy":
            self.mt_state = hip_ops.mt_state_from_numpy(np.random.get_state(), dev)
            self.mt_scratch = hip_ops.sample_mt_scratch(N, A, dev)
        self.stream = torch.cuda.Stream(device=dev)
        self.graph_a = [None, None]
        self.graph_conv = [None, None]
        self.graph_b = None
        self.graph_multi = [None, None]                # MULTI consecutive cycles in one launch, by the ring parity they start at
        self.graph_multi_long = [None, None]           # MULTI_LONG of them
        self.graph_ua = [None, None]                   # data parallel: update of the previous cycle + graph_a
        self.pending_update = False
        # data parallel: the cycle contains the gradient exchange
        self.phased = parallel.collectives_active()
        # PAAC_ALLREDUCE = graph (default): ONE all-reduce of the whole flat gradient after the full backward, CAPTURED into
        #   the cycle's hipGraph between the backward and the optimizer step -- the data-parallel cycle is replayed exactly
        #   like the single-process one (MULTI cycles per graph launch, nothing issued eagerly); if the collective cannot be
        #   captured (backend gloo, or the capture raises) the loop falls back to `single`.
        # single: the same all-reduce issued eagerly on the rollout stream between two graph launches per cycle (measured
        #   with a one-rank RCCL group: +15 us per cycle over the plain replay).
        # split: the fc/heads tail (95 % of the bytes) goes out on the collective's stream while the conv backward still
        #   computes (+61 us per cycle of extra graph launch and cross-stream waits before any wire time: pays only when
        #   the large all-reduce takes longer than about 120 us)
        mode = os.environ.get("PAAC_ALLREDUCE", "graph")
        self.single_exchange = mode != "split"
        self.graph_exchange = self.phased and mode == "graph" and use_graph and parallel.backend() == "nccl"
        self.side_group = parallel.side_group() if (self.phased and not self.single_exchange) else None    # collective call
        # what the exchange really runs as (graph mode may fall back: capture()); PAAC_VERIFY_EXCHANGE=0 skips the check of
        # the replayed collective against the eager one
        self.exchange_mode = "none" if not self.phased else ("split" if not self.single_exchange else "single")
        self.exchange_fallback = None
        # --ppo_epochs K: epochs 2..K ride behind the cycle's update, each with its own exchange (one all-reduce per epoch)
        # --ppo_minibatches M: K * M optimizer steps per cycle instead, the first of them behind the record pass
        self.K = L.ppo_steps
        if self.K > 1 and self.phased and not self.single_exchange:
            raise ValueError("--ppo_epochs above 1%s is not built for PAAC_ALLREDUCE=split (the two-piece exchange): use graph "
                             "or single" % (" with --ppo_minibatches above 1" if L.minibatch_on else ""))
        self.graph_epoch = [[], []]                    # eager exchange: [parity][k - 1] = update + epoch k + 1's backward
        # --adv_norm: the actor term of every epoch reads the normalised advantages; self.adv stays the recorded raw array
        self.actor_adv = L.adv_n if L.adv_norm else self.adv
        self.short_first = os.environ.get("PAAC_SHORT_GRAPH_FIRST", "1") != "0"
        self.spin_sync = os.environ.get("PAAC_SPIN_SYNC", "1") != "0"
        self.verify_exchange = os.environ.get("PAAC_VERIFY_EXCHANGE", "1") != "0"
        # flat gradient = [conv tensors | fc_w fc_b actor critic]; the tail is 95 % of the bytes
        self.tail_offset = [t["offset"] for t in L.network.layout["tensors"] if t["name"].startswith("fc")][0]
        # The update needs no forward of its own: weights are frozen inside a cycle, so the T acting forwards have already
        # computed the activations paac.py:163-165 recomputes (TensorFlow's feed/fetch model forces that second pass; nothing
        # else does).  Acting step t keeps its rows at [t*N, (t+1)*N) of the training activation set, the N bootstrap
        # observations (paac.py:140-142) run as one acting-shaped forward into rows [T*N, (T+1)*N), and the backward starts
        # from there.  PAAC_REUSE_ACTING=0 restores the recomputed training forward (both routes are tested).
        # PAAC_MT_AHEAD=0: the large shards' step as paac_forward + paac_sample_mt_synth_step (every sampler workgroup rebuilds
        # the MT19937 blocks and doubles itself)
        # (the fused conv launches -- csrc/tower.h, csrc/tower2.h -- exist for the reference's two stock trunks)
        towered = getattr(L.network, "ARCH", None) in ("NATURE", "NIPS") and os.environ.get("PAAC_TOWER", "1") != "0"
        self.act_step_large = os.environ.get("PAAC_MT_AHEAD", "1") != "0" and N <= hip_ops.ACT_STEP_MAX_ENVS_LARGE and towered
        self.reuse_acting = os.environ.get("PAAC_REUSE_ACTING", "1") != "0" and towered and N <= hip_ops.KEEP_FORWARD_MAX_ROWS
        self.route = self._route()
        # The small act_step route runs pipelined (hip_ops.act_step_pipe): two launches per step, the sampler and the bookkeeping
        # of step t riding the fc launch of step t + 1 and those of the last step the bootstrap forward's -- which is why it
        # needs the kept acting rows (reuse_acting).  It rests on the path-A synthetic environments' frames not depending on
        # the action.  PAAC_ACT_PIPELINE=0, read here, restores the three-launch step.
        self.act_pipeline = (os.environ.get("PAAC_ACT_PIPELINE", "1") != "0" and self.route == "act_step" and self.raw is None
                             and self.reuse_acting and N <= hip_ops.ACT_STEP_MAX_ENVS
                             and N * (A - 1) <= hip_ops.ACT_STEP_MAX_DRAWS and A <= hip_ops.ACT_PIPE_MAX_ACTIONS)
        # what step t records, as every route's step call takes it (the per-cycle counterpart: cycle_tick above)
        self.records = [(self.rewards[t], self.masks[t], self.ep_reward, self.ep_len, self.finished) for t in range(T)]
        if self.pool is not None:
            hip_ops.duel_ghost_reset(env_spec["seed"], self.env_offset, self.env_state[0], self.states[0], self.ghost_states[0])
        elif self.stateful:
            self.stateful["reset"](env_spec["seed"], self.env_offset, self.env_state[0], self.states[0])
        else:
            hip_ops.synth_reset(env_spec["seed"], self.env_offset, self.states[0], self.raw)
        torch.cuda.synchronize(dev)

    # -- stages --------------------------------------------------------------------------------------
    def _slot(self, parity, t):
        return parity * self.T + t

    def rollout_states(self, parity=None):
        """[T*N,84,84,4] view of the states the LAST run cycle trained on (t-major, paac.py:151)."""
        parity = (self.parity ^ 1) if parity is None else parity
        T, N = self.T, self.N
        return self.states[parity * T:(parity + 1) * T].view(T * N, 84, 84, 4)

    def _route(self):
        """How an acting step runs (_act_step), decided once.  stateful: forward (+ sampler), then the game's step.  act_step (numpy
        sampler): the whole step in three launches -- conv tower, fc + head partials, heads finish + sampler + env step -- or, for
        the large shards (act_step_large), four.  fused: numpy sampler and env step in one launch behind the forward.  heads_step:
        counter-based sampler AND env step inside the heads kernel.  separate: forward + sampler, then the env step.  (Path B --
        self.raw -- rides act_step and fused too: they write the raw screen pairs and the preprocess launch follows.)"""
        N, draws = self.N, self.N * (self.A - 1)
        if self.stateful:
            return "stateful"
        if self.sampler != "numpy":
            return "heads_step" if self.raw is None else "separate"
        if draws > hip_ops.FUSED_SAMPLE_MAX_DRAWS:
            return "separate"
        small = N <= hip_ops.ACT_STEP_MAX_ENVS and draws <= hip_ops.ACT_STEP_MAX_DRAWS
        return "act_step" if (self.act_step_large or small) else "fused"

    def _act_step(self, parity, t):
        """Acting step t of a cycle: observation slot t -> action, value and records t, observation slot t + 1."""
        L, route = self.L, self.route
        params, slot, records = L.network.params, self._slot(parity, t), self.records[t]
        obs, nxt = self.states[slot], self.states[slot + 1]
        # the ring wraps after an odd cycle: its last step also writes slot 0 (the next even cycle's first slot)
        wrap = self.states[0] if (parity == 1 and t == self.T - 1) else None
        seed = self.env_spec["seed"]
        if self.reuse_acting:
            L.ctx.keep_next_forward(t * self.N)
        if route == "act_step" and self.act_pipeline:
            L.ctx.act_step_pipe(params, obs, self.mt_state, self.actions[t], self.probs, self.values[t], seed, self.env_offset,
                                self.env_spec["terminal_threshold"], self.tick, t, nxt, *records, stack_out2=wrap)
        elif route == "act_step":
            L.ctx.act_step_mt(params, obs, self.mt_state, self.actions[t], self.probs, self.values[t], seed, self.env_offset,
                              self.env_spec["terminal_threshold"], self.tick, t, nxt, *records, stack_out2=wrap,
                              raw_scratch=self.raw, walk_scratch=self.walk_scratch)
        elif route == "heads_step":
            L.ctx.forward_sample_synth_step(params, obs, self.sampler_seed, self.tick, t, self.env_offset, self.actions[t], seed,
                                            self.env_spec["terminal_threshold"], nxt, *records, probs=self.probs,
                                            values=self.values[t])
            if wrap is not None:          # this launch has no second output
                wrap.copy_(nxt)
        else:
            if self.sampler != "numpy":
                L.ctx.forward_sample(params, obs, self.sampler_seed, self.tick, t, self.env_offset, self.actions[t],
                                     probs=self.probs, values=self.values[t])
            else:
                L.ctx.forward(params, obs, probs=self.probs, values=self.values[t])
                if route != "fused":
                    hip_ops.sample_mt(self.probs, self.mt_state, self.mt_scratch, self.actions[t])
            if self.pool is not None:
                # the ghosts' forward on the pool's own context, behind the learner's (whose kept-forward state it never
                # sees), then the pooled step: the ghost's action is sampled inside it
                second = wrap is not None
                self.pool.ctx.forward(self.pool.opponent, self.ghost_states[slot], probs=self.ghost_probs)
                hip_ops.duel_ghost_step(seed, self.env_offset, self.actions[t], self.ghost_probs, self.sampler_seed, self.tick, t,
                                        self.env_state[slot], self.env_state[slot + 1], obs, nxt, self.ghost_states[slot],
                                        self.ghost_states[slot + 1], self.ghost_actions[t], *records, stack_out2=wrap,
                                        state_out2=self.env_state[0] if second else None,
                                        ghost_stack_out2=self.ghost_states[0] if second else None,
                                        truncs_out=self.truncs[t] if self.truncs is not None else None)
            elif route == "stateful" and self.prev is not None:
                second = wrap is not None
                self.stateful["step_sticky"](self.sticky_p, self.tick, t, self.prev[slot], self.prev[slot + 1], seed,
                                             self.env_offset, self.actions[t], self.env_state[slot], self.env_state[slot + 1],
                                             obs, nxt, *records, stack_out2=wrap,
                                             state_out2=self.env_state[0] if second else None,
                                             prev_out2=self.prev[0] if second else None,
                                             **(dict(truncs_out=self.truncs[t]) if self.truncs is not None else {}),
                                             **self.env_step_kwargs)
            elif route == "stateful":
                self.stateful["step"](seed, self.env_offset, self.actions[t], self.env_state[slot], self.env_state[slot + 1], obs,
                                      nxt, *records, stack_out2=wrap, state_out2=self.env_state[0] if wrap is not None else None,
                                      **(dict(truncs_out=self.truncs[t]) if self.truncs is not None else {}),
                                      **self.env_step_kwargs)
            elif route == "fused":
                hip_ops.sample_mt_synth_step(self.probs, self.mt_state, self.actions[t], seed, self.env_offset,
                                             self.env_spec["terminal_threshold"], self.tick, t, obs, nxt, *records,
                                             stack_out2=wrap, walk_scratch=self.walk_scratch, raw_scratch=self.raw)
            else:
                hip_ops.synth_step(seed, self.env_offset, self.actions[t], self.env_spec["terminal_threshold"], self.tick, t, obs,
                                   nxt, *records, stack_out2=wrap, raw_scratch=self.raw)

    def _rollout_and_backward(self, parity):
        L, T, N = self.L, self.T, self.N
        params = L.network.params
        keep = self.reuse_acting
        for t in range(T):
            self._act_step(parity, t)
        # training forward over the T*N rollout rows with the N bootstrap observations appended (paac.py:140-142)
        # (the forward stops after the fc layer: the heads of the rollout rows AND the value head of the bootstrap rows are
        # finished inside the backward's first launch)
        if keep:      # (its fc launch also pays what the last pipelined step owes: act_pipeline)
            L.ctx.bootstrap_forward_trunk(params, self.states[self._slot(parity, T)], T * N)
        else:
            L.ctx.train_forward_trunk(params, self.states[parity * T:(parity + 1) * T + 1].view((T + 1) * N, 84, 84, 4))
        phase = ((0 if self.single_exchange else 1) if self.phased else 3)
        if L.minibatch_on:
            self._record_and_first_minibatch(parity, phase)
            return
        if L.adv_norm:
            # --adv_norm: a row's workgroup cannot know the rollout's mean, so the returns leave the backward's first launch:
            # heads of the bootstrap rows, then returns + statistics + normalisation + the cycle's bookkeeping in one launch,
            # then the backward on (y, adv_n); the rollout rows' heads still ride in the backward's first launch
            L.ctx.returns_norm_tick(params, None, self.rewards, self.masks, self.values, L.gamma, self.y, self.adv, L.adv_n,
                                    L.adv_stats, gae_lambda=L.gae_lambda, truncs=self.truncs, **self.cycle_tick)
            L.ctx.loss_backward(params, self.rollout_states(parity), self.actions.view(-1), self.y, L.adv_n, L.entropy_beta,
                                L.grad, L.loss_dev, forward_done=True, phase=phase, p_old_out=L.p_old if self.K > 1 else None)
            if L.vclip_on:
                L.ctx.train_values_into(L.v_old, T * N)
            return
        # n-step returns + global_step/lr schedule + frame counter (paac.py:127,144-156) ride in the backward's first
        # launch.  One process: whole backward here, with the slab reduction of the conv weight gradients left to the norm
        # pass of the optimizer step that follows (phase 3: one launch less); data parallel: the complete gradient
        # (phase 0: the all-reduce needs it) or, in the split form, heads + fc only (phase 1), so that the all-reduce of
        # the fc/heads gradient tail overlaps the conv backward (phase 2, _backward_conv)
        L.ctx.loss_backward_returns(params, self.rollout_states(parity), self.actions.view(-1), None, self.rewards,
                                    self.masks, self.values, L.gamma, self.y, self.adv, L.entropy_beta, L.grad,
                                    L.loss_dev, forward_done=True, phase=phase, gae_lambda=L.gae_lambda,
                                    p_old_out=L.p_old if self.K > 1 else None, truncs=self.truncs, **self.cycle_tick)
        if L.vclip_on:         # --ppo_vclip: v_old = the values epoch 1's heads just computed (one captured copy)
            L.ctx.train_values_into(L.v_old, T * N)

    def _record_and_first_minibatch(self, parity, phase):
        """--ppo_minibatches: what follows the rollout and the bootstrap forward in an M > 1 cycle up to the first gradient --
        the record pass on the pre-update weights (p_old, v_old and the bootstrap values out of the finished heads; y / adv /
        adv_n and the cycle's bookkeeping from the standalone returns launches), the cycle's K shuffles on the frame counter
        the returns launch has just advanced, then optimizer step 0 (epoch 1's gather, minibatch 1)."""
        L, T, N = self.L, self.T, self.N
        B = T * N
        L.minibatch_record(self.actions.view(-1), B + N)
        v_boot = L.v_rec[B:]
        if L.adv_norm:
            hip_ops.returns_norm_tick(v_boot, self.rewards, self.masks, self.values, L.gamma, self.y, self.adv, L.adv_n,
                                      L.adv_stats, gae_lambda=L.gae_lambda, truncs=self.truncs, **self.cycle_tick)
        else:
            hip_ops.returns_tick(v_boot, self.rewards, self.masks, self.values, L.gamma, self.y, self.adv, L.gae_lambda,
                                 truncs=self.truncs, **self.cycle_tick)
        L.minibatch_perms(self.sampler_seed, self.tick)
        L.minibatch_step_backward(0, self.rollout_states(parity), self.actions.view(-1), self.y, self.actor_adv, phase)

    def _epoch_backward(self, parity, k):
        """Epoch k + 1 of the cycle up to its gradient (the update of epoch k has run); --ppo_minibatches: optimizer step k."""
        if self.L.minibatch_on:
            self.L.minibatch_step_backward(k, self.rollout_states(parity), self.actions.view(-1), self.y, self.actor_adv,
                                           phase=0 if self.phased else 3)
            return
        self.L.ppo_epoch_backward(k, self.rollout_states(parity), self.actions.view(-1), self.y, self.actor_adv,
                                  phase=0 if self.phased else 3)

    def _later_epochs(self, parity, exchange, before_last_update=None):
        """Behind the cycle's first update: epochs 2..K, each backward -> [exchange] -> update."""
        for k in range(1, self.K):
            self._epoch_backward(parity, k)
            if exchange:
                self._exchange(None)
            if before_last_update is not None and k == self.K - 1:
                before_last_update()
            self._update(k)

    def _backward_conv(self, parity):
        L = self.L
        L.ctx.loss_backward(L.network.params, self.rollout_states(parity), self.actions.view(-1), self.y, self.adv,
                            L.entropy_beta, L.grad, L.loss_dev, forward_done=True, phase=2)

    def _update(self, step):
        """Optimizer step `step` of the cycle (--ppo_target_kl gates by it); --window_stats: the cycle's fold behind its last one,
        inside the captured cycle."""
        self.L.apply_gradients(step)
        if self.window_f is not None and step == self.K - 1:
            self.L.window_fold(self.window_f, self.window_i, self.values, self.rewards, self.masks, self.actions, self.y, self.adv,
                               truncs=self.truncs, finished=self.finished)

    def capture(self):
        """Capture the cycle into hipGraphs: one per observation-ring parity (and a separate update graph when a
        gradient all-reduce sits between backward and the optimizer step)."""
        def captured(fn):
            g = hip_ops.Graph()
            g.begin()
            try:
                fn()
            except Exception:
                g.abort()
                raise
            g.end()
            return g

        def cycle(parity, with_update):
            self._rollout_and_backward(parity)
            if with_update:
                if self.graph_exchange:
                    self._exchange(None)          # recorded into the graph like the kernels around it
                self._update(0)
                self._later_epochs(parity, self.graph_exchange)

        if self.graph_exchange:
            # the communicator must exist before a capture can record its collective: one eager all-reduce of a scratch
            # word first; a capture that raises leaves the eager form in charge
            reason = None
            try:
                parallel.allreduce_sum_(torch.zeros(1, dtype=torch.float32, device=self.L.torch_device))
                torch.cuda.synchronize(self.L.torch_device)
                with torch.cuda.stream(self.stream):
                    for parity in (0, 1):
                        self.graph_a[parity] = captured(lambda: cycle(parity, True))
                    for p0 in (0, 1):
                        self.graph_multi[p0] = captured(lambda: [cycle((k + p0) & 1, True) for k in range(self.MULTI)])
                        if self.MULTI_LONG > self.MULTI:
                            self.graph_multi_long[p0] = captured(lambda: [cycle((k + p0) & 1, True) for k in range(self.MULTI_LONG)])
            except Exception as exc:      # noqa: BLE001 -- whatever the runtime / RCCL raised: keep training, eagerly
                reason = "the capture raised: %s" % (exc,)
            # every rank takes the same route: one that kept replaying graphs beside a peer issuing its collectives eagerly
            # would pair the wrong calls
            if not parallel.all_ranks(reason is None, self.L.torch_device):
                reason = reason or "the capture failed on another rank"
            elif self.verify_exchange:
                # ... and before the replayed collective is trusted: the same cycle, from the same state, once with the
                # eager exchange and once replayed -- the exchanged gradients must agree bit for bit, on every rank
                with torch.cuda.stream(self.stream):
                    same = self._replay_matches_eager()
                if not parallel.all_ranks(same, self.L.torch_device):
                    reason = "a replayed cycle's exchanged gradient differs from the eager exchange's" + ("" if not same else " on another rank")
            if reason is None:
                self.exchange_mode = "graph"
                return
            logging.warning("PAAC_ALLREDUCE=graph not used (%s): the all-reduce is issued eagerly between two graph launches", reason)
            self.exchange_fallback = reason
            self.close()
            self.graph_exchange = False
        with torch.cuda.stream(self.stream):
            for parity in (0, 1):
                self.graph_a[parity] = captured(lambda: cycle(parity, not self.phased))
                if self.phased:
                    if not self.single_exchange:
                        self.graph_conv[parity] = captured(lambda: self._backward_conv(parity))
                    # the optimizer step of cycle k rides in front of cycle k+1's graph: two graph launches per
                    # cycle around the exchange instead of three (synchronize() flushes a pending step)
                    self.graph_ua[parity] = captured(lambda: (self._update(self.K - 1), cycle(parity, False)))
                    self.graph_epoch[parity] = [captured(lambda: (self._update(k - 1), self._epoch_backward(parity, k)))
                                                for k in range(1, self.K)]
            if self.phased:
                self.graph_b = captured(lambda: self._update(self.K - 1))
            else:
                for p0 in (0, 1):
                    self.graph_multi[p0] = captured(lambda: [cycle((k + p0) & 1, True) for k in range(self.MULTI)])
                    if self.MULTI_LONG > self.MULTI:
                        self.graph_multi_long[p0] = captured(lambda: [cycle((k + p0) & 1, True) for k in range(self.MULTI_LONG)])

    # -- trust, but verify: the captured exchange ---------------------------------------------------------
    def _cycle_state(self):
        """Every tensor one cycle reads and writes (the rollout's and the learner's): a snapshot of them is a restart point.
        (The optimizer state includes Adam's bias-correction powers: left out, a replayed check would advance them twice.)"""
        L = self.L
        ts = [self.states, self.actions, self.values, self.rewards, self.masks, self.probs, self.y, self.adv, self.ep_reward,
              self.ep_len, self.finished, self.tick, self.global_step_dev] + [t for _, t in L.update_state] + \
             [L.grad_store, L.lr_dev, L.gnorm_dev, L.loss_dev] + \
             [t for t in (L.p_old, L.ppo_loss, L.ppo_stats, L.adv_n, L.adv_stats, L.v_old, L.kl_stop, L.ppo_applied, L.ppo_kl_checked)
              if t is not None]
        if L.minibatch_on:      # (the staging block of states is rewritten by every epoch's gather before anything reads it)
            ts += [L.v_rec] + [t for k, t in L.mb.items() if t is not None and k != "states"]
        for name in ("raw", "walk_scratch", "mt_state", "env_state", "prev", "truncs", "ghost_states", "ghost_probs", "ghost_actions"):
            t = getattr(self, name, None)
            if t is not None:
                ts.append(t)
        return ts

    def _replay_matches_eager(self):
        """One cycle from the current state with the all-reduce issued eagerly, the state put back, the same cycle replayed
        from the captured graph (all-reduce inside), the state put back again: True when the two exchanged gradients are
        bit-identical.  Nothing of either run survives: training starts from the state this was called in."""
        L = self.L
        state = self._cycle_state()
        saved = [t.clone() for t in state]

        def restore():
            for t, s in zip(state, saved):
                t.copy_(s)
            L.ctx.pack_weights(L.network.params)          # the optimizer step re-packed the updated weights

        self._rollout_and_backward(0)
        self._exchange(None)
        eager = [L.grad.clone()]
        self._update(0)                                   # (consumes what the backward left pending in the ctx)
        # (--ppo_epochs: the LAST epoch's exchanged gradient is compared -- it depends on every exchange before it)
        self._later_epochs(0, True, before_last_update=lambda: eager.__setitem__(0, L.grad.clone()))
        eager = eager[0]
        restore()
        self.graph_a[0].launch()                          # backward -> captured all-reduce -> update; grad stays as exchanged
        replayed = L.grad.clone()
        restore()
        self.stream.synchronize()
        return bool(torch.equal(eager, replayed))

    def check_replicas(self, what="weights"):
        """Data parallel: all ranks must hold bit-identical weights and optimizer slots (identical start, identical
        all-reduced gradient, identical update).  Raises parallel.ReplicaMismatch on every rank when they do not."""
        L = self.L
        self.synchronize()
        named = L.update_state if what == "weights" else [("grad", L.grad)]
        names, tensors = [n for n, _ in named], [t for _, t in named]
        with torch.cuda.stream(self.stream):
            ok, same = parallel.replicas_identical(tensors)
        if not ok:
            bad = [n for n, s in zip(names, same) if not s]
            raise parallel.ReplicaMismatch("data-parallel replicas diverged: %s differ between ranks (exchange mode %s, rank %d of %d)"
                                           % (", ".join(bad), self.exchange_mode, parallel.rank(), parallel.world_size()))
        return True

    # cycles per launch of graph_multi / graph_multi_long (even: the ring parity is back at 0 afterwards).  Measured at the
    # headline configuration, cycles per launch 4 / 8 / 16 / 32: 643.5 / 645.6 / 648.6 / 648.1 k env-steps/s.
    MULTI = max(2, int(os.environ.get("PAAC_CYCLES_PER_LAUNCH", "4")) // 2 * 2)
    MULTI_LONG = max(MULTI, int(os.environ.get("PAAC_CYCLES_PER_LONG_LAUNCH", "16")) // 2 * 2)

    def run_cycles(self, count):
        """`count` cycles.  Graph replay batches them MULTI_LONG or MULTI per hipGraph launch where it can: the gap between
        two graph launches on the GPU (about 8 us) is paid once per batch instead of every cycle."""
        count = int(count)
        if self.use_graph and self.graph_a[0] is None and count > 0:
            with torch.cuda.stream(self.stream):
                self.capture()            # first: a captured exchange that is refused changes which graphs exist
        while count > 0:
            if self.use_graph and (not self.phased or self.graph_exchange) and count >= self.MULTI:
                # (an even number of cycles per launch: the ring parity is the same afterwards; there is a graph per starting
                # parity -- a caller that has run an odd number of cycles, e.g. a 5-cycle warm-up, keeps the batched launches)
                with torch.cuda.stream(self.stream):
                    # the SHORT graph first: submitting a replay costs host time in proportion to its nodes, and an idle GPU
                    # waits for it -- behind MULTI cycles already running, the long graphs' submissions are hidden
                    if self.graph_multi_long[self.parity] is not None and count >= self.MULTI_LONG and (
                            self.short_first is False or count % self.MULTI_LONG < self.MULTI):
                        self.graph_multi_long[self.parity].launch()
                        count -= self.MULTI_LONG
                        continue
                    self.graph_multi[self.parity].launch()
                count -= self.MULTI
            else:
                self.run_cycle()
                count -= 1

    def run_cycle(self):
        with torch.cuda.stream(self.stream):
            if self.use_graph:
                if self.graph_a[0] is None:
                    self.capture()
                if self.phased and not self.graph_exchange:
                    (self.graph_ua if self.pending_update else self.graph_a)[self.parity].launch()
                    self._exchange(None if self.single_exchange else self.graph_conv[self.parity].launch)
                    for g in self.graph_epoch[self.parity]:      # update of the epoch before + this epoch's backward
                        g.launch()
                        self._exchange(None)
                    self.pending_update = True
                else:
                    self.graph_a[self.parity].launch()
            else:
                self._rollout_and_backward(self.parity)
                if self.phased:
                    self._exchange(None if self.single_exchange else (lambda: self._backward_conv(self.parity)))
                self._update(0)
                self._later_epochs(self.parity, self.phased)
        self.parity ^= 1

    def _exchange(self, conv_backward):
        """Sum all-reduce of the flat gradient: one collective on our stream after the full backward (conv_backward is
        None), or in two pieces -- the fc/heads tail goes out on the collective's own stream while `conv_backward` still
        computes the conv head on ours; the update waits for both."""
        grad = self.L.grad
        if conv_backward is None:          # PAAC_ALLREDUCE=single: the backward is complete, one collective
            # (the whole store: under --ppo_target_kl the step's approx_kl travels behind the gradient)
            parallel.allreduce_sum_(self.L.grad_store)  # a blocking-style call runs ON our stream: no cross-stream event hops
            return
        tail = parallel.allreduce_sum_async(grad[self.tail_offset:])
        conv_backward()
        # the small conv part follows the conv backward on our own stream (nothing to overlap it with) and on a second
        # communicator (it does not queue behind the 6.4 MB one); the update then waits for the large one, which has been
        # travelling on the collective's stream meanwhile
        parallel.allreduce_sum_(grad[:self.tail_offset], group=self.side_group)
        if tail is not None:
            tail.wait()

    def synchronize(self):
        """Completes everything issued so far, including a data-parallel optimizer step still waiting to ride in
        front of the next cycle: afterwards weights, optimizer state and buffers are those of the last cycle."""
        if self.pending_update:
            with torch.cuda.stream(self.stream):
                self.graph_b.launch()
            self.pending_update = False
        if self.spin_sync:
            # poll instead of sleeping on the stream: the wake-up of a blocking synchronize costs tens of microseconds, which a
            # caller that brackets short runs (bench.py's 20-cycle windows are 5 ms) pays every time
            done = torch.cuda.Event()
            done.record(self.stream)
            while not done.query():
                pass
            return
        self.stream.synchronize()

    def finished_episodes(self):
        """Drain the device ring of finished episodes -> list of (reward, length)."""
        host = self.finished.cpu().numpy()
        count = int(host[0])
        n = min(count, 4096)
        rewards = host[2:2 + 4096].view(np.float32)
        lens = host[2 + 4096:2 + 8192]
        idx = [(count - n + i) & 4095 for i in range(n)]
        return count, [(float(rewards[i]), int(lens[i])) for i in idx]

    def close(self):
        for g in (self.graph_a[0], self.graph_a[1], self.graph_conv[0], self.graph_conv[1], self.graph_b, self.graph_multi[0],
                  self.graph_multi[1], self.graph_multi_long[0], self.graph_multi_long[1],
                  self.graph_ua[0], self.graph_ua[1]) + tuple(self.graph_epoch[0]) + tuple(self.graph_epoch[1]):
            if g is not None:
                g.close()
        self.graph_a = [None, None]
        self.graph_conv = [None, None]
        self.graph_b = None
        self.graph_multi = [None, None]
        self.graph_multi_long = [None, None]
        self.graph_ua = [None, None]
        self.graph_epoch = [[], []]


class DeviceObservations(object):
    """Observations of host environments that emit raw screens, built on the GPU: the screen pairs travel through
    pinned staging buffers, paac_preprocess_stack does max + nearest resize + history push for all environments in
    one launch per slot (one slot per step; HISTORY slots for the environments that were just reset)."""

    def __init__(self, n_envs, slots, dev):
        self.staging = torch.empty((slots, n_envs, 2, hip_ops.RAW_H, hip_ops.RAW_W), dtype=torch.uint8).pin_memory()
        self.mask_staging = torch.empty((slots, n_envs), dtype=torch.uint8).pin_memory()
        self.d_raw = torch.empty((slots, n_envs, 2, hip_ops.RAW_H, hip_ops.RAW_W), dtype=torch.uint8, device=dev)
        self.d_mask = torch.empty((slots, n_envs), dtype=torch.uint8, device=dev)
        self.current = torch.zeros((n_envs, 84, 84, 4), dtype=torch.uint8, device=dev)

    def update(self, raw, counts):
        """raw u8 [N,slots,2,210,160], counts [N]: environment i pushes its first counts[i] slots."""
        if tuple(raw.shape[2:]) != (2, hip_ops.RAW_H, hip_ops.RAW_W):
            raise ValueError("device preprocessing expects %dx%d screens, got %s" %
                             (hip_ops.RAW_H, hip_ops.RAW_W, tuple(raw.shape[3:])))
        counts = np.asarray(counts).astype(np.int64)
        for j in range(int(counts.max())):
            self.staging[j].copy_(torch.from_numpy(raw[:, j]))
            self.mask_staging[j].copy_(torch.from_numpy((counts > j).astype(np.uint8)))
            self.d_raw[j].copy_(self.staging[j], non_blocking=True)
            self.d_mask[j].copy_(self.mask_staging[j], non_blocking=True)
            hip_ops.preprocess_stack(self.d_raw[j], self.current, self.current, push_mask=self.d_mask[j])
        return self.current


class PAACLearner(ActorLearner):
    def __init__(self, network_creator, environment_creator, args):
        super(PAACLearner, self).__init__(network_creator, environment_creator, args)
        self.workers = args.emulator_workers
        self.args = args
        self.runners = None
        self.rollout = None
        self.metrics = None
        self.stop_requested = False      # set by the signal handler (train.py); honoured at the next cycle boundary
        self.host_truncated_steps = None   # host loop under --bootstrap_truncated: ones in the last rollout's truncation plane
        self.host_window = None            # host loop under --window_stats: its (acc_f, acc_i) block
        self.host_window_episodes = ([], [])   # ... and the (returns, lengths) of the episodes finished since the last record

    def _open_metrics(self):
        """metrics.jsonl in the debugging folder (rank 0 only): what the reference sends to TensorBoard."""
        if self.metrics is None and parallel.rank() == 0 and getattr(self.args, "metrics", True):
            self.metrics = logger_utils.MetricsWriter(self.debugging_folder)
        return self.metrics

    def truncated_steps(self):
        """--bootstrap_truncated: the number of ones in the last rollout's truncation plane (this rank's); None when no plane
        exists -- the flag is off, or the environments have no step cap to report."""
        if self.rollout is not None and self.rollout.truncs is not None:
            return int(self.rollout.truncs.sum().item())
        return self.host_truncated_steps

    def _truncation_applies(self):
        """Whether --bootstrap_truncated has anything to act on; logs the one line that says so when it has not."""
        if not self.bootstrap_truncated:
            return False
        if self._use_device_envs():
            kind = device_kind(self.environment_creator.device_env_spec)
            on = bool(kind and kind["truncates"])
        else:
            on = any(hasattr(e, TRUNCATED_ATTRIBUTE) for e in self.emulators)
        if not on:
            logging.info("--bootstrap_truncated true does nothing here: these environments report no step-cap endings")
        return on

    def _progress_record(self, steps_per_s, steps_per_s_avg, last_ten):
        if self.metrics is None:
            return
        # (an M > 1 --ppo_minibatches cycle has no full-batch update: its summary line carries the last optimizer step's loss)
        loss = (self.ppo_loss[-1] if self.minibatch_on else self.loss_dev).cpu().numpy()
        stats = self.ctx.grad_stats(self.clip_norm, self.clip_mode)      # actor_learner.py:85-87 summaries
        self.metrics.write("gradients", global_step=int(self.global_step), **stats)
        # --ppo_target_kl: which optimizer steps of the last cycle were applied, and the value each gate compared
        applied = checked = None
        if self.target_kl_on:
            applied, checked = self.ppo_applied.cpu().numpy(), self.ppo_kl_checked.cpu().numpy()
        self.metrics.write("progress", global_step=int(self.global_step), steps_per_s=float(steps_per_s),
                           steps_per_s_avg=float(steps_per_s_avg), last_10_rewards_avg=float(last_ten),
                           lr=float(self.lr_dev.item()), grad_norm=float(self.gnorm_dev.item()), loss=float(loss[0]),
                           actor_loss=float(loss[1]), critic_loss=float(loss[2]), entropy=float(loss[3]),
                           **(dict(ppo_steps_applied=int(applied.sum())) if applied is not None else {}),
                           **(dict(truncated_steps=self.truncated_steps()) if self.truncated_steps() is not None else {}))
        if self.ppo_epochs > 1:          # one record per epoch of the last cycle (epoch 1: the update above, ratio == 1)
            losses, stats = self.ppo_loss.cpu().numpy(), self.ppo_stats.cpu().numpy()
            if not self.minibatch_on:
                losses[0] = loss
            for k in range(self.ppo_steps):
                # --ppo_minibatches above 1: one record per optimizer step, `minibatch` = 1..M inside its epoch
                where = dict(minibatch=k % self.ppo_minibatches + 1) if self.minibatch_on else {}
                epoch = k // self.ppo_minibatches + 1 if self.minibatch_on else k + 1
                self.metrics.write("ppo_epoch", global_step=int(self.global_step), epoch=epoch, **where, loss=float(losses[k, 0]),
                                   actor_loss=float(losses[k, 1]), critic_loss=float(losses[k, 2]),
                                   entropy=float(losses[k, 3]), clip_fraction=float(stats[k, 0]),
                                   approx_kl=float(stats[k, 1]),
                                   **(dict(value_clip_fraction=float(stats[k, 2])) if self.vclip_on else {}),
                                   **(dict(applied=bool(applied[k]), kl_checked=float(checked[k])) if self.is_gated_step(k)
                                      else {}))
        if self.adv_norm:                # the statistics the last rollout's advantages were normalised by (this rank's)
            mean, std = self.adv_stats.cpu().numpy()
            self.metrics.write("adv_norm", global_step=int(self.global_step), mean=float(mean), std=float(std))
        self.metrics.flush()

    def window_fold(self, acc_f, acc_i, values, rewards, masks, actions, y, adv, truncs=None, finished=None):
        """--window_stats: the cycle that has just had its last optimizer step, folded into the block -- the rollout's planes as
        given, the update's scalars from where this learner's update options leave them."""
        ppo = self.ppo_epochs > 1
        hip_ops.window_fold(acc_f, acc_i, values, rewards, masks, actions, y, adv, self.num_actions,
                            loss=self.ppo_loss if ppo else self.loss_dev.view(1, 4), gnorm=self.gnorm_dev, truncs=truncs,
                            # (a full-batch PPO cycle reports epoch 1 through loss_dev, and its ppo_stats row 0 stays zero)
                            loss0=self.loss_dev if ppo and not self.minibatch_on else None,
                            ppo_stats=self.ppo_stats if ppo else None, stats_first=0 if self.minibatch_on else 1,
                            applied=self.ppo_applied, finished=finished)

    def _window_loss_rows(self):
        """The loss scalars a cycle's fold read, one row per optimizer step (what window_fold hands over, on the host)."""
        if self.ppo_epochs == 1:
            return self.loss_dev.cpu().numpy().reshape(1, 4)
        rows = self.ppo_loss.cpu().numpy().copy()
        if not self.minibatch_on:
            rows[0] = self.loss_dev.cpu().numpy()
        return rows

    def _window_read(self, acc_f, acc_i, episodes=None):
        """--window_stats at a progress record: the block copied out (the caller has synchronised) and emptied on the current
        stream -- ring_cursor stays with the ring -> (the `window` record's fields, what the log line gains).  episodes: the
        host loop's (returns, lengths) of the window, folded on the host."""
        acc = window_stats.Block(acc_f.cpu().numpy(), acc_i.cpu().numpy())
        if episodes is not None:
            window_stats.fold_episodes(acc, *episodes)
        acc_f.zero_()
        acc_i[:window_stats.FIELDS_I["ring_cursor"][0]].zero_()
        truncation = self.rollout.truncs is not None if self.rollout is not None else bool(getattr(self, "truncation_on", False))
        record = window_stats.summary(acc, num_actions=self.num_actions, truncation=truncation,
                                      ppo=self.ppo_epochs > 1, vclip=self.vclip_on)
        ev, ret = record["explained_variance"], record["episode_return_mean"]
        return record, ", explained variance {}, {} episodes of mean return {} in the window".format(
            "n/a" if ev is None else "%.4f" % ev, record["episodes"], "n/a" if ret is None else "%.4f" % ret)

    def _window_record(self, record):
        """The `window` record behind the `progress` record."""
        if self.metrics is not None:
            self.metrics.write("window", global_step=int(self.global_step), **record)
            self.metrics.flush()

    @staticmethod
    def choose_next_actions(network, num_actions, states, session):
        network_output_v, network_output_pi = session.run(
            [network.output_layer_v, network.output_layer_pi],
            feed_dict={network.input_ph: states})
        action_indices = PAACLearner._sample_policy_action(network_output_pi)
        new_actions = np.eye(num_actions)[action_indices]
        return new_actions, network_output_v, network_output_pi

    @staticmethod
    def _sample_policy_action(probs):
        """paac.py:34-45 executed by paac_sample_mt on the global np.random MT19937 stream: the stream is
        uploaded, advanced on the device exactly as numpy's multinomial would advance it, and written back."""
        probs = np.ascontiguousarray(np.asarray(probs, dtype=np.float32))
        dev = torch.device("cuda", torch.cuda.current_device())
        p = torch.from_numpy(probs).to(dev)
        state = hip_ops.mt_state_from_numpy(np.random.get_state(), dev)
        scratch = hip_ops.sample_mt_scratch(p.shape[0], p.shape[1], dev)
        actions = torch.empty((p.shape[0],), dtype=torch.int32, device=dev)
        hip_ops.sample_mt(p, state, scratch, actions)
        np.random.set_state(hip_ops.mt_state_to_numpy(state))
        return [int(a) for a in actions.cpu().numpy()]

    def _use_device_envs(self):
        spec = getattr(self.environment_creator, "device_env_spec", None)
        return spec is not None and not getattr(self.args, "host_environments", False)

    def train(self):
        """Main actor learner loop for parallel advantage actor critic learning (paac.py:59-183)."""
        self.global_step = self.init_network()
        logging.debug("Starting training at Step {}".format(self.global_step))
        self.truncation_on = self._truncation_applies()
        if self._use_device_envs():
            self._train_device()
        else:
            self._train_host()
        self.cleanup()

    # -- device-resident loop ------------------------------------------------------------------------
    def _train_device(self):
        args = self.args
        world = self._world()
        rank = 0
        if world > 1:
            import torch.distributed as dist
            rank = dist.get_rank()
        N, T = self.emulator_counts, self.max_local_steps
        self.rollout = DeviceRollout(self, self.environment_creator.device_env_spec,
                                     sampler=getattr(args, "sampler", "philox"),
                                     sampler_seed=getattr(args, "sampler_seed", 42), env_offset=rank * N,
                                     use_graph=getattr(args, "use_graph", True))
        counter = 0
        global_step_start = self.global_step
        start_time = time.time()
        log_every = 2048 / self.emulator_counts            # paac.py:172 (float division, as upstream)
        steps_per_cycle = N * T * world
        metrics = self._open_metrics()
        episodes_seen = 0
        from .actor_learner import CHECKPOINT_INTERVAL
        since_stop_check = 0
        # data parallel: the replicas are compared (checksums of weights and optimizer slots, MIN / MAX over ranks) right
        # after the first update -- with the exchanged gradient -- and then every PAAC_REPLICA_CHECK_CYCLES cycles; a
        # mismatch ends the run on every rank (parallel.ReplicaMismatch -> non-zero exit)
        check_every = max(1, int(os.environ.get("PAAC_REPLICA_CHECK_CYCLES", "1024")))
        next_check = 1 if parallel.collectives_active() else None
        # --eval_every: a DeviceEvaluator (paac_amd/evaluation.py) on a context of its own -- unmanaged: its forwards repack the
        # weights they are given -- scores the live weights at the first chunk boundary at or after every multiple of
        # eval_every global steps.  It draws from its own Philox streams and writes only its own buffers: the training
        # context, its kept-forward state, its graphs, tick, the finished ring and the MT19937 state are never touched
        from . import evaluation
        evaluator = eval_ctx = None
        eval_every = int(getattr(args, "eval_every", 0)) if evaluation.check_train_flags(args, world) else 0
        # --eval_match: at every evaluation the live weights also play duel boards against a device copy of the weights of the
        # previous evaluation (paac_amd/match.py: DeviceMatch) -- on the evaluator's context, its own streams and buffers
        from . import match
        # --duel_pool: the rollout's pool of frozen opponents (paac_amd/duel_pool.py); its events cap the chunk as the
        # evaluations do
        from . import duel_pool
        pool = self.rollout.pool
        matcher = snapshot = None
        match_boards = int(getattr(args, "eval_match", 0)) if match.check_train_flags(args) else 0
        if eval_every:
            count = int(getattr(args, "eval_count", 64))
            seed = int(getattr(args, "random_seed", 3)) + 1
            eval_ctx = hip_ops.Context(self.network.arch_id, self.num_actions,
                                       max_batch=min(max(count, match_boards), evaluation.MAX_CHUNK),
                                       device_index=self.torch_device.index or 0)
            spec = eval_env_spec(self.environment_creator.device_env_spec, seed=seed, single_life=False)
            scripted = self.environment_creator.device_env_spec.get("kind") in PAIRED_KINDS       # duel: scored on rally
            evaluator = evaluation.DeviceEvaluator(self.network, eval_ctx, spec, count, noops=30,
                                                   greedy=bool(getattr(args, "eval_greedy", True)), seed=seed,
                                                   use_graph=getattr(args, "use_graph", True), stream=self.rollout.stream,
                                                   sticky_p=sticky.flag_of(args))
            next_eval = (self.global_step // eval_every + 1) * eval_every
            if match_boards:
                with torch.cuda.stream(self.rollout.stream):
                    snapshot = self.network.params.clone()          # the weights the run started or resumed from
                self.rollout.stream.synchronize()
                snapshot_step = int(self.global_step)
                matcher = match.DeviceMatch(self.network.params, eval_ctx, snapshot, eval_ctx, match_boards, noops=30,
                                            greedy=bool(getattr(args, "eval_greedy", True)), seed=seed, game_seed=seed,
                                            use_graph=getattr(args, "use_graph", True), stream=self.rollout.stream)
        while self.global_step < self.max_global_steps:
            if next_check is not None and counter >= next_check:
                if next_check == 1:
                    self.rollout.check_replicas("grad")
                self.rollout.check_replicas("weights")
                next_check = counter + check_every
            if world == 1:
                if self.stop_requested:
                    break
            elif since_stop_check >= 16:       # all ranks must leave at the same cycle (one collective per >= 16 cycles)
                since_stop_check = 0
                if parallel.any_rank(self.stop_requested, self.torch_device):
                    break
            loop_start_time = time.time()
            # as many cycles per call as fit before the next event the reference checks every cycle: the end of
            # training, the progress line (paac.py:172) and the checkpoint (actor_learner.py:89-93)
            chunk = 1
            if float(log_every).is_integer():
                until_end = -(-(self.max_global_steps - self.global_step) // steps_per_cycle)
                until_log = int(log_every) - counter % int(log_every)
                until_save = -(-(self.last_saving_step + CHECKPOINT_INTERVAL - self.global_step) // steps_per_cycle)
                chunk = max(1, min(until_end, until_log, until_save))
                if evaluator is not None:
                    until_eval = -(-(next_eval - self.global_step) // steps_per_cycle)
                    chunk = max(1, min(chunk, until_eval))
                if pool is not None:
                    chunk = max(1, min(chunk, duel_pool.until_pool(pool.schedule.next_event, self.global_step, steps_per_cycle)))
            if next_check is not None:
                chunk = max(1, min(chunk, next_check - counter))
            self.rollout.run_cycles(chunk)
            self.global_step += chunk * steps_per_cycle
            counter += chunk
            since_stop_check += chunk
            if counter % log_every == 0:
                self.rollout.synchronize()
                curr_time = time.time()
                count, eps = self.rollout.finished_episodes()
                last_ten = 0.0 if len(eps) < 1 else np.mean([r for r, _ in eps[-10:]])
                window, window_text = None, ""
                if self.rollout.window_f is not None:
                    with torch.cuda.stream(self.rollout.stream):
                        window, window_text = self._window_read(self.rollout.window_f, self.rollout.window_i)
                logging.info("Ran {} steps, at {} steps/s ({} steps/s avg), last 10 rewards avg {}{}"
                             .format(self.global_step, chunk * steps_per_cycle / (curr_time - loop_start_time),
                                     (self.global_step - global_step_start) / (curr_time - start_time), last_ten, window_text))
                if metrics is not None:
                    for r, l in eps[max(0, len(eps) - (count - episodes_seen)):]:     # new since the last drain
                        metrics.write("episode", global_step=int(self.global_step), reward=float(r), length=int(l))
                    episodes_seen = count
                    self._progress_record(chunk * steps_per_cycle / (curr_time - loop_start_time),
                                          (self.global_step - global_step_start) / (curr_time - start_time), last_ten)
                if window is not None:
                    self._window_record(window)
            if pool is not None and pool.schedule.due(self.global_step):
                # a pool event, between two run_cycles calls and on the rollout's stream: two device-to-device copies and the
                # repack, queued behind the cycles already issued -- nothing here waits for the GPU
                with torch.cuda.stream(self.rollout.stream):
                    record = pool.event(self.global_step, self.network.params)
                logging.info("Duel pool at {} steps: live weights into slot {} ({} of {} taken), next opponent slot {} (the "
                             "weights of {} steps{})".format(record["global_step"], record["slot"], record["size"], pool.schedule.K,
                                                             record["opponent_slot"], record["opponent_global_step"],
                                                             ", the newest" if record["latest"] else ""))
                if metrics is not None:
                    metrics.write("duel_pool", **record)
                    metrics.flush()
            if evaluator is not None and self.global_step >= next_eval:
                self.rollout.synchronize()
                scores, lengths, seconds = evaluator.timed_run()
                record = evaluator.summary(scores, lengths, seconds)
                if scripted:
                    record["opponent"] = "scripted"
                next_eval = (self.global_step // eval_every + 1) * eval_every
                logging.info("Evaluation at {} steps: {} episodes ({}), mean {:.3f}, min {:.3f}, max {:.3f}, std {:.3f}, mean "
                             "length {:.1f}, {:.3f} s".format(self.global_step, record["count"],
                                                              ("greedy" if record["greedy"] else "sampled") +
                                                              (", sticky actions P = %g" % record["sticky_action_p"]
                                                               if "sticky_action_p" in record else ""), record["mean"],
                                                              record["min"], record["max"], record["std"],
                                                              record["mean_length"], seconds))
                if metrics is not None:
                    metrics.write("eval", global_step=int(self.global_step), **record)
                    metrics.flush()
                if matcher is not None:
                    scores, lengths, seconds = matcher.timed_run()
                    record = matcher.summary(scores, lengths, seconds)
                    logging.info("Match at {} steps against the weights of {} steps: {} boards ({}), mean {:.3f}, wins / draws / "
                                 "losses {:.3f} / {:.3f} / {:.3f}, mean length {:.1f}, {:.3f} s"
                                 .format(self.global_step, snapshot_step, record["count"],
                                         "greedy" if record["greedy"] else "sampled", record["mean"], record["wins"],
                                         record["draws"], record["losses"], record["mean_length"], seconds))
                    if metrics is not None:
                        metrics.write("match", global_step=int(self.global_step), opponent="previous",
                                      opponent_global_step=snapshot_step, **record)
                        metrics.flush()
                    with torch.cuda.stream(self.rollout.stream):
                        snapshot.copy_(self.network.params)          # the next match's opponent
                    self.rollout.stream.synchronize()
                    snapshot_step = int(self.global_step)
            self.save_vars()          # _sync_device() flushes the rollout first when a checkpoint is due
        self.rollout.synchronize()
        if matcher is not None:
            matcher.close()
        if evaluator is not None:
            evaluator.close()
            eval_ctx.close()
        if next_check is not None:
            self.rollout.check_replicas("weights")

    # -- host-environment loop (the reference's structure, kernels instead of session.run) ------------
    def _train_host(self):
        dev = self.torch_device
        N, T, A = self.emulator_counts, self.max_local_steps, self.num_actions
        counter = 0
        global_step_start = self.global_step
        total_rewards = []
        raw_mode = bool(getattr(self.args, "device_preprocess", False))
        # --bootstrap_truncated: one more shared array carries the last step's truncation flags (runners.py), one more [T, N]
        # plane travels to the device with the masks; off, nothing below exists
        truncation_on = getattr(self, "truncation_on", False)
        if raw_mode:
            # environments hand out raw screen pairs; observations are built on the GPU (DeviceObservations)
            if not all(hasattr(e, "next_raw") and hasattr(e, "initial_raw") for e in self.emulators):
                raise Exception("--device_preprocess needs environments with initial_raw() / next_raw()")
            first = np.stack([emulator.initial_raw() for emulator in self.emulators]).astype(np.uint8)
            variables = [first, np.full(N, first.shape[1], dtype=np.float32), np.zeros(N, dtype=np.float32),
                         np.asarray([False] * N, dtype=np.float32), np.zeros((N, A), dtype=np.float32)]
            variables += [np.zeros(N, dtype=np.float32)] if truncation_on else []
            self.runners = Runners(RawEmulatorRunner, self.emulators, self.workers, variables)
            self.runners.start()
            shared_raw, shared_counts, shared_rewards, shared_episode_over, shared_actions = \
                self.runners.get_shared_variables()[:5]
            observations = DeviceObservations(N, first.shape[1], dev)
            observations.update(shared_raw, shared_counts)
            current_states = lambda: observations.current
        else:
            variables = [(np.asarray([emulator.get_initial_state() for emulator in self.emulators], dtype=np.uint8)),
                         (np.zeros(N, dtype=np.float32)),
                         (np.asarray([False] * N, dtype=np.float32)),
                         (np.zeros((N, A), dtype=np.float32))]
            variables += [np.zeros(N, dtype=np.float32)] if truncation_on else []
            self.runners = Runners(EmulatorRunner, self.emulators, self.workers, variables)
            self.runners.start()
            shared_states, shared_rewards, shared_episode_over, shared_actions = self.runners.get_shared_variables()[:4]
            host_states = torch.from_numpy(shared_states)
            # page-lock the shared observation array in place: the per-step H2D is then one DMA straight out of the
            # memory the emulator workers write, instead of a staged pageable copy
            pinned = hip_ops.pin_host_array(host_states)
            current_states = lambda: host_states

        shared_truncs = self.runners.get_shared_variables()[-1] if truncation_on else None
        truncs = np.zeros((T, N), dtype=np.float32) if truncation_on else None
        d_truncs = torch.zeros((T, N), dtype=torch.float32, device=dev) if truncation_on else None
        emulator_steps = np.zeros(N, dtype=np.int64)
        total_episode_rewards = np.zeros(N, dtype=np.float64)
        d_states = torch.zeros((T, N, 84, 84, 4), dtype=torch.uint8, device=dev)
        d_cur = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        d_actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
        d_values = torch.zeros((T, N), dtype=torch.float32, device=dev)
        d_rewards = torch.zeros((T, N), dtype=torch.float32, device=dev)
        d_masks = torch.zeros((T, N), dtype=torch.float32, device=dev)
        d_probs = torch.zeros((N, A), dtype=torch.float32, device=dev)
        d_vboot = torch.zeros((N,), dtype=torch.float32, device=dev)
        d_y = torch.zeros((T * N,), dtype=torch.float32, device=dev)
        d_adv = torch.zeros((T * N,), dtype=torch.float32, device=dev)
        mt_state = hip_ops.mt_state_from_numpy(np.random.get_state(), dev)
        mt_scratch = hip_ops.sample_mt_scratch(N, A, dev)
        mb_step = torch.zeros((1,), dtype=torch.int64, device=dev)      # --ppo_minibatches: the shuffles' step counter
        # --window_stats: the block (folded eagerly once per cycle, behind the update) and the window's episodes so far
        if self.window_stats and parallel.collectives_active():
            raise ValueError(window_stats.DATA_PARALLEL_REFUSAL)
        self.host_window = hip_ops.window_block(dev) if self.window_stats else None
        rewards = np.zeros((T, N), dtype=np.float32)
        masks = np.zeros((T, N), dtype=np.float32)
        # the sampled action indices come back through a page-locked buffer: an asynchronous copy + an event instead of a
        # synchronising .cpu(), so the host does the previous step's bookkeeping while the GPU runs this step's forward
        h_actions = torch.zeros((N,), dtype=torch.int32).pin_memory()
        actions_ready = torch.cuda.Event()
        env_index = np.arange(N)
        params = self.network.params
        start_time = time.time()
        self.last_feed = None
        metrics = self._open_metrics()
        # data parallel: global_step counts the environment steps of ALL ranks (paac.py:127 counts every environment of
        # the one learner), like the device loop -- lr anneals and max_global_steps ends on the global count
        world = self._world()
        check_every = max(1, int(os.environ.get("PAAC_REPLICA_CHECK_CYCLES", "1024")))

        stock_rescale = type(self).rescale_reward is ActorLearner.rescale_reward

        def bookkeeping(t, step_rewards, step_overs, step_truncs=None):
            """paac.py:119-138 for one step, vectorised over the environments that did not end an episode; the finished
            ones are visited in index order with the global_step the reference's per-environment loop would show them."""
            masks[t] = 1.0 - step_overs
            if step_truncs is not None:
                truncs[t] = step_truncs
            total_episode_rewards[:] += step_rewards
            if stock_rescale:
                rewards[t] = np.clip(step_rewards, -1.0, 1.0)      # rescale_reward, actor_learner.py:95-101
            else:                                                  # a subclass's own rescale_reward, per reward like upstream
                rewards[t] = [self.rescale_reward(r) for r in step_rewards]
            emulator_steps[:] += 1
            before = self.global_step
            self.global_step += N * world
            for e in np.nonzero(step_overs)[0]:
                total_rewards.append(total_episode_rewards[e])
                if self.host_window is not None:
                    self.host_window_episodes[0].append(total_episode_rewards[e])
                    self.host_window_episodes[1].append(emulator_steps[e])
                if metrics is not None:                      # paac.py:130-135
                    metrics.write("episode", global_step=int(before + (e + 1) * world),
                                  reward=float(total_episode_rewards[e]), length=int(emulator_steps[e]))
                total_episode_rewards[e] = 0
                emulator_steps[e] = 0

        # One step's GPU work -- observations H2D, policy forward, numpy-parity sampler, action indices D2H -- as ONE hipGraph
        # launch per step where it can be captured (page-locked shared observations, up to 64 environments on a stock trunk:
        # paac_act_step_mt's sampling-only form, three kernels), instead of seven API calls whose host cost is what this
        # loop is made of; PAAC_HOST_GRAPH=0, or anything that cannot be captured, keeps the eager calls
        fused_act = (N <= hip_ops.ACT_STEP_MAX_ENVS and N * (A - 1) <= hip_ops.ACT_STEP_MAX_DRAWS
                     and getattr(self.network, "ARCH", None) in ("NATURE", "NIPS"))
        host_stream = torch.cuda.Stream(device=dev)
        host_stream.wait_stream(torch.cuda.current_stream(dev))
        step_graphs = [None] * T

        def step_gpu(t):
            d_states[t].copy_(current_states(), non_blocking=True)
            if fused_act:
                self.ctx.act_mt(params, d_states[t], mt_state, d_actions[t], d_probs, d_values[t])
            else:
                self.ctx.forward(params, d_states[t], probs=d_probs, values=d_values[t])
                hip_ops.sample_mt(d_probs, mt_state, mt_scratch, d_actions[t])
            h_actions.copy_(d_actions[t], non_blocking=True)

        if (os.environ.get("PAAC_HOST_GRAPH", "1") != "0" and not raw_mode and pinned and fused_act):
            with torch.cuda.stream(host_stream):
                try:
                    for t in range(T):
                        g = hip_ops.Graph()
                        g.begin()
                        try:
                            step_gpu(t)
                        except Exception:
                            g.abort()
                            raise
                        g.end()
                        step_graphs[t] = g
                except Exception as exc:      # noqa: BLE001 -- a copy or launch the runtime would not record: eager calls
                    logging.debug("host-plugin loop: per-step graph not captured (%s), issuing the calls eagerly", exc)
                    for g in step_graphs:
                        if g is not None:
                            g.close()
                    step_graphs = [None] * T
        ctx_stream = torch.cuda.stream(host_stream)
        ctx_stream.__enter__()          # everything below is issued on the loop's own stream
        while self.global_step < self.max_global_steps and not parallel.any_rank(self.stop_requested, dev):
            loop_start_time = time.time()
            pending = None
            for t in range(T):
                if step_graphs[t] is not None:
                    step_graphs[t].launch()
                else:
                    step_gpu(t)
                actions_ready.record()
                if pending is not None:            # the previous step's records, while the GPU is busy with this step
                    bookkeeping(*pending)
                actions_ready.synchronize()
                shared_actions[...] = 0.0          # one-hot rows (the convention of runners.py: workers take the argmax)
                shared_actions[env_index, h_actions.numpy()] = 1.0
                self.runners.update_environments()
                self.runners.wait_updated()
                if raw_mode:
                    observations.update(shared_raw, shared_counts)
                pending = (t, shared_rewards.astype(np.float32), shared_episode_over.astype(np.float32),
                           shared_truncs.astype(np.float32) if truncation_on else None)
            bookkeeping(*pending)
            d_cur.copy_(current_states())
            self.ctx.forward(params, d_cur, values=d_vboot)
            d_rewards.copy_(torch.from_numpy(rewards))
            d_masks.copy_(torch.from_numpy(masks))
            if truncation_on:
                d_truncs.copy_(torch.from_numpy(truncs))
                self.host_truncated_steps = int(truncs.sum())
            hip_ops.returns(d_vboot, d_rewards, d_masks, d_values, self.gamma, d_y, d_adv, self.gae_lambda, truncs=d_truncs)
            d_actor_adv = d_adv
            if self.adv_norm:         # the actor term reads the normalised advantages; d_adv stays the recorded raw array
                hip_ops.adv_normalize(d_adv, self.adv_n, self.adv_stats)
                d_actor_adv = self.adv_n
            lr = self.get_lr()
            self.lr_dev.fill_(float(np.float32(lr)))
            if self.minibatch_on:
                # --ppo_minibatches: record pass on the pre-update weights, the cycle's shuffles (on the frames each environment
                # has taken so far, the device loop's counter), then K x M optimizer steps on the staged minibatches
                rows, acts = d_states.view(T * N, 84, 84, 4), d_actions.view(-1)
                self.ctx.train_forward_trunk(params, rows)
                self.minibatch_record(acts, T * N)
                mb_step.fill_((counter + 1) * T)
                self.minibatch_perms(getattr(self.args, "sampler_seed", 42), mb_step)
                for k in range(self.ppo_steps):
                    self.minibatch_step_backward(k, rows, acts, d_y, d_actor_adv, phase=0)
                    self._allreduce_grad()
                    self.apply_gradients(k)
            else:
                self.ctx.loss_backward(params, d_states.view(T * N, 84, 84, 4), d_actions.view(-1), d_y, d_actor_adv,
                                       self.entropy_beta, self.grad, self.loss_dev,
                                       p_old_out=self.p_old if self.ppo_epochs > 1 else None)
                if self.vclip_on:         # v_old = the values epoch 1's heads just computed
                    self.ctx.train_values_into(self.v_old, T * N)
                self._allreduce_grad()
                self.apply_gradients(0)
                for k in range(1, self.ppo_epochs):      # epochs 2..K on the frozen y / adv / p_old (/ v_old), the same lr
                    self.ppo_epoch_backward(k, d_states.view(T * N, 84, 84, 4), d_actions.view(-1), d_y, d_actor_adv, phase=0)
                    self._allreduce_grad()
                    self.apply_gradients(k)
            if self.host_window is not None:
                self.window_fold(*self.host_window, d_values, d_rewards, d_masks, d_actions, d_y, d_adv, truncs=d_truncs)
            if getattr(self.args, "record_feeds", False):
                self.last_feed = dict(states=d_states.view(T * N, 84, 84, 4).cpu().numpy(), y=d_y.cpu().numpy(),
                                      adv=d_adv.cpu().numpy(), actions=d_actions.view(-1).cpu().numpy(), lr=lr,
                                      values=d_values.cpu().numpy(), global_step=self.global_step,
                                      rewards=d_rewards.cpu().numpy(), masks=d_masks.cpu().numpy(),
                                      v_boot=d_vboot.cpu().numpy(),
                                      **(dict(truncs=d_truncs.cpu().numpy()) if truncation_on else {}),
                                      # --window_stats: the update's scalars the cycle's fold read (one row per optimizer step)
                                      **(dict(window_loss=self._window_loss_rows(), window_gnorm=self.gnorm_dev.cpu().numpy())
                                         if self.host_window is not None else {}))
                if getattr(self.args, "feed_callback", None):
                    self.args.feed_callback(self.last_feed)
            if getattr(self.args, "cycle_callback", None):      # bench hook: one call per finished cycle, nothing copied
                self.args.cycle_callback(self.global_step)
            counter += 1
            if parallel.collectives_active() and (counter == 1 or counter % check_every == 0):
                ok, same = parallel.replicas_identical([t for _, t in self.update_state])
                if not ok:
                    raise parallel.ReplicaMismatch("data-parallel replicas diverged after %d updates: %s differ between ranks"
                                                   % (counter, ", ".join(n for (n, _), s in zip(self.update_state, same) if not s)))
            if counter % (2048 / self.emulator_counts) == 0:
                curr_time = time.time()
                last_ten = 0.0 if len(total_rewards) < 1 else np.mean(total_rewards[-10:])
                window, window_text = None, ""
                if self.host_window is not None:
                    host_stream.synchronize()
                    window, window_text = self._window_read(*self.host_window, episodes=self.host_window_episodes)
                    self.host_window_episodes = ([], [])
                logging.info("Ran {} steps, at {} steps/s ({} steps/s avg), last 10 rewards avg {}{}"
                             .format(self.global_step, T * N * world / (curr_time - loop_start_time),
                                     (self.global_step - global_step_start) / (curr_time - start_time), last_ten, window_text))
                self._progress_record(T * N * world / (curr_time - loop_start_time),
                                      (self.global_step - global_step_start) / (curr_time - start_time), last_ten)
                if window is not None:
                    self._window_record(window)
            self.save_vars()
        host_stream.synchronize()
        ctx_stream.__exit__(None, None, None)
        for g in step_graphs:
            if g is not None:
                g.close()
        if not raw_mode and pinned:
            hip_ops.unpin_host_array(host_states)      # the stream is drained and the graphs copying from it are gone
        logging.debug("Host-plugin loop: %d update cycles, global step %d", counter, self.global_step)
        np.random.set_state(hip_ops.mt_state_to_numpy(mt_state))

    def _sync_device(self):
        """Everything issued so far has completed -- graph-replayed cycles still running on the rollout's own stream and
        a data-parallel optimizer step still waiting to ride in front of the next cycle included -- so a checkpoint
        taken now holds the weights and the optimizer state (update_state) of one and the same update."""
        if self.rollout is not None:
            self.rollout.synchronize()
        super(PAACLearner, self)._sync_device()

    def cleanup(self):
        super(PAACLearner, self).cleanup()       # save_vars(True) -> _sync_device() first
        if self.runners is not None:
            self.runners.stop()
            self.runners = None
        if self.rollout is not None:
            self.rollout.close()
            if self.rollout.pool is not None:
                self.rollout.pool.close()
        if self.metrics is not None:
            self.metrics.close()
            self.metrics = None
