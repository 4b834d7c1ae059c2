"""GPU-resident evaluation of the device games: many episodes of `--emulator catch|bricks|rally` scored without the host.

This is the SPEC of an evaluation, as catch.py, bricks.py and rally.py are the specs of the games; the same numbers are produced
  * on the host by the plain-numpy functions below (`eval_noops`, `eval_action`, `account`, `replay_on_twins`), and
  * on the device by paac_eval_step (csrc/games.hip; include/paac_hip.h has the contract), one evaluation step of N
    environments per launch, driven by `DeviceEvaluator`.

Spec
  randomness   philox4x32-10 (Salmon et al. 2011) on counter (g, step lo, step hi, stream), key (seed lo, seed hi), g = the
               global environment index, seed = the EVALUATION's seed (not the game's).  The two streams are
               EVAL_STREAM_ACTION and EVAL_STREAM_NOOP: the rollout sampler draws from stream 0 and the minibatch shuffles from
               0x504D0000 + epoch, so an evaluation never shares random words with training, whatever the seeds.
  no-ops       environment g starts with noops_g = word 0 of philox(g, 0, 0, EVAL_STREAM_NOOP) % (noops + 1) no-op steps
               (noops = 0: none) -- the reproducible stand-in for random.randint(0, noops) of the host loop (test.py)
  action       step t < noops_g: the game's no-op, action 0 in every game.  Otherwise, greedy: argmax of the probabilities, the
               lowest index on ties (a NaN row is not a supported input); sampled: the throughput sampler's rule, the first j
               with u < p_0 + .. + p_j on float32 running sums, else A - 1, with u = the 24 high bits of word 0 of
               philox(g, t lo, t hi, EVAL_STREAM_ACTION) * 2^-24
  accounting   the host loop's rule, per environment: rewards and terminals of the no-op steps are ignored (the game resets
               itself there); from t = noops_g on the reward is added to score_g and length_g grows by one, until the first
               terminal step at t >= noops_g, whose reward is included; then done_g = 1 and nothing of g changes again
  bound        max_steps = noops + the game's longest episode (paac.STATEFUL_KINDS: 13 for catch, 500 for bricks, 1000 for rally): every
               environment is done by then; a smaller max_steps given by hand leaves done_g = 0
  game         the games' own specs, single_life off (test.py's restore_settings forces it off too); environment g of an
               evaluation is game environment g of the game seed, whatever the chunking
"""
import time

import numpy as np

EVAL_STREAM_ACTION = 0x45560001        # csrc/games.hip: kEvalStreamAction
EVAL_STREAM_NOOP = 0x45560002          # csrc/games.hip: kEvalStreamNoop
MAX_COUNT = 4096                       # environments of one evaluation
MAX_CHUNK = 1024                       # ... of one acting forward of it

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def philox_word0(seed, step, env_ids, stream):
    """Word 0 of philox4x32-10 on counter (env, step lo, step hi, stream), key (seed lo, seed hi) -> uint32 per environment."""
    env = np.asarray(env_ids).astype(np.uint64) & _MASK
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    c0, c1 = env, np.full(env.shape, step & 0xFFFFFFFF, dtype=np.uint64)
    c2, c3 = np.full(env.shape, step >> 32, dtype=np.uint64), np.full(env.shape, int(stream) & 0xFFFFFFFF, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0.astype(np.uint32)


def eval_noops(seed, env_ids, noops):
    """-> int32 per environment: the no-op steps environment g plays first, in 0..noops."""
    noops = int(noops)
    if noops < 0:
        raise ValueError("noops %d is negative" % noops)
    env_ids = np.asarray(env_ids)
    if noops == 0:
        return np.zeros(env_ids.shape, dtype=np.int32)
    return (philox_word0(seed, 0, env_ids, EVAL_STREAM_NOOP) % np.uint32(noops + 1)).astype(np.int32)


def eval_action(probs_f32, seed, step, env_ids, greedy):
    """-> int32 [N]: the action of every row of probs_f32 [N, A] at step `step` (past its no-ops)."""
    p = np.asarray(probs_f32, dtype=np.float32)
    N, A = p.shape
    if greedy:
        return np.argmax(p, axis=1).astype(np.int32)
    u = (philox_word0(seed, step, env_ids, EVAL_STREAM_ACTION) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    acts = np.full(N, A - 1, dtype=np.int32)
    chosen = np.zeros(N, dtype=bool)
    c = np.zeros(N, dtype=np.float32)
    for j in range(A - 1):
        c = (c + p[:, j]).astype(np.float32)
        hit = (~chosen) & (u < c)
        acts[hit] = j
        chosen |= hit
    return acts


def account(rewards, terminals, noops, max_steps=None):
    """The accounting rule on recorded rewards / terminals [steps, N] and per-environment no-op counts [N] ->
    (score float32 [N], length int32 [N], done int32 [N]); max_steps (default: all recorded steps) ends the loop."""
    rewards, terminals = np.asarray(rewards, dtype=np.float32), np.asarray(terminals).astype(bool)
    steps, N = rewards.shape
    noops = np.broadcast_to(np.asarray(noops, dtype=np.int64), (N,))
    score, length, done = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    for t in range(steps if max_steps is None else min(steps, int(max_steps))):
        scored = (t >= noops) & (done == 0)
        score[scored] += rewards[t][scored]
        length[scored] += 1
        done[scored & terminals[t]] = 1
    return score, length, done


def step_twins(environments, actions):
    """One step of host twins on action indices -> (rewards float32 [N], terminals bool [N]); a twin that ends its episode shows
    its next start state with an empty history, as the device game does (the runner's get_initial_state())."""
    rewards, terminals = np.zeros(len(environments), dtype=np.float32), np.zeros(len(environments), dtype=bool)
    for e, (env, a) in enumerate(zip(environments, actions)):
        _, rewards[e], terminals[e] = env.next(np.eye(env.num_actions)[int(a)])
        if terminals[e]:
            env.get_initial_state()
    return rewards, terminals


def replay_on_twins(env_creator, actions_trace, noops, env_offset=0):
    """Steps the host twins env_creator.create_environment(env_offset + e) through a recorded [steps, N] action trace under
    the accounting rule (the no-op wherever t < noops_e, whatever the trace holds) -> (scores float32 [N], lengths int32 [N]).
    noops: the per-environment no-op counts [N] (or one count for all)."""
    trace = np.asarray(actions_trace)
    steps, N = trace.shape
    noops = np.broadcast_to(np.asarray(noops, dtype=np.int64), (N,))
    environments = [env_creator.create_environment(int(env_offset) + e) for e in range(N)]
    for env in environments:
        env.get_initial_state()
    rewards, terminals = np.zeros((steps, N), dtype=np.float32), np.zeros((steps, N), dtype=bool)
    for t in range(steps):
        rewards[t], terminals[t] = step_twins(environments, np.where(t < noops, 0, trace[t]))
    score, length, _ = account(rewards, terminals, noops)
    return score, length


def max_steps_of(kind, noops):
    """noops + the longest episode of game `kind` (paac.STATEFUL_KINDS, then the user's game: paac.USER_KINDS)."""
    from .paac import stateful_kind
    return int(noops) + int(stateful_kind(kind)["max_episode_steps"])


def check_count(count, what="count"):
    if isinstance(count, bool) or int(count) != count or not 1 <= int(count) <= MAX_COUNT:
        raise ValueError("%s %r: expected an integer in [1, %d]" % (what, count, MAX_COUNT))
    return int(count)


def check_env_spec(env_spec):
    """The device games an evaluation can play, or a ValueError naming them."""
    from .paac import stateful_kind
    kind = None if env_spec is None else env_spec.get("kind", "synthetic")
    if stateful_kind(kind) is None:
        raise ValueError("device evaluation plays the games resident on the GPU only: --emulator catch|bricks|rally (got %s; the "
                         "synthetic reward is a hash, and ALE or user plugins are stepped on the host)"
                         % ("a host-only environment" if kind is None else "'%s'" % kind))
    return kind


def check_train_flags(args, world_size=1):
    """Start-up refusals of --eval_every / --eval_count / --eval_greedy (train.py); old Namespaces without the fields: off."""
    every = getattr(args, "eval_every", 0)
    if isinstance(every, bool) or int(every) != every or int(every) < 0:
        raise ValueError("eval_every %r: expected a step count >= 0 (0 = off)" % (every,))
    if int(every) == 0:
        return False
    check_count(getattr(args, "eval_count", 64), "eval_count")
    if getattr(args, "host_environments", False):
        raise ValueError("--eval_every evaluates on the device games: it cannot be combined with --host_environments true")
    # (duel: a paired game, evaluated as rally against the scripted opponent -- paac.eval_env_spec)
    # (user: a game compiled in through --device_game, paac_amd/user_game.py)
    if getattr(args, "emulator", "synthetic") not in ("catch", "bricks", "rally", "duel", "user"):
        raise ValueError("--eval_every needs a game resident on the GPU: --emulator catch|bricks|rally (got '%s')"
                         % getattr(args, "emulator", "synthetic"))
    if int(world_size) > 1:
        raise ValueError("--eval_every is not built for data-parallel runs (world size %d): evaluate the checkpoints with "
                         "python -m paac_amd.test --device_environments true" % int(world_size))
    return True


class DeviceDriver(object):
    """What DeviceEvaluator and match.DeviceMatch share: `count` boards of a device game, one scored episode each, played in
    chunks on buffers of the largest chunk's rows (rows_per_board rows a board) -- blocks of `block` steps, one hipGraph per
    chunk when use_graph, until the chunk's `alive` count, the one int32 that crosses to the host per block, reaches zero.

    A chunk is a tuple (boards n, env_offset, ...) and the key of its captured block.  A subclass sets max_steps and supplies
    _chunks() -> the chunks of a run, _reset(*chunk), _block(*chunk) = `block` steps issued on the current stream,
    _scored_rows(*chunk) -> the rows whose score / length are the boards', and _place_trace(full, trace, *chunk)."""

    rows_per_board = 1

    def __init__(self, hip_ops, count, noops, seed, greedy, steps_per_launch, record, use_graph):
        self.count = check_count(count)
        if isinstance(noops, bool) or int(noops) != noops or int(noops) < 0:
            raise ValueError("noops %r: expected an integer >= 0" % (noops,))
        if int(steps_per_launch) < 1:
            raise ValueError("steps_per_launch %r: expected a positive integer" % (steps_per_launch,))
        self.hip_ops = hip_ops
        self.noops, self.greedy, self.seed, self.record = int(noops), bool(greedy), int(seed), bool(record)
        self.block = (int(steps_per_launch) + 1) // 2 * 2
        self.use_graph = bool(use_graph) and not self.record
        self.graphs = {}                                   # chunk -> the captured block
        self.launches = 0                                  # blocks issued by the last run()

    def _allocate(self, chunk, words, num_actions, dev, stream):
        """The buffers of chunks of up to `chunk` boards: ping-pong stacks and state records, one block of actions, the accounts."""
        import torch
        self.chunk = chunk
        rows = chunk * self.rows_per_board
        self.stacks = [torch.zeros((rows, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((rows, words), dtype=torch.int32, device=dev) for _ in range(2)]
        self.probs = torch.zeros((rows, num_actions), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((self.block, rows), dtype=torch.int32, device=dev)
        self.score = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.length = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.done = torch.zeros(rows, dtype=torch.int32, device=dev)
        self.alive = torch.zeros(1, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stream = stream if stream is not None else torch.cuda.Stream(device=dev)

    def _captured(self, chunk):
        if chunk not in self.graphs:
            g = self.hip_ops.Graph()
            g.begin()
            try:
                self._block(*chunk)
            except Exception:
                g.abort()
                raise
            g.end()
            self.graphs[chunk] = g
        return self.graphs[chunk]

    def run(self):
        """-> (scores float32 [count], lengths int32 [count]) in board order; with record=True also the action trace int32
        [steps, rows_per_board * count] (zero where a chunk had stopped earlier) and the per-board no-op counts int32 [count]."""
        import torch
        scores, lengths = np.zeros(self.count, dtype=np.float32), np.zeros(self.count, dtype=np.int32)
        traces = []
        self.launches = 0
        with torch.cuda.stream(self.stream):
            for chunk in self._chunks():
                n, env_offset = chunk[:2]
                rows = n * self.rows_per_board
                self._reset(*chunk)
                for t in (self.score, self.length, self.done, self.step):
                    t.zero_()
                self.alive.fill_(rows)
                trace, steps = [], 0
                while steps < self.max_steps:
                    if self.use_graph:
                        self._captured(chunk).launch()
                    else:
                        self._block(*chunk)
                    steps += self.block
                    self.launches += 1
                    if self.record:
                        trace.append(self.actions[:, :rows].cpu().numpy().copy())
                    if int(self.alive.cpu().item()) == 0:          # (synchronises the stream: the block has run)
                        break
                mine = self._scored_rows(*chunk)
                scores[env_offset:env_offset + n] = self.score[mine].cpu().numpy()
                lengths[env_offset:env_offset + n] = self.length[mine].cpu().numpy()
                traces.append((chunk, np.concatenate(trace) if trace else None))
        if not self.record:
            return scores, lengths
        full = np.zeros((max(len(t) for _, t in traces), self.rows_per_board * self.count), dtype=np.int32)
        for chunk, t in traces:
            self._place_trace(full, t, *chunk)
        return scores, lengths, full, eval_noops(self.seed, np.arange(self.count), self.noops)

    def timed_run(self):
        """run() with its wall time -> (scores, lengths, seconds)."""
        start = time.time()
        scores, lengths = self.run()[:2]
        return scores, lengths, time.time() - start

    def close(self):
        for g in self.graphs.values():
            g.close()
        self.graphs = {}


class DeviceEvaluator(DeviceDriver):
    """Scores `count` environments of a device game, one episode each, with the policy of `network` -- nothing crosses to the
    host but one int32 per block of steps.

    network: its live `params` are read at every run().  ctx: a hip_ops.Context of the network's geometry that this evaluator
    may use freely (its acting forwards only); count above ctx.max_batch (or MAX_CHUNK) is played in chunks of that many
    environments, env_offset advancing -- environment e is always game environment e of seed env_spec["seed"].  Scores need not
    be bit-identical across chunk sizes: the acting forward picks different tile routes at different batches, and a
    probability that differs in the last place can turn a sampled action or break a greedy tie.  seed: the evaluation's own
    (no-ops and sampled actions).  steps_per_launch: forward + evaluation steps per block (made even: the ping-pong closes),
    one hipGraph per block when use_graph; record=True runs eagerly and keeps the action trace.  stream: the torch stream
    everything is issued on (default: one of its own).  sticky_p (paac_amd/sticky.py): above 0 the games execute sticky actions
    on the evaluation's own stream, keyed by `seed` -- a plane of previous actions ping-pongs beside the state records inside
    the block, and the trace keeps the CHOSEN actions (replay_on_twins over wrapped twins reproduces the scores); 0: today's
    entry and today's numbers."""

    def __init__(self, network, ctx, env_spec, count, noops=30, greedy=False, seed=0, steps_per_launch=16, record=False,
                 use_graph=True, stream=None, sticky_p=0.0):
        from . import hip_ops
        from .paac import stateful_kind
        self.kind = check_env_spec(env_spec)
        super(DeviceEvaluator, self).__init__(hip_ops, count, noops, seed, greedy, steps_per_launch, record, use_graph)
        if ctx.num_actions != network.num_actions or ctx.arch != network.arch_id:
            raise ValueError("the context was not made for this network")
        self.network, self.ctx = network, ctx
        self.game = stateful_kind(self.kind)
        self.env_seed = int(env_spec["seed"])
        self.max_steps = max_steps_of(self.kind, self.noops)
        self._allocate(min(self.count, ctx.max_batch, MAX_CHUNK), self.game["words"], network.num_actions, network.torch_device,
                       stream)
        from . import sticky
        self.sticky_p = sticky.check_p(sticky_p, "sticky_p")
        self.prev = None
        if self.sticky_p > 0.0:
            import torch
            self.prev = [torch.zeros(self.chunk, dtype=torch.int32, device=network.torch_device) for _ in range(2)]

    def _chunks(self):
        return [(min(self.chunk, self.count - env_offset), env_offset) for env_offset in range(0, self.count, self.chunk)]

    def _reset(self, n, env_offset):
        self.game["reset"](self.env_seed, env_offset, self.states[0][:n], self.stacks[0][:n])
        if self.prev is not None:
            self.prev[0].zero_()

    def _block(self, n, env_offset):
        """`block` x [acting forward -> evaluation step] on the first n environments, then the step counter moves on."""
        ops = self.hip_ops
        for j in range(self.block):
            a, b = j & 1, (j & 1) ^ 1
            self.ctx.forward(self.network.params, self.stacks[a][:n], probs=self.probs[:n])
            if self.prev is not None:
                ops.eval_step_sticky(self.kind, self.sticky_p, self.prev[a][:n], self.prev[b][:n], self.probs[:n], self.greedy,
                                     self.seed, self.noops, self.step, j, self.env_seed, env_offset, self.states[a][:n],
                                     self.states[b][:n], self.stacks[a][:n], self.stacks[b][:n], self.actions[j][:n],
                                     self.score[:n], self.length[:n], self.done[:n], self.alive)
                continue
            ops.eval_step(self.kind, self.probs[:n], self.greedy, self.seed, self.noops, self.step, j, self.env_seed, env_offset,
                          self.states[a][:n], self.states[b][:n], self.stacks[a][:n], self.stacks[b][:n], self.actions[j][:n],
                          self.score[:n], self.length[:n], self.done[:n], self.alive)
        ops.counter_add(self.step, self.block)

    def _scored_rows(self, n, env_offset):
        return slice(0, n)

    def _place_trace(self, full, trace, n, env_offset):
        full[:len(trace), env_offset:env_offset + n] = trace

    def summary(self, scores, lengths, seconds):
        """The fields of an `eval` record of metrics.jsonl (without global_step)."""
        record = dict(count=self.count, greedy=self.greedy, mean=float(np.mean(scores)), min=float(np.min(scores)),
                      max=float(np.max(scores)), std=float(np.std(scores)), mean_length=float(np.mean(lengths)),
                      seconds=float(seconds))
        if self.sticky_p > 0.0:
            record["sticky_action_p"] = self.sticky_p          # (only named when on: the records of P = 0 are today's)
        return record
