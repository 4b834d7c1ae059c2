"""-m gpu: GPU-resident evaluation (paac_eval_step, evaluation.DeviceEvaluator, test.py --device_environments, train.py
--eval_every) against its specification paac_amd/evaluation.py and the games' host twins."""
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import bricks, catch, evaluation

SEED = (0x5EED << 32) + 11           # the evaluation's seed: a non-zero high word
GAME_SEED = (7 << 32) + 2            # the games': catch episodes end inside the no-op phase, always-stay bricks last 24 steps
TWINS = {"catch": catch.CatchEnvironment, "bricks": bricks.BricksEnvironment}


class Creator(object):
    num_actions = 3

    def __init__(self, game, seed):
        self.game, self.seed = game, seed

    def create_environment(self, i):
        return TWINS[self.game](i, seed=self.seed)


class Buffers(object):
    """What paac_eval_step launches of N environments read and write; state / stack ping-pong between index 0 and 1."""

    def __init__(self, game, N, A=3, env_offset=0, game_seed=GAME_SEED, steps=1, dev="cuda"):
        from paac_amd import hip_ops
        from paac_amd.paac import STATEFUL_KINDS
        self.game, self.N, self.env_offset, self.game_seed = game, N, env_offset, game_seed
        kind = STATEFUL_KINDS[game]
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, kind["words"]), dtype=torch.int32, device=dev) for _ in range(2)]
        self.probs = torch.zeros((steps, N, A), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((steps, N), dtype=torch.int32, device=dev)
        self.score = torch.zeros(N, dtype=torch.float32, device=dev)
        self.length, self.done = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
        self.alive = torch.full((1,), N, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        kind["reset"](game_seed, env_offset, self.states[0], self.stacks[0])

    def eval_step(self, greedy, noops, slot=0, parity=0, step_offset=0, seed=SEED):
        from paac_amd import hip_ops
        a, b = parity, parity ^ 1
        hip_ops.eval_step(self.game, self.probs[slot], greedy, seed, noops, self.step, step_offset, self.game_seed, self.env_offset,
                          self.states[a], self.states[b], self.stacks[a], self.stacks[b], self.actions[slot], self.score,
                          self.length, self.done, self.alive)

    def accounts(self):
        return (self.score.cpu().numpy(), self.length.cpu().numpy(), self.done.cpu().numpy(), int(self.alive.item()))


def hand_made_rows(N, rs):
    """[N, 3] float32: a one-hot row, a tie, a row whose running sum stays below every u > 0, uniform rows, then random ones."""
    p = rs.dirichlet(np.ones(3), size=N).astype(np.float32)
    p[0] = (0.0, 1.0, 0.0)
    p[1] = (0.25, 0.375, 0.375)          # greedy tie between 1 and 2
    p[2] = (0.0, 0.0, 0.0)               # falls through to A - 1
    p[3] = p[4] = (1 / 3, 1 / 3, 1 / 3)  # a three-way tie
    if N > 64:
        p[64] = (0.5, 0.5, 0.0)
        p[N - 1] = (0.0, 0.0, 1.0)
    return p


@pytest.mark.parametrize("N", [5, 70])
def test_action_choice_matches_the_specification(N):
    env_offset = 9
    b = Buffers("catch", N, env_offset=env_offset)
    env_ids = env_offset + np.arange(N)
    p = hand_made_rows(N, np.random.RandomState(N))
    b.probs[0].copy_(torch.from_numpy(p))
    seen = set()
    for step in (0, 1, 2 ** 32 + 3):
        b.step.fill_(step - 1)           # the launch reads *step_base + step_offset
        for greedy in (False, True):
            b.eval_step(greedy, noops=0, step_offset=1)
            want = evaluation.eval_action(p, SEED, step, env_ids, greedy)
            got = b.actions[0].cpu().numpy()
            assert np.array_equal(got, want), (step, greedy, got, want)
            seen.update(got.tolist())
            if greedy:
                assert got[:5].tolist() == [1, 1, 0, 0, 0]
            else:
                assert got[0] == 1 and got[2] == 2
    assert seen == {0, 1, 2}
    # no-ops: while t < noops_e the action is 0 whatever the row says
    p[:] = (0.0, 0.0, 1.0)
    b.probs[0].copy_(torch.from_numpy(p))
    noops_e = evaluation.eval_noops(SEED, env_ids, 3)
    for step in (0, 1, 2, 3, 2 ** 32 + 3):
        b.step.fill_(step)
        for greedy in (False, True):
            b.eval_step(greedy, noops=3)
            assert np.array_equal(b.actions[0].cpu().numpy(), np.where(step < noops_e, 0, 2)), (step, greedy)
    assert len(set(noops_e.tolist())) > 1


def twin_step(twins, actions):
    rewards, terminals = evaluation.step_twins(twins, actions)
    return np.stack([np.copy(env.stack) for env in twins]), np.stack([env.state_words() for env in twins]), rewards, terminals


@pytest.mark.parametrize("game", ["catch", "bricks"])
def test_game_and_accounting_match_the_twins(game):
    N, noops, A = 5, 3, 3
    max_steps = evaluation.max_steps_of(game, noops)
    b = Buffers(game, N)
    twins = [TWINS[game](e, seed=GAME_SEED) for e in range(N)]
    assert np.array_equal(b.stacks[0].cpu().numpy(), np.stack([env.get_initial_state() for env in twins]))
    noops_e = evaluation.eval_noops(SEED, np.arange(N), noops)
    rs = np.random.RandomState(5)
    trace, rewards, terminals, alive_seen = [], [], [], []
    frozen = None
    want = (np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32))
    for t in range(max_steps):
        if game == "catch":
            script = rs.randint(0, A, N)
        else:          # always-stay loses its three lives in 24 steps; environment 4 tracks the ball and plays to the step cap
            script = np.array([0, 0, 0, 0, bricks.track_action(twins[4].state)])
        b.probs[0].copy_(torch.from_numpy(np.eye(A, dtype=np.float32)[script]))
        b.step.fill_(t)
        b.eval_step(greedy=bool(t & 1), noops=noops, parity=t & 1)          # a one-hot row: sampled == greedy == its index
        got_actions = b.actions[0].cpu().numpy()
        assert np.array_equal(got_actions, np.where(t < noops_e, 0, script)), "step %d" % t
        want_stacks, want_states, r, term = twin_step(twins, got_actions)
        out = (t & 1) ^ 1
        assert np.array_equal(b.states[out].cpu().numpy(), want_states), "step %d: states" % t
        assert np.array_equal(b.stacks[out].cpu().numpy(), want_stacks), "step %d: stacks" % t
        trace.append(got_actions)
        rewards.append(r)
        terminals.append(term)
        score, length, done, alive = b.accounts()
        scored = (t >= noops_e) & (want[2] == 0)          # the rule, one step at a time (account() restates it on whole traces)
        want[0][scored] += r[scored]
        want[1][scored] += 1
        want[2][scored & term] = 1
        assert np.array_equal(score, want[0]) and np.array_equal(length, want[1]) and np.array_equal(done, want[2]), "step %d" % t
        assert alive == N - int(want[2].sum())
        alive_seen.append(alive)
        if game == "bricks" and alive == 1 and frozen is None:
            frozen = (t, score[:4].copy(), length[:4].copy())
        if alive == 0:
            break
    steps = len(trace)
    score, length, done, alive = b.accounts()
    want_score, want_length = evaluation.replay_on_twins(Creator(game, GAME_SEED), np.array(trace), noops_e)
    assert alive == 0 and done.tolist() == [1] * N
    assert np.array_equal(score, want_score) and np.array_equal(length, want_length)
    for x, y in zip(want, evaluation.account(np.array(rewards), np.array(terminals), noops_e)):
        assert np.array_equal(x, y)
    print(game, "steps", steps, "noops", noops_e, "scores", score, "lengths", length)
    if game == "catch":
        assert steps <= noops + 13 and set(score.tolist()) <= {-1.0, 1.0} and (length <= 13).all()
        # the case the rule is about did occur: a terminal step inside an environment's no-op phase, ignored
        assert any(terminals[t][e] for e in range(N) for t in range(noops_e[e]))
    else:
        # the four always-stay environments (a no-op is a stay: three lives in 24 steps) were done long before the tracking
        # one, which played on alone to the game's step cap -- 500 steps of the game, its no-ops among them
        assert frozen is not None and frozen[0] == 23 and alive_seen[39] == 1 and steps == 500
        assert length[4] == 500 - noops_e[4] and score[4] > 5.0
        assert np.array_equal(score[:4], frozen[1]) and np.array_equal(length[:4], frozen[2])
        assert length[:4].tolist() == (24 - noops_e[:4]).tolist()


@pytest.mark.parametrize("game,blocks", [("catch", 4), ("bricks", 10)])
def test_captured_block_replays_like_the_eager_steps(game, blocks):
    """steps_per_launch = 4 in one hipGraph, replayed: the device step counter moves the no-op phase and the sampled actions
    on by itself.  Fixed, soft probabilities: the actions are sampled on the evaluation's stream."""
    from paac_amd import hip_ops
    N, noops, K = 5, 3, 4
    p = np.random.RandomState(8).dirichlet(np.ones(3), size=(K, N)).astype(np.float32)
    outs = []
    for captured in (False, True):
        b = Buffers(game, N, steps=K)
        b.probs.copy_(torch.from_numpy(p))

        def block():
            for j in range(K):
                b.eval_step(False, noops, slot=j, parity=j & 1, step_offset=j)
            hip_ops.counter_add(b.step, K)

        stream = torch.cuda.Stream()
        trace = []
        with torch.cuda.stream(stream):
            graph = None
            if captured:
                graph = hip_ops.Graph()
                graph.begin()
                block()
                graph.end()
            for _ in range(blocks):
                graph.launch() if captured else block()
                trace.append(b.actions.cpu().numpy().copy())
            stream.synchronize()
            if graph is not None:
                graph.close()
        outs.append(dict(trace=np.concatenate(trace), states=b.states[0].cpu().numpy(), stacks=b.stacks[0].cpu().numpy(),
                         accounts=b.accounts(), step=int(b.step.item())))
    eager, replayed = outs
    assert eager["step"] == replayed["step"] == K * blocks
    for k in ("trace", "states", "stacks"):
        assert np.array_equal(eager[k], replayed[k]), k
    for x, y in zip(eager["accounts"], replayed["accounts"]):
        assert np.array_equal(x, y)
    # ... and both are the specification: the actions of step t, the twins' accounts
    noops_e = evaluation.eval_noops(SEED, np.arange(N), noops)
    for t in range(K * blocks):
        want = np.where(t < noops_e, 0, evaluation.eval_action(p[t % K], SEED, t, np.arange(N), False))
        assert np.array_equal(eager["trace"][t], want), t
    want_score, want_length = evaluation.replay_on_twins(Creator(game, GAME_SEED), eager["trace"], noops_e)
    assert np.array_equal(eager["accounts"][0], want_score) and np.array_equal(eager["accounts"][1], want_length)
    assert len(set(eager["trace"][noops:].reshape(-1).tolist())) == 3


def test_refusals_come_back_as_errors_without_a_launch():
    from paac_amd import _lib, hip_ops
    N = 2
    b = Buffers("bricks", N)
    before = (b.states[0].clone(), b.stacks[0].clone())

    def call(**kw):
        a = dict(game="bricks", probs=b.probs[0], greedy=False, eval_seed=1, noops=0, step_base_dev=b.step, step_offset=0,
                 env_seed=1, env_offset=0, state_in=b.states[0], state_out=b.states[1], stack_in=b.stacks[0],
                 stack_out=b.stacks[1], actions_out=b.actions[0], score=b.score, length=b.length, done=b.done, alive=b.alive)
        a.update(kw)
        hip_ops.eval_step(**a)

    with pytest.raises(_lib.PaacHipError, match="in place"):
        call(state_out=b.states[0])
    with pytest.raises(_lib.PaacHipError, match="in place"):
        call(stack_out=b.stacks[0])
    for A in (1, 33):
        with pytest.raises(_lib.PaacHipError, match="A=%d" % A):
            call(probs=torch.zeros((N, A), device="cuda"))
    with pytest.raises(_lib.PaacHipError, match="noops"):
        call(noops=-1)
    with pytest.raises(_lib.PaacHipError):
        call(probs=torch.zeros((0, 3), device="cuda"), state_in=b.states[0][:0], state_out=b.states[1][:0],
             stack_in=b.stacks[0][:0], stack_out=b.stacks[1][:0])
    with pytest.raises(ValueError):          # a catch record is no bricks record
        call(state_out=torch.zeros((N, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(stack_out=b.stacks[1][:1])
    with pytest.raises(ValueError, match=r"catch\|bricks"):
        call(game="synthetic")
    torch.cuda.synchronize()
    assert torch.equal(before[0], b.states[0]) and torch.equal(before[1], b.stacks[0])
    assert not b.states[1].any() and not b.stacks[1].any() and b.accounts()[3] == N          # nothing was launched
    call()                                                                                   # ... and the plain call is fine
    torch.cuda.synchronize()
    assert b.states[1].any()


# -- through a network ---------------------------------------------------------------------------------------------------------
def catch_args(**kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "catch", "--arch", "NIPS"])
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_evaltest_")
    args.emulator_workers = 0
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def fresh_network(args):
    from paac_amd import train
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    network = network_creator()
    network.initialize(np.random.RandomState(0))
    return network, env_creator


def test_evaluator_replays_on_the_twins_exactly():
    from paac_amd import hip_ops
    network, env_creator = fresh_network(catch_args())
    spec = env_creator.device_env_spec
    assert spec == dict(kind="catch", seed=3)
    ctx = hip_ops.Context(network.arch_id, 3, max_batch=40)
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=33, noops=2, record=True, seed=SEED)      # 33: past the 32-row fc tile
    scores, lengths, trace, noops_e = ev.run()
    assert scores.dtype == np.float32 and scores.shape == (33,) and lengths.dtype == np.int32 and trace.shape[1] == 33
    assert np.array_equal(noops_e, evaluation.eval_noops(SEED, np.arange(33), 2)) and trace.shape[0] <= 16
    want = evaluation.replay_on_twins(env_creator, trace, noops_e)
    assert np.array_equal(scores, want[0]) and np.array_equal(lengths, want[1])
    assert set(scores.tolist()) <= {-1.0, 1.0} and lengths.min() >= 1 and lengths.max() <= 13
    ev.close()
    # greedy, recorded: the same check; greedy through the captured blocks: the same scores, twice
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=33, noops=2, greedy=True, record=True, seed=SEED)
    g_scores, g_lengths, g_trace, _ = ev.run()
    want = evaluation.replay_on_twins(env_creator, g_trace, noops_e)
    assert np.array_equal(g_scores, want[0]) and np.array_equal(g_lengths, want[1])
    ev.close()
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=33, noops=2, greedy=True, seed=SEED, steps_per_launch=4)
    first, second = ev.run(), ev.run()
    assert ev.use_graph and len(ev.graphs) == 1 and ev.launches <= 4
    for x, y, z in zip(first, second, (g_scores, g_lengths)):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    ev.close()
    ctx.close()


def test_evaluator_plays_large_counts_in_chunks():
    from paac_amd import hip_ops
    network, env_creator = fresh_network(catch_args())
    spec = env_creator.device_env_spec
    ctx = hip_ops.Context(network.arch_id, 3, max_batch=16)
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=40, noops=2, record=True, seed=SEED)
    assert ev.chunk == 16
    scores, lengths, trace, noops_e = ev.run()
    assert scores.shape == (40,) and set(scores.tolist()) <= {-1.0, 1.0}
    for offset in (0, 16, 32):          # environment e is game environment e, whatever the chunk
        n = min(16, 40 - offset)
        want = evaluation.replay_on_twins(env_creator, trace[:, offset:offset + n], noops_e[offset:offset + n], env_offset=offset)
        assert np.array_equal(scores[offset:offset + n], want[0]) and np.array_equal(lengths[offset:offset + n], want[1])
    ev.close()
    # captured: one graph per chunk
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=40, noops=2, greedy=True, seed=SEED)
    scores, lengths = ev.run()
    assert len(ev.graphs) == 3 and scores.shape == (40,) and (lengths >= 1).all()
    ev.close()
    for kwargs in (dict(count=0), dict(count=4097), dict(count=4, noops=-1)):
        with pytest.raises(ValueError):
            evaluation.DeviceEvaluator(network, ctx, spec, **dict(dict(count=4), **kwargs))
    with pytest.raises(ValueError, match=r"--emulator catch\|bricks"):
        evaluation.DeviceEvaluator(network, ctx, dict(kind="synthetic", seed=3), count=4)
    ctx.close()


def seeded_learner(args):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(0))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


def test_harness_scores_a_training_folder_on_the_device(capsys):
    from paac_amd import logger_utils
    from paac_amd import test as harness
    args = catch_args(emulator_counts=8, max_local_steps=5, max_global_steps=2 * 8 * 5)
    folder = args.debugging_folder
    logger_utils.save_args(args, folder)
    seeded_learner(args).train()          # two cycles; cleanup() saves the checkpoint
    capsys.readouterr()
    rewards = harness.main(["-f", folder, "--device_environments", "true", "-tc", "48", "-np", "4"])
    out = capsys.readouterr().out
    assert rewards.dtype == np.float32 and rewards.shape == (48,) and set(rewards.tolist()) <= {-1.0, 1.0}
    for label in ("Performed 48 tests", "Mean:", "Min:", "Max:", "Std:", "Mean length:"):
        assert label in out
    # fixed seeds: the same numbers again, and other ones under another seed
    again = harness.main(["-f", folder, "--device_environments", "true", "-tc", "48", "-np", "4", "--eval_seed", "3"])
    assert np.array_equal(rewards, again)
    greedy = harness.main(["-f", folder, "--device_environments", "true", "-tc", "48", "--greedy", "true", "--eval_seed", "5"])
    assert greedy.shape == (48,)
    capsys.readouterr()
    # the host loop is what it was
    rewards = harness.main(["-f", folder, "--device_environments", "false", "-tc", "3", "-np", "5"])
    out = capsys.readouterr().out
    assert rewards.shape == (3,) and "Performed 3 tests" in out and "Mean length" not in out


@pytest.mark.parametrize("sampler", ["philox", "numpy"])
def test_training_is_bit_identical_with_evaluation_on(sampler):
    """12 cycles of 8 catch environments with evaluations at 160, 320 and 480 steps against the same run without: weights,
    optimizer slots, tick and sampler state bit for bit.  The finished-episode ring is compared as its count and its sorted
    entries: the step kernels hand out ring slots with an atomicAdd, so two runs of the SAME command already order the episodes
    of one step differently."""
    runs = []
    for eval_every in (160, 0):
        args = catch_args(emulator_counts=8, max_local_steps=5, max_global_steps=12 * 8 * 5, sampler=sampler,
                          eval_every=eval_every, eval_count=16)
        learner = seeded_learner(args)
        np.random.seed(9)
        learner.train()
        ro = learner.rollout
        runs.append(dict(params=learner.network.params.cpu().numpy(),
                         slots=[t.cpu().numpy() for _, t in learner.optimizer_state],
                         finished=ro.finished_episodes(), tick=int(ro.tick.item()),
                         mt=ro.mt_state.cpu().numpy() if sampler == "numpy" else None,
                         numpy_state=np.random.get_state(), folder=args.debugging_folder))
    on, off = runs
    assert np.array_equal(on["params"], off["params"])
    assert len(on["slots"]) == 2 and all(np.array_equal(x, y) for x, y in zip(on["slots"], off["slots"]))
    # (environments that finish on the same step take their ring slots in the order their workgroups arrive)
    assert on["finished"][0] == off["finished"][0] > 0 and sorted(on["finished"][1]) == sorted(off["finished"][1])
    assert on["tick"] == off["tick"] == 60
    assert np.array_equal(on["numpy_state"][1], off["numpy_state"][1]) and on["numpy_state"][2:] == off["numpy_state"][2:]
    if sampler == "numpy":
        assert np.array_equal(on["mt"], off["mt"])
    records = [json.loads(line) for line in open(os.path.join(on["folder"], "metrics.jsonl"))]
    evals = [r for r in records if r["kind"] == "eval"]
    assert [r["global_step"] for r in evals] == [160, 320, 480]
    for r in evals:
        assert {"global_step", "count", "greedy", "mean", "min", "max", "std", "mean_length", "seconds"} <= set(r)
        assert r["count"] == 16 and r["greedy"] is True and -1.0 <= r["min"] <= r["mean"] <= r["max"] <= 1.0
        assert 1.0 <= r["mean_length"] <= 13.0 and r["seconds"] > 0 and r["std"] >= 0
    off_records = [json.loads(line) for line in open(os.path.join(off["folder"], "metrics.jsonl"))] \
        if os.path.exists(os.path.join(off["folder"], "metrics.jsonl")) else []
    assert not [r for r in off_records if r["kind"] == "eval"]
