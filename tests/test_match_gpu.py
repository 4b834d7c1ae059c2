"""-m gpu: head-to-head matches (paac_match_step, match.DeviceMatch, test.py --versus, train.py --eval_match) against their
specification paac_amd/match.py and the numpy twin duel.DuelBoards."""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import duel, evaluation, match

SEED = (0x5EED << 32) + 11           # the match's seed: a non-zero high word
GAME_SEED = 3
A = 6


class Buffers(object):
    """What paac_match_step launches of N rows read and write; state / stack ping-pong between index 0 and 1."""

    def __init__(self, N, env_offset=0, steps=1, dev="cuda"):
        from paac_amd import hip_ops
        self.N, self.env_offset = N, env_offset
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, hip_ops.DUEL_STATE_WORDS), dtype=torch.int32, device=dev) for _ in range(2)]
        self.probs = torch.zeros((steps, N, A), dtype=torch.float32, device=dev)
        self.actions = torch.zeros((steps, N), dtype=torch.int32, device=dev)
        self.score = torch.zeros(N, dtype=torch.float32, device=dev)
        self.length, self.done = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
        self.alive = torch.full((1,), N, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        if N >= 2 and N % 2 == 0:
            hip_ops.duel_reset(GAME_SEED, env_offset, self.states[0], self.stacks[0])

    def match_step(self, greedy, noops, slot=0, parity=0, step_offset=0, seed=SEED):
        from paac_amd import hip_ops
        a, b = parity, parity ^ 1
        hip_ops.match_step(self.probs[slot], greedy, seed, noops, self.step, step_offset, GAME_SEED, self.env_offset,
                           self.states[a], self.states[b], self.stacks[a], self.stacks[b], self.actions[slot], self.score,
                           self.length, self.done, self.alive)

    def accounts(self):
        return (self.score.cpu().numpy(), self.length.cpu().numpy(), self.done.cpu().numpy(), int(self.alive.item()))


def mirrored(records):
    n = len(records) // 2
    return all(tuple(records[b + n][:10]) == duel.mirror(tuple(records[b][:10])) for b in range(n))


def spec_run(N, env_offset, greedy, noops, steps, probs_seed):
    """The specification on fresh Dirichlet rows every step -> per step (probs, actions, records, stacks, score, length, done,
    the rewards that were scored, terminals), the rows' no-op counts and the number of scored episodes decided at five points."""
    n = N // 2
    ids = env_offset + np.arange(n)
    counts = np.tile(evaluation.eval_noops(SEED, ids, noops), 2)
    rs = np.random.RandomState(probs_seed)
    boards = duel.DuelBoards(N, GAME_SEED, env_offset)
    boards.reset()
    score, length, done = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    out, decided = [], 0
    for t in range(steps):
        p = rs.dirichlet(np.ones(A), size=N).astype(np.float32)
        actions = np.where(t < counts, 0, match.match_actions(p, SEED, t, ids, greedy)).astype(np.int32)
        records, stacks, rewards, terminals, truncated = boards.step(actions)
        scored = (t >= counts) & (done == 0)                 # evaluation.account's rule, one step at a time
        score[scored] += rewards[scored]
        length[scored] += 1
        done[scored & terminals] = 1
        decided += int((terminals & ~truncated & scored)[:n].sum())
        out.append((p, actions, records, stacks, score.copy(), length.copy(), done.copy(), rewards * scored, terminals))
    return out, counts, decided


# (N, env_offset, greedy) -> the seed of the Dirichlet rows, chosen on the twin so that within 160 steps every row is done, each
# side has scored a point in a scored episode, and a scored episode was decided at five points (asserted below)
PROBS_SEEDS = {(2, 0, False): 2, (2, 0, True): 5, (6, 4, False): 1, (6, 4, True): 1}


@pytest.mark.parametrize("greedy", [False, True])
@pytest.mark.parametrize("N,env_offset", [(2, 0), (6, 4)])
def test_the_entry_matches_the_specification_step_by_step(N, env_offset, greedy):
    steps, noops, n = 160, 3, N // 2
    want, counts, decided = spec_run(N, env_offset, greedy, noops, steps, PROBS_SEEDS[(N, env_offset, greedy)])
    b = Buffers(N, env_offset)
    twin = duel.DuelBoards(N, GAME_SEED, env_offset)
    records0, stacks0 = twin.reset()
    assert np.array_equal(b.states[0].cpu().numpy(), records0) and np.array_equal(b.stacks[0].cpu().numpy(), stacks0)
    points = []
    for t, (p, actions, records, stacks, score, length, done, r, term) in enumerate(want):
        b.probs[0].copy_(torch.from_numpy(p))
        b.step.fill_(t)
        b.match_step(greedy, noops, parity=t & 1)
        out = (t & 1) ^ 1
        assert np.array_equal(b.actions[0].cpu().numpy(), actions), "step %d: actions" % t
        got = b.states[out].cpu().numpy()
        assert np.array_equal(got, records) and mirrored(got), "step %d: records" % t
        assert np.array_equal(b.stacks[out].cpu().numpy(), stacks), "step %d: stacks" % t          # all four channels
        got = b.accounts()
        assert np.array_equal(got[0], score) and np.array_equal(got[1], length) and np.array_equal(got[2], done), "step %d" % t
        assert got[3] == N - int(done.sum()), "step %d: alive" % t
        points.append(r)
    score, length, done, alive = b.accounts()
    # (account() adds a reward only where the step is scored: the masked rewards give its result)
    for x, y in zip((score, length, done), evaluation.account(np.array(points), np.array([w[8] for w in want]), counts)):
        assert np.array_equal(x, y)
    print("N", N, "greedy", greedy, "noops", counts[:n], "scores", score, "lengths", length, "decided", decided)
    # what the seeds were chosen for
    assert alive == 0 and done.tolist() == [1] * N                                    # every row is done
    points = np.array(points)[:, :n]
    assert (points > 0).any() and (points < 0).any()                                  # each side has scored, in a scored episode
    assert decided >= 1 and (np.abs(score) <= 5).all()                                # an episode was decided at five points
    assert np.array_equal(score[n:], -score[:n]) and np.array_equal(length[n:], length[:n])
    assert len(set(np.array([w[1] for w in want]).reshape(-1).tolist())) == A


def test_a_record_two_steps_short_of_the_cap_is_driven_into_it():
    N = 2
    b = Buffers(N)
    short = (5, 8, 1, 1, 9, 3, 2, 1, 998, 4)                 # steps = 998, the ball in the middle: no point pending
    rows = np.zeros((N, 12), dtype=np.int32)
    rows[0, :10], rows[1, :10] = short, duel.mirror(short)
    b.states[0].copy_(torch.from_numpy(rows))
    twin = duel.DuelBoards(N, GAME_SEED)
    twin.reset()
    twin.rows = [short, duel.mirror(short)]
    twin.stacks = b.stacks[0].cpu().numpy()
    b.probs[0].copy_(torch.from_numpy(np.eye(A, dtype=np.float32)[[0, 0]]))
    for t in range(2):
        b.step.fill_(t)
        b.match_step(False, 0, parity=t & 1)
        records, stacks, rewards, terminals, truncated = twin.step([0, 0])
        assert np.array_equal(b.states[(t & 1) ^ 1].cpu().numpy(), records) and np.array_equal(b.stacks[(t & 1) ^ 1].cpu().numpy(), stacks)
        score, length, done, alive = b.accounts()
        assert terminals.tolist() == [t == 1] * 2 and truncated.tolist() == [t == 1] * 2
        assert done.tolist() == [t] * 2 and alive == (2 if t == 0 else 0) and length.tolist() == [t + 1] * 2
    assert score.tolist() == [0.0, 0.0]                      # terminal at the cap, scored, done
    assert tuple(records[0][:10]) == duel.start_board(GAME_SEED, 0, 5) and not stacks[..., :3].any()
    b.step.fill_(2)                                          # ... and nothing of a done row changes again
    b.match_step(False, 0, parity=0)
    assert b.accounts()[1].tolist() == [2, 2] and b.accounts()[3] == 0


def test_refusals_come_back_as_errors_without_a_launch():
    from paac_amd import _lib, hip_ops
    N = 4
    b = Buffers(N)
    before = (b.states[0].clone(), b.stacks[0].clone())

    def call(**kw):
        a = dict(probs=b.probs[0], greedy=False, eval_seed=1, noops=0, step_base_dev=b.step, step_offset=0, env_seed=1,
                 env_offset=0, state_in=b.states[0], state_out=b.states[1], stack_in=b.stacks[0], stack_out=b.stacks[1],
                 actions_out=b.actions[0], score=b.score, length=b.length, done=b.done, alive=b.alive)
        a.update(kw)
        hip_ops.match_step(**a)

    with pytest.raises(_lib.PaacHipError, match="in place"):
        call(state_out=b.states[0])
    with pytest.raises(_lib.PaacHipError, match="in place"):
        call(stack_out=b.stacks[0])
    for rows in (3, 1, 0):
        with pytest.raises(_lib.PaacHipError, match="N=%d" % rows):
            call(probs=torch.zeros((rows, A), device="cuda"), state_in=b.states[0][:rows], state_out=b.states[1][:rows],
                 stack_in=b.stacks[0][:rows], stack_out=b.stacks[1][:rows], actions_out=b.actions[0][:rows], score=b.score[:rows],
                 length=b.length[:rows], done=b.done[:rows])
    for actions in (3, 5, 7):
        with pytest.raises(_lib.PaacHipError, match="A=%d" % actions):
            call(probs=torch.zeros((N, actions), device="cuda"))
    with pytest.raises(_lib.PaacHipError, match="noops"):
        call(noops=-1)
    with pytest.raises(ValueError):
        call(state_out=torch.zeros((N, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        call(stack_out=b.stacks[1][:2])
    # null pointers, straight at the C entry: the message names the argument
    lib = _lib.load()
    pointers = dict(probs=b.probs[0], state_in=b.states[0], state_out=b.states[1], stack_in=b.stacks[0], stack_out=b.stacks[1],
                    actions_out=b.actions[0], score=b.score, length=b.length, done=b.done, alive=b.alive)
    for missing in pointers:
        p = {k: (None if k == missing else ctypes.c_void_p(v.data_ptr())) for k, v in pointers.items()}
        rc = lib.paac_match_step(p["probs"], N, A, 0, 1, 0, None, 0, 1, 0, p["state_in"], p["state_out"], p["stack_in"],
                                 p["stack_out"], p["actions_out"], p["score"], p["length"], p["done"], p["alive"], None)
        assert rc < 0 and missing in lib.paac_last_error().decode(), missing
    torch.cuda.synchronize()
    assert torch.equal(before[0], b.states[0]) and torch.equal(before[1], b.stacks[0])
    assert not b.states[1].any() and not b.stacks[1].any() and b.accounts()[3] == N          # nothing was launched
    call()                                                                                   # ... and the plain call is fine
    torch.cuda.synchronize()
    assert b.states[1].any()


def test_captured_block_replays_like_the_eager_steps():
    """16 steps in one hipGraph, replayed six times at N = 4: the device step counter moves the no-op phase and both players'
    sampled actions on by itself."""
    from paac_amd import hip_ops
    N, noops, K, blocks = 4, 3, 16, 6
    p = np.random.RandomState(8).dirichlet(np.ones(A), size=(K, N)).astype(np.float32)
    outs = []
    for captured in (False, True):
        b = Buffers(N, steps=K)
        b.probs.copy_(torch.from_numpy(p))

        def block():
            for j in range(K):
                b.match_step(False, noops, slot=j, parity=j & 1, step_offset=j)
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
    # ... and both are the specification: the actions of step t, the twin's accounts
    ids = np.arange(N // 2)
    counts = evaluation.eval_noops(SEED, ids, noops)
    for t in range(K * blocks):
        want = np.where(t < np.tile(counts, 2), 0, match.match_actions(p[t % K], SEED, t, ids, False))
        assert np.array_equal(eager["trace"][t], want), t
    want_score, want_length = match.replay_match(GAME_SEED, 0, eager["trace"], counts)
    assert np.array_equal(eager["accounts"][0], want_score) and np.array_equal(eager["accounts"][1], want_length)
    assert mirrored(eager["states"]) and len(set(eager["trace"][noops:].reshape(-1).tolist())) == A


# -- through networks ------------------------------------------------------------------------------------------------------------
def make_args(emulator, *flags, **kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", emulator, "--arch", "NIPS"] + list(flags))
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_matchtest_")
    args.emulator_workers = 0
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def fresh_network(params_seed):
    from paac_amd import train
    network = train.get_network_and_environment_creator(make_args("duel"))[0]()
    network.initialize(np.random.RandomState(params_seed))
    return network


def build_learner(args, params_seed=0):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(params_seed))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


def x_side(count, rows, swap_sides=False):
    """X's entries of a [2 count] per-row result, in board order."""
    return np.where(match.x_is_bottom(count, swap_sides), rows[:count], rows[count:])


def test_a_device_match_replays_on_the_twin_exactly():
    from paac_amd import hip_ops
    x, y = fresh_network(0), fresh_network(1)
    assert not torch.equal(x.params, y.params)
    ctx = hip_ops.Context(x.arch_id, A, max_batch=2)
    count = 5
    game = match.DeviceMatch(x.params, ctx, y.params, ctx, count, noops=2, seed=SEED, game_seed=GAME_SEED, record=True)
    assert game.chunk == 2 and match.legs(count, game.chunk) == [(0, 2, True), (2, 1, True), (3, 2, False)]
    scores, lengths, trace, counts = game.run()
    game.close()
    assert scores.dtype == np.float32 and scores.shape == (count,) and lengths.dtype == np.int32 and trace.shape[1] == 2 * count
    assert np.array_equal(counts, evaluation.eval_noops(SEED, np.arange(count), 2))
    want_scores, want_lengths = match.replay_match(GAME_SEED, 0, trace, counts)
    assert np.array_equal(scores, x_side(count, want_scores)) and np.array_equal(lengths, x_side(count, want_lengths))
    assert (lengths >= 1).all() and (np.abs(scores) <= 5).all() and scores.any()
    record = game.summary(scores, lengths, 0.5)
    assert record["count"] == count and record["wins"] + record["draws"] + record["losses"] == pytest.approx(1.0)
    assert record["wins"] == float(np.mean(scores > 0)) and record["mean"] == float(np.mean(scores))
    # captured: one graph per (chunk size, offset, leg), the same numbers
    game = match.DeviceMatch(x.params, ctx, y.params, ctx, count, noops=2, seed=SEED, game_seed=GAME_SEED)
    again = game.run()
    assert game.use_graph and len(game.graphs) == 3
    game.close()
    assert np.array_equal(again[0], scores) and np.array_equal(again[1], lengths)
    # the other way round on the other sides: the same boards, seen by Y
    game = match.DeviceMatch(y.params, ctx, x.params, ctx, count, noops=2, seed=SEED, game_seed=GAME_SEED, swap_sides=True)
    other = game.run()
    game.close()
    assert np.array_equal(other[0], -scores) and np.array_equal(other[1], lengths)
    for kwargs in (dict(count=0), dict(count=4097), dict(noops=-1), dict(steps_per_launch=0)):
        with pytest.raises(ValueError):
            match.DeviceMatch(x.params, ctx, y.params, ctx, **dict(dict(count=4), **kwargs))
    ctx.close()


def test_versus_plays_two_training_folders(capsys):
    from paac_amd import hip_ops, logger_utils
    from paac_amd import test as harness
    folders, weights = [], []
    for emulator, params_seed in (("duel", 0), ("rally", 1)):
        args = make_args(emulator, emulator_counts=4, max_local_steps=5, max_global_steps=2 * 4 * 5)
        logger_utils.save_args(args, args.debugging_folder)
        learner = build_learner(args, params_seed)
        learner.train()                                      # two cycles; cleanup() saves the checkpoint
        folders.append(args.debugging_folder)
        weights.append(learner.network.params.clone())
    capsys.readouterr()
    count = 6
    got = harness.main(["-f", folders[0], "--device_environments", "true", "--versus", folders[1], "-tc", str(count), "-np", "4",
                        "--eval_seed", "5"])
    out = capsys.readouterr().out
    contexts = [hip_ops.Context(0, A, max_batch=count) for _ in range(2)]
    game = match.DeviceMatch(weights[0], contexts[0], weights[1], contexts[1], count, noops=4, seed=5, game_seed=5)
    scores, lengths = game.run()
    record = game.summary(scores, lengths, 0.0)
    game.close()
    for ctx in contexts:
        ctx.close()
    assert got.dtype == np.float32 and np.array_equal(got, scores)
    assert "Performed 6 matches: %s vs %s" % (folders[0], folders[1]) in out
    for line in ("Mean: %.2f" % record["mean"], "Min: %.2f" % record["min"], "Max: %.2f" % record["max"], "Std: %.2f" % record["std"],
                 "Wins / Draws / Losses: %.3f / %.3f / %.3f" % (record["wins"], record["draws"], record["losses"]),
                 "Mean length: %.2f" % record["mean_length"]):
        assert line in out, line
    # without --versus everything is as it was: the duel folder is scored as a rally agent against the script
    alone = harness.main(["-f", folders[0], "--device_environments", "true", "-tc", "4", "-np", "4"])
    out = capsys.readouterr().out
    assert alone.shape == (4,) and "Performed 4 tests" in out and "Wins" not in out


def train_run(sampler, eval_match):
    N, T, cycles = 4, 5, 8
    flags = ["-ec", str(N), "--max_local_steps", str(T), "--sampler", sampler, "--eval_every", str(cycles * N * T),
             "--eval_count", "8"] + (["--eval_match", str(eval_match)] if eval_match else [])
    args = make_args("duel", *flags, max_global_steps=cycles * N * T)
    learner = build_learner(args)
    np.random.seed(9)
    learner.train()
    ro = learner.rollout
    path = os.path.join(args.debugging_folder, "metrics.jsonl")
    return dict(learner=learner, params=learner.network.params.cpu().numpy(), slots=[t.cpu().numpy() for _, t in learner.optimizer_state],
                tick=int(ro.tick.item()), mt=ro.mt_state.cpu().numpy() if sampler == "numpy" else None,
                numpy_state=np.random.get_state(), records=[json.loads(line) for line in open(path)], seed=int(args.random_seed) + 1)


@pytest.mark.parametrize("sampler", ["philox", "numpy"])
def test_training_writes_a_match_record_and_is_bit_identical_with_it(sampler):
    from paac_amd import hip_ops
    on, off = train_run(sampler, 4), train_run(sampler, 0)
    assert np.array_equal(on["params"], off["params"])
    assert len(on["slots"]) == 2 and all(np.array_equal(x, y) for x, y in zip(on["slots"], off["slots"]))
    assert on["tick"] == off["tick"] == 40
    assert np.array_equal(on["numpy_state"][1], off["numpy_state"][1]) and on["numpy_state"][2:] == off["numpy_state"][2:]
    if sampler == "numpy":
        assert np.array_equal(on["mt"], off["mt"])
    matches = [r for r in on["records"] if r["kind"] == "match"]
    assert [r["global_step"] for r in matches] == [160] and not [r for r in off["records"] if r["kind"] == "match"]
    record = matches[0]
    assert record["opponent"] == "previous" and record["opponent_global_step"] == 0 and record["count"] == 4
    assert {"greedy", "mean", "min", "max", "std", "mean_length", "seconds", "wins", "draws", "losses"} <= set(record)
    assert record["greedy"] is True and record["wins"] + record["draws"] + record["losses"] == pytest.approx(1.0)
    # the `eval` records are what they are without the flag (but for their wall time)
    evals = [[{k: v for k, v in r.items() if k not in ("seconds", "time")} for r in run["records"] if r["kind"] == "eval"]
             for run in (on, off)]
    assert evals[0] == evals[1] and [r["global_step"] for r in evals[0]] == [160]
    # by hand: the final weights against a second learner's initial weights, on a context of the evaluator's size
    start = build_learner(make_args("duel", "-ec", "4")).network.params
    ctx = hip_ops.Context(on["learner"].network.arch_id, A, max_batch=8)
    game = match.DeviceMatch(on["learner"].network.params, ctx, start, ctx, 4, noops=30, greedy=True, seed=on["seed"],
                             game_seed=on["seed"])
    scores, lengths = game.run()
    game.close()
    ctx.close()
    assert record["mean"] == float(np.mean(scores)) and record["mean_length"] == float(np.mean(lengths))
