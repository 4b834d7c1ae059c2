"""CPU: the match spec (paac_amd/match.py) against evaluation's and duel's, its anchor to rally, the side assignment, the
refusals of --versus and --eval_match, and the C ABI of paac_match_step.  The device side: tests/test_match_gpu.py."""
import argparse
import os
import re

import numpy as np
import pytest

from paac_amd import duel, evaluation, match, rally

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = (0x5EED << 32) + 11           # the match's seed: a non-zero high word
GAME_SEED = 3
A = 6


def hand_made_rows(n, rs):
    """[n, 6] float32: a one-hot row, a greedy tie, a row whose running sum stays below every u > 0, uniform rows, then random
    ones (tests/test_evaluation_gpu.py: hand_made_rows, at six actions)."""
    p = rs.dirichlet(np.ones(A), size=n).astype(np.float32)
    p[0] = (0, 1, 0, 0, 0, 0)
    p[1] = (0.125, 0.25, 0.125, 0.25, 0.125, 0.125)          # greedy tie between 1 and 3
    p[2] = 0.0                                               # falls through to A - 1
    p[3] = p[4] = 1.0 / A                                    # a six-way tie
    return p


def sampled_by_hand(p, seed, step, ids, stream):
    """The sampling rule restated on one stream: the first j < A - 1 with u < the float32 running sum, else A - 1."""
    u = (evaluation.philox_word0(seed, step, ids, stream) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    sums = np.cumsum(p.astype(np.float32), axis=1, dtype=np.float32)[:, :A - 1]
    below = u[:, None] < sums
    return np.where(below.any(axis=1), below.argmax(axis=1), A - 1).astype(np.int32)


def test_the_two_players_draw_from_streams_of_their_own():
    assert match.MATCH_STREAM_TOP == 0x45560003
    assert len({match.MATCH_STREAM_TOP, evaluation.EVAL_STREAM_ACTION, evaluation.EVAL_STREAM_NOOP, 0}) == 4
    n = 40
    ids = 9 + np.arange(n)
    half = hand_made_rows(n, np.random.RandomState(n))
    p = np.concatenate([half, half])                         # identical rows for the two players of every board
    differing = 0
    seen = set()
    for step in (0, 1, 2 ** 32 + 3):
        for greedy in (False, True):
            got = match.match_actions(p, SEED, step, ids, greedy)
            assert got.dtype == np.int32 and got.shape == (2 * n,)
            assert np.array_equal(got[:n], evaluation.eval_action(half, SEED, step, ids, greedy)), (step, greedy)
            if greedy:
                assert np.array_equal(got[n:], got[:n]) and got[:5].tolist() == [1, 1, 0, 0, 0]
            else:
                assert np.array_equal(got[n:], sampled_by_hand(half, SEED, step, ids, match.MATCH_STREAM_TOP)), step
                assert np.array_equal(got[:n], sampled_by_hand(half, SEED, step, ids, evaluation.EVAL_STREAM_ACTION)), step
                assert got[0] == got[n] == 1 and got[2] == got[n + 2] == A - 1
                differing += int((got[n:] != got[:n]).sum())
            seen.update(got.tolist())
    assert differing >= n and seen == set(range(A))          # another stream: other actions on the same rows
    # the high word of the step counts: step 2^32 + 3 is not step 3
    assert not np.array_equal(match.match_actions(p, SEED, 2 ** 32 + 3, ids, False), match.match_actions(p, SEED, 3, ids, False))
    # nothing depends on n or on the chunking: a sub-range of the boards gives the sub-range of the actions
    whole = match.match_actions(p, SEED, 7, ids, False)
    part = match.match_actions(np.concatenate([half[10:20], half[10:20]]), SEED, 7, ids[10:20], False)
    assert np.array_equal(part, np.concatenate([whole[10:20], whole[n + 10:n + 20]]))
    with pytest.raises(ValueError):
        match.match_actions(p[:-1], SEED, 0, ids, False)


def test_no_ops_are_keyed_by_the_board_and_both_rows_play_them():
    n, env_offset, noops = 4, 5, 6
    counts = evaluation.eval_noops(SEED, env_offset + np.arange(n), noops)
    assert len(set(counts.tolist())) > 1 and counts.max() <= noops
    rs = np.random.RandomState(4)
    trace = rs.randint(1, A, size=(260, 2 * n))              # never the no-op itself
    boards = duel.DuelBoards(2 * n, GAME_SEED, env_offset)
    records, _ = boards.reset()
    rewards, terminals = [], []
    for t in range(len(trace)):
        played = np.where(t < np.tile(counts, 2), 0, trace[t])
        before = records
        records, _, r, term, _ = boards.step(played)
        for b in range(n):
            if t < counts[b]:                                # neither paddle of the board moved
                assert records[b][4] == before[b][4] and records[b][5] == before[b][5], (t, b)
                assert records[b + n][4] == before[b + n][4] and records[b + n][5] == before[b + n][5], (t, b)
        rewards.append(r)
        terminals.append(term)
    want = evaluation.account(np.array(rewards), np.array(terminals), np.tile(counts, 2))
    got = match.replay_match(GAME_SEED, env_offset, trace, counts)
    assert want[2].all() and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... and the counts matter: without them the same trace scores other episodes
    other = match.replay_match(GAME_SEED, env_offset, trace, 0)
    assert not np.array_equal(other[1], got[1])


def test_a_replayed_match_is_antisymmetric():
    for n, env_offset, seed in ((1, 0, 3), (3, 4, 3), (5, 1, 8)):
        rs = np.random.RandomState(7 + n)
        counts = rs.randint(0, 6, size=n)
        trace = rs.randint(0, A, size=(300, 2 * n))
        scores, lengths = match.replay_match(seed, env_offset, trace, counts)
        assert scores.dtype == np.float32 and lengths.dtype == np.int32 and scores.shape == lengths.shape == (2 * n,)
        assert np.array_equal(scores[n:], -scores[:n]) and np.array_equal(lengths[n:], lengths[:n])
        assert (lengths > 0).all() and (lengths < 300 - 6).all()          # every board's scored episode did end
        assert (np.abs(scores) <= rally.POINTS).all() and scores.any()


class RallyCreator(object):
    num_actions = A

    def __init__(self, seed):
        self.seed = seed

    def create_environment(self, i):
        return rally.RallyEnvironment(i, seed=self.seed)


@pytest.mark.parametrize("noops", [0, 30])
def test_with_the_script_on_top_a_match_scores_like_rally(noops):
    """Boards 8, 9, 10 of game seed 3, the top rows' trace rally's script of the board at every step, the bottom rows' a mostly
    returning player's: the bottom rows' scores and lengths are evaluation.replay_on_twins of rally on the same bottom trace.
    The scored episode is episode 0, where duel's first serve is rally's.  With 30 no-ops the top player of a match stands still
    where rally's script may move; on these boards the script itself stands still through the 30 steps (checked below: the
    serves go to the bottom player, who loses four points), so the no-op steps are rally's too."""
    n, env_offset = 3, 8
    counts = np.full(n, noops)
    rs = np.random.RandomState(1)
    boards = duel.DuelBoards(2 * n, GAME_SEED, env_offset)
    boards.reset()
    trace = []
    for t in range(noops + rally.MAX_STEPS):
        states = [boards.rows[b] for b in range(n)]
        top = [duel.scripted_top_action(GAME_SEED, env_offset + b, states[b]) for b in range(n)]
        if t < noops:
            assert top == [rally.NOOP] * n, t
        if t == noops:
            assert [s[9] for s in states] == [0] * n          # still episode 0
        bottom = [rally.return_action(states[b]) if rs.rand() < 0.8 else int(rs.randint(A)) for b in range(n)]
        trace.append(bottom + top)
        boards.step(np.where(t < noops, 0, trace[-1]))
    trace = np.array(trace)
    scores, lengths = match.replay_match(GAME_SEED, env_offset, trace, counts)
    want = evaluation.replay_on_twins(RallyCreator(GAME_SEED), trace[:, :n], counts, env_offset=env_offset)
    assert np.array_equal(scores[:n], want[0]) and np.array_equal(lengths[:n], want[1])
    assert np.array_equal(scores[n:], -scores[:n]) and len(set(lengths[:n].tolist())) > 1


def test_sides_are_fixed_by_the_board_index():
    assert match.x_is_bottom(5).tolist() == [True, True, True, False, False]
    assert match.x_is_bottom(4).tolist() == [True, True, False, False]
    assert match.x_is_bottom(1).tolist() == [True]
    assert match.x_is_bottom(5, swap_sides=True).tolist() == [False, False, False, True, True]
    assert match.x_is_bottom(4, swap_sides=True).tolist() == [False, False, True, True]
    # the legs' chunks: board b is board b in any chunking
    assert match.legs(5, 2) == [(0, 2, True), (2, 1, True), (3, 2, False)]
    assert match.legs(5, 2, swap_sides=True) == [(0, 2, False), (2, 1, False), (3, 2, True)]
    assert match.legs(4, 1024) == [(0, 2, True), (2, 2, False)]
    assert match.legs(1, 8) == [(0, 1, True)]
    for count, chunk, swap in ((4096, 1024, False), (7, 3, True), (33, 5, False)):
        sides = np.zeros(count, dtype=bool)
        covered = np.zeros(count, dtype=int)
        for off, n, bottom in match.legs(count, chunk, swap):
            assert 1 <= n <= chunk
            sides[off:off + n] = bottom
            covered[off:off + n] += 1
        assert (covered == 1).all() and np.array_equal(sides, match.x_is_bottom(count, swap))


def train_args(*extra):
    from paac_amd import train
    return train.get_arg_parser().parse_args(list(extra))


def test_eval_match_refusals_name_the_flag():
    from paac_amd import train
    assert train_args().eval_match == 0 and ("--eval_match",) in {f[0] for f in train.BUILD_FLAGS}
    assert match.check_train_flags(train_args()) is False
    assert match.check_train_flags(argparse.Namespace(emulator="duel", eval_every=100)) is False      # an args.json from before
    on = train_args("--emulator", "duel", "--eval_every", "100", "--eval_match", "64")
    assert match.check_train_flags(on) is True and on.eval_match == 64
    assert match.check_train_flags(train_args("--emulator", "duel", "--eval_every", "100", "--eval_match", "4096")) is True
    for extra in (("--eval_match", "-1"), ("--eval_match", "4097")):
        with pytest.raises(ValueError, match="--eval_match"):
            match.check_train_flags(train_args("--emulator", "duel", "--eval_every", "100", *extra))
    with pytest.raises(ValueError, match=r"--eval_match.*--eval_every"):
        match.check_train_flags(train_args("--emulator", "duel", "--eval_match", "8"))
    for emulator in ("rally", "catch", "synthetic"):
        with pytest.raises(ValueError, match=r"--eval_match.*--emulator duel"):
            match.check_train_flags(train_args("--emulator", emulator, "--eval_every", "100", "--eval_match", "8"))
    with pytest.raises(SystemExit):
        train_args("--eval_match", "many")
    # the flag travels through args.json
    import tempfile
    from paac_amd import logger_utils
    folder = tempfile.mkdtemp(prefix="paac_matchargs_")
    logger_utils.save_args(on, folder)
    assert logger_utils.load_args(os.path.join(folder, "args.json"))["eval_match"] == 64


def saved_run(emulator, **kw):
    import tempfile
    from paac_amd import logger_utils
    folder = tempfile.mkdtemp(prefix="paac_versus_%s_" % emulator)
    args = train_args("--emulator", emulator, "--arch", "NIPS")
    for k, v in kw.items():
        setattr(args, k, v)
    logger_utils.save_args(args, folder)
    return folder


def test_versus_refusals_name_the_flag_and_the_folder():
    from paac_amd import test as harness
    cli = harness.get_arg_parser().parse_args(["-f", "a"])
    assert cli.versus is None
    duel_run, rally_run, catch_run = saved_run("duel"), saved_run("rally"), saved_run("catch")
    with pytest.raises(ValueError, match=r"--versus.*--device_environments"):
        harness.main(["-f", duel_run, "--versus", rally_run])
    with pytest.raises(ValueError, match=r"--versus.*--gif_name"):
        harness.main(["-f", duel_run, "--versus", rally_run, "--device_environments", "true", "-gn", "x"])
    with pytest.raises(ValueError, match="test_count"):
        harness.main(["-f", duel_run, "--versus", rally_run, "--device_environments", "true", "-tc", "4097"])
    # a run of another game: refused before the GPU is touched, the folder named
    with pytest.raises(ValueError, match=r"--versus.*%s.*catch" % re.escape(catch_run)):
        harness.main(["-f", duel_run, "--versus", catch_run, "--device_environments", "true"])
    with pytest.raises(ValueError, match=r"--versus.*%s.*catch" % re.escape(catch_run)):
        harness.main(["-f", catch_run, "--versus", duel_run, "--device_environments", "true"])
    # two user architectures need two kernel libraries
    first, second = saved_run("duel", user_arch="32,64,64,1024"), saved_run("rally", user_arch="16,32,256")
    with pytest.raises(ValueError, match=r"--versus.*%s.*--user_arch" % re.escape(second)):
        harness.main(["-f", first, "--versus", second, "--device_environments", "true"])
    runs = [(f, harness.restore_settings(cli, f)) for f in (duel_run, rally_run)]
    harness.check_versus_runs(runs)                          # rally and duel agents may meet, either way round
    harness.check_versus_runs(runs[::-1])
    assert runs[0][1].emulator == "duel" and runs[1][1].emulator == "rally"


def test_the_c_entry_is_declared_and_exported():
    from paac_amd import _lib, hip_ops
    header = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    assert "paac_match_step" in _lib.EXPORTED_SYMBOLS
    declared = re.search(r"\bint paac_match_step\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in declared.split(",")]
    assert names == ["probs", "N", "A", "greedy", "eval_seed", "noops", "step_base_dev", "step_offset", "env_seed", "env_offset",
                     "state_in", "state_out", "stack_in", "stack_out", "actions_out", "score", "length", "done", "alive", "stream"]
    result, arguments = _lib._SIGNATURES["paac_match_step"]
    assert len(arguments) == len(names) == 20 and result is _lib.c_int
    # paac_eval_step's list without `game`, type for type
    assert arguments == _lib._SIGNATURES["paac_eval_step"][1][1:]
    evaluated = re.search(r"\bint paac_eval_step\(([^;]*)\);", header).group(1)
    assert [" ".join(a.split()) for a in declared.split(",")] == [" ".join(a.split()) for a in evaluated.split(",")][1:]
    # an entry of its own, not a fourth evaluation id
    assert not hasattr(_lib, "EVAL_DUEL") and "PAAC_EVAL_DUEL" not in header and set(hip_ops.EVAL_GAMES) == {"catch", "bricks", "rally"}
    with pytest.raises(AttributeError):          # None.dim: the 17 arguments were accepted by position
        hip_ops.match_step(*[None] * 17)


def test_the_top_stream_is_the_kernels_constant():
    source = open(os.path.join(ROOT, "paac_amd", "csrc", "games.hip")).read()
    top = re.search(r"constexpr uint32_t kMatchStreamTop = (0x[0-9A-Fa-f]+)u;", source).group(1)
    assert int(top, 16) == match.MATCH_STREAM_TOP
    for name, value in (("kEvalStreamAction", evaluation.EVAL_STREAM_ACTION), ("kEvalStreamNoop", evaluation.EVAL_STREAM_NOOP)):
        assert int(re.search(r"constexpr uint32_t %s = (0x[0-9A-Fa-f]+)u;" % name, source).group(1), 16) == value
    assert "match_step_kernel" in source and "kMatchStreamTop : kEvalStreamAction" in source
