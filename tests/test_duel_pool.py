"""CPU: the pooled duel spec (paac_amd/duel_pool.py) -- the split twin against duel's, its anchor to rally, the ghost's action
rule and stream, the pool's schedule, the flags' refusals and the C ABI.  The device side: tests/test_duel_pool_gpu.py."""
import argparse
import os
import re
import tempfile

import numpy as np
import pytest

from paac_amd import duel, duel_pool, evaluation, match, rally

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3


def test_the_pooled_twin_is_duels_split():
    """8 boards x 1500 random steps: the learner half equals the bottom rows of DuelBoards(16), the ghost observations its
    top rows -- records, observations, rewards, terminals, truncation flags, after the reset and after every step."""
    n, steps, env_offset = 8, 1500, 2
    pooled, whole = duel_pool.PooledBoards(n, SEED, env_offset), duel.DuelBoards(2 * n, SEED, env_offset)
    records, stacks, ghosts = pooled.reset()
    want_records, want_stacks = whole.reset()
    assert np.array_equal(records, want_records[:n]) and np.array_equal(stacks, want_stacks[:n])
    assert np.array_equal(ghosts, want_stacks[n:]) and ghosts.any()
    rng = np.random.RandomState(0)
    terminals = 0
    for step in range(steps):
        a = rng.randint(6, size=2 * n)
        records, stacks, ghosts, rewards, term, trunc = pooled.step(a[:n], a[n:])
        w_records, w_stacks, w_rewards, w_term, w_trunc = whole.step(a)
        assert np.array_equal(records, w_records[:n]) and np.array_equal(stacks, w_stacks[:n]), step
        assert np.array_equal(ghosts, w_stacks[n:]), step
        assert np.array_equal(rewards, w_rewards[:n]) and np.array_equal(term, w_term[:n]) and np.array_equal(trunc, w_trunc[:n])
        # the ghost's record is never kept: it is the mirror of the learner's
        assert all(tuple(w_records[b + n][:10]) == duel.mirror(tuple(records[b][:10])) for b in range(n))
        terminals += int(term.sum())
    assert terminals >= n
    with pytest.raises(ValueError):
        duel_pool.PooledBoards(0, SEED)
    with pytest.raises(ValueError):
        pooled.step(np.zeros(n), np.zeros(n - 1))


def test_with_the_script_as_the_ghost_the_learner_rows_are_rally():
    """The ghost playing rally's scripted opponent: the learner rows' rewards, terminals and truncation flags are rally's step,
    and so is the record after a non-terminal step (tests/test_duel.py's anchor, through the pooled twin)."""
    n = 4
    pooled = duel_pool.PooledBoards(n, SEED)
    records, _, _ = pooled.reset()
    rng = np.random.RandomState(1)
    states = [rally.start_state(SEED, g, 0) for g in range(n)]
    assert [tuple(r[:10]) for r in records] == states
    ended = 0
    for step in range(1200):
        a = rng.randint(6, size=n)
        ghost = [duel.scripted_top_action(SEED, g, states[g]) for g in range(n)]
        records, _, _, rewards, term, trunc = pooled.step(a, ghost)
        for g in range(n):
            want_state, want_reward, want_terminal, want_truncated = rally.step_state_truncated(SEED, g, states[g], int(a[g]))
            assert (rewards[g], term[g], trunc[g]) == (want_reward, want_terminal, want_truncated), (step, g)
            if want_terminal:
                ended += 1
                states[g] = tuple(int(v) for v in records[g][:10])          # duel's next episode (its serve alternates)
                assert states[g] == duel.start_board(SEED, g, want_state[9])
            else:
                assert tuple(records[g][:10]) == want_state, (step, g)
                states[g] = want_state
    assert ended >= 4


def test_the_ghost_action_rule_and_its_stream():
    ids = np.arange(4) + 7
    # hand-made rows: a certain action, the last action by exhaustion, a zero row, a split row
    p = np.array([[0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0], [0.5, 0, 0, 0.5, 0, 0]], dtype=np.float32)
    seen = set()
    for tick in list(range(40)) + [(1 << 32) + 5, (1 << 40) + 1]:
        a = duel_pool.ghost_actions(p, 42, tick, ids)
        assert a.dtype == np.int32 and a[0] == 2 and a[1] == 5 and a[2] == 5 and a[3] in (0, 3)
        seen.add(int(a[3]))
        # the inverse CDF on the stream's own word
        u = (evaluation.philox_word0(42, tick, ids, duel_pool.GHOST_STREAM) >> np.uint32(8)).astype(np.float32) / np.float32(16777216.0)
        assert a[3] == (0 if u[3] < np.float32(0.5) else 3)
    assert seen == {0, 3}
    # past 2^32 the high word of the tick counts
    lo, hi = 5, (1 << 32) + 5
    assert not np.array_equal(evaluation.philox_word0(42, lo, ids, duel_pool.GHOST_STREAM),
                              evaluation.philox_word0(42, hi, ids, duel_pool.GHOST_STREAM))
    # match_actions' top rule, given that stream: one body (match.sampled_on_stream)
    rs = np.random.RandomState(2)
    for tick in (0, 9, (1 << 33) + 1):
        rows = rs.dirichlet(np.ones(6), size=8).astype(np.float32)
        top = match.match_actions(rows, 42, tick, ids, False)[4:]
        assert np.array_equal(top, match.sampled_on_stream(rows[4:], 42, tick, ids, match.MATCH_STREAM_TOP))
        assert np.array_equal(duel_pool.ghost_actions(rows[4:], 42, tick, ids),
                              match.sampled_on_stream(rows[4:], 42, tick, ids, duel_pool.GHOST_STREAM))
        # ... and eval_action's own rule on the evaluation stream is the same body
        assert np.array_equal(evaluation.eval_action(rows[:4], 42, tick, ids, False),
                              match.sampled_on_stream(rows[:4], 42, tick, ids, evaluation.EVAL_STREAM_ACTION))
    # no word shared with the rollout sampler's stream 0, the evaluation streams or the match's
    streams = [0, evaluation.EVAL_STREAM_ACTION, evaluation.EVAL_STREAM_NOOP, match.MATCH_STREAM_TOP, duel_pool.GHOST_STREAM,
               duel_pool.POOL_STREAM_LATEST, duel_pool.POOL_STREAM_SLOT]
    assert len(set(streams)) == len(streams)
    many = np.arange(64)
    words = [evaluation.philox_word0(42, t, many, s) for s in streams for t in range(16)]
    flat = np.concatenate(words)
    assert len(set(flat.tolist())) == flat.size
    with pytest.raises(ValueError):
        duel_pool.ghost_actions(p, 42, 0, np.arange(3))


def test_the_stream_is_the_kernels_constant():
    source = open(os.path.join(ROOT, "paac_amd", "csrc", "games.hip")).read()
    assert int(re.search(r"constexpr uint32_t kGhostStream = (0x[0-9A-Fa-f]+)u;", source).group(1), 16) == duel_pool.GHOST_STREAM
    assert (duel_pool.GHOST_STREAM, duel_pool.POOL_STREAM_LATEST, duel_pool.POOL_STREAM_SLOT) == (0x44500001, 0x44500002, 0x44500003)


def spec_draw(seed, j, P, slot, size):
    """The issue's rule, restated: -> (opponent slot, latest)."""
    u = (int(evaluation.philox_word0(seed, j, 0, 0x44500002)) >> 8) / 2.0 ** 24
    if u < P:
        return slot, True
    return int(evaluation.philox_word0(seed, j, 0, 0x44500003)) % size, False


def test_the_schedule_slots_sizes_and_draws():
    every = 640
    # K = 1: one slot, always the newest whatever P says
    s = duel_pool.PoolSchedule(1, every, 0.0, SEED)
    assert s.tags == [0] and s.opponent_slot == 0 and s.size == 1 and s.next_event == every and not s.due(every - 1)
    for j in range(1, 5):
        assert s.due(j * every)
        r = s.event(j * every)
        assert (r["slot"], r["size"], r["opponent_slot"], r["opponent_global_step"]) == (0, 1, 0, j * every)
    # K = 3 over 8 events: slot j % 3, size min(j + 1, 3), the draws by the rule
    s = duel_pool.PoolSchedule(3, every, 0.5, SEED)
    tags, latest_seen = {0: 0}, set()
    for j in range(1, 9):
        r = s.event(j * every)
        tags[j % 3] = j * every
        size = min(j + 1, 3)
        want_slot, want_latest = spec_draw(SEED, j, 0.5, j % 3, size)
        assert r == dict(global_step=j * every, event=j, slot=j % 3, size=size, opponent_slot=want_slot,
                         opponent_global_step=tags[want_slot], latest=want_latest), j
        assert s.next_event == (j + 1) * every and s.size == size
        latest_seen.add(want_latest)
    assert latest_seen == {True, False}
    # P = 1: always the slot just written; P = 0: never by the first draw (the second may still land on it)
    s1, s0 = duel_pool.PoolSchedule(4, every, 1.0, SEED), duel_pool.PoolSchedule(4, every, 0.0, SEED)
    for j in range(1, 10):
        r1, r0 = s1.event(j * every), s0.event(j * every)
        assert r1["latest"] is True and r1["opponent_slot"] == j % 4 and r1["opponent_global_step"] == j * every
        assert r0["latest"] is False and r0["opponent_slot"] == int(evaluation.philox_word0(SEED, j, 0, 0x44500003)) % min(j + 1, 4)
    # determinism in random_seed: the same seed the same records, another seed other draws
    def run(seed):
        return duel_pool.schedule(0, 20, 40 * every, 8, every, 0.5, seed)
    assert run(3) == run(3) and len(run(3)) == 40
    assert [r["opponent_slot"] for r in run(3)] != [r["opponent_slot"] for r in run(4)]
    assert [(r["slot"], r["size"]) for r in run(3)] == [(r["slot"], r["size"]) for r in run(4)]
    # every opponent is a pushed step
    pushed = {0} | {r["global_step"] for r in run(3)}
    assert all(r["opponent_global_step"] in pushed for r in run(3))


def test_event_positions():
    # -ec 32, T = 5: 2048 / 32 is integral, 160 steps per cycle divide 102400: exactly there
    assert [duel_pool.event_step(0, 160, j, 102400) for j in (1, 2, 3)] == [102400, 204800, 307200]
    # -ec 6, T = 5: 2048 / 6 is not integral -- every cycle is a chunk boundary; 30 does not divide 640
    assert [duel_pool.event_step(0, 30, j, 640) for j in (1, 2, 3)] == [660, 1290, 1920]
    assert duel_pool.until_pool(640, 0, 30) == 22 and duel_pool.until_pool(640, 630, 30) == 1 and duel_pool.until_pool(640, 660, 30) == 1
    records = duel_pool.schedule(0, 30, 2000, 3, 640, 0.5, SEED)
    assert [r["global_step"] for r in records] == [660, 1290, 1920] and [r["event"] for r in records] == [1, 2, 3]
    # a resumed run: a fresh pool from the restored weights, tagged with that step, the events where they would have been
    resumed = duel_pool.PoolSchedule(3, 640, 0.5, SEED, start_step=1300)
    assert resumed.size == 1 and resumed.tags[resumed.opponent_slot] == 1300 and resumed.next_event == 1920
    records = duel_pool.schedule(1300, 20, 3300, 3, 640, 0.5, SEED)
    assert [r["global_step"] for r in records] == [1920, 2560, 3200] and [r["size"] for r in records] == [2, 3, 3]
    assert all(r["opponent_global_step"] in (1300, 1920, 2560, 3200) for r in records)
    # a boundary that passed two multiples at once runs one event, of the larger j
    wide = duel_pool.PoolSchedule(4, 100, 1.0, SEED)
    r = wide.event(250)
    assert (r["event"], r["slot"], r["size"], r["opponent_slot"]) == (2, 2, 2, 2) and wide.next_event == 300
    zero = duel_pool.PoolSchedule(4, 100, 0.0, SEED)
    zero.event(250)
    assert zero.opponent_slot in (0, 2)                      # drawn among the occupied slots only


def train_args(*extra):
    from paac_amd import train
    return train.get_arg_parser().parse_args(list(extra))


def test_refusals_name_the_flag():
    from paac_amd import logger_utils, train
    defaults = train_args()
    assert (defaults.duel_pool, defaults.duel_pool_every, defaults.duel_pool_latest_p) == (0, 102400, 0.5)
    assert {"duel_pool", "duel_pool_every", "duel_pool_latest_p"} <= {dest for _, dest, _, _, _ in train.BUILD_FLAGS}
    assert duel_pool.check_train_flags(defaults, 1) == 0
    assert duel_pool.check_train_flags(argparse.Namespace(emulator="duel"), 1) == 0          # an args.json from before the flags
    on = train_args("--emulator", "duel", "--duel_pool", "3", "--duel_pool_every", "640", "--duel_pool_latest_p", "0.25")
    assert duel_pool.check_train_flags(on, 1) == 3
    assert duel_pool.check_train_flags(train_args("--emulator", "duel", "--duel_pool", "16", "--duel_pool_latest_p", "1"), 1) == 16
    assert duel_pool.check_train_flags(train_args("--emulator", "duel", "--duel_pool", "1", "--duel_pool_latest_p", "0"), 1) == 1
    for K in ("-1", "17"):
        with pytest.raises(ValueError, match="--duel_pool "):
            duel_pool.check_train_flags(train_args("--emulator", "duel", "--duel_pool", K), 1)
    for K in (2.5, True, "3"):
        with pytest.raises(ValueError, match="--duel_pool "):
            duel_pool.check_train_flags(argparse.Namespace(emulator="duel", duel_pool=K), 1)
    with pytest.raises(SystemExit):
        train_args("--duel_pool", "2.5")
    for every in ("0", "-640"):
        with pytest.raises(ValueError, match="--duel_pool_every"):
            duel_pool.check_train_flags(train_args("--emulator", "duel", "--duel_pool", "2", "--duel_pool_every", every), 1)
    for p in ("-0.1", "1.5", "nan", "inf"):
        with pytest.raises(ValueError, match="--duel_pool_latest_p"):
            duel_pool.check_train_flags(train_args("--emulator", "duel", "--duel_pool", "2", "--duel_pool_latest_p", p), 1)
    for emulator in ("rally", "catch", "synthetic"):
        with pytest.raises(ValueError, match=r"--duel_pool.*--emulator duel"):
            duel_pool.check_train_flags(train_args("--emulator", emulator, "--duel_pool", "2"), 1)
    with pytest.raises(ValueError, match=r"--duel_pool.*2 data-parallel ranks"):
        duel_pool.check_train_flags(on, 2)
    # K = 0 ignores the other two flags, any emulator and any world size
    off = train_args("--emulator", "rally", "--duel_pool_every", "-5", "--duel_pool_latest_p", "7")
    assert duel_pool.check_train_flags(off, 4) == 0
    # the flags travel through args.json
    folder = tempfile.mkdtemp(prefix="paac_poolargs_")
    logger_utils.save_args(on, folder)
    loaded = logger_utils.load_args(os.path.join(folder, "args.json"))
    assert (loaded["duel_pool"], loaded["duel_pool_every"], loaded["duel_pool_latest_p"]) == (3, 640, 0.25)


def test_the_env_spec_gains_the_pool_only_when_it_is_on():
    from paac_amd import environment_creator
    for flags, want in (((), dict(kind="duel", seed=3)), (("--duel_pool", "0"), dict(kind="duel", seed=3)),
                        (("--duel_pool", "5"), dict(kind="duel", seed=3, pool=5))):
        args = train_args("--emulator", "duel", *flags)
        args.random_seed = 3
        assert environment_creator.EnvironmentCreator(args).device_env_spec == want
    args = argparse.Namespace(emulator="duel", emulator_counts=4, random_seed=3)          # from before the flags
    assert environment_creator.EnvironmentCreator(args).device_env_spec == dict(kind="duel", seed=3)
    # the existing refusal of an odd -ec stays, pool or not
    with pytest.raises(ValueError, match="emulator_counts"):
        environment_creator.EnvironmentCreator(train_args("--emulator", "duel", "-ec", "3", "--duel_pool", "2"))


def test_the_entries_are_declared_and_exported_and_no_kind_was_added():
    from paac_amd import _lib, environment_creator, hip_ops, paac
    header = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    step = re.search(r"\bint paac_duel_ghost_step\(([^;]*)\);", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in step.split(",")]
    assert names == ["seed", "env_offset", "N", "actions", "ghost_probs", "A", "sampler_seed", "step_base_dev", "step_offset",
                     "state_in", "state_out", "state_out2", "stack_in", "stack_out", "stack_out2", "ghost_stack_in",
                     "ghost_stack_out", "ghost_stack_out2", "rec", "ghost_actions_out", "stream"]
    assert "const paac_env_records* rec" in step
    assert len(_lib._SIGNATURES["paac_duel_ghost_step"][1]) == len(names) == 21
    reset = re.search(r"\bint paac_duel_ghost_reset\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in reset.split(",")] == ["seed", "env_offset", "N", "state_out", "stack_out",
                                                                     "ghost_stack_out", "stream"]
    assert len(_lib._SIGNATURES["paac_duel_ghost_reset"][1]) == 7
    for entry in ("paac_duel_ghost_reset", "paac_duel_ghost_step"):
        assert entry in _lib.EXPORTED_SYMBOLS and _lib._SIGNATURES[entry][0] is _lib.c_int
    assert callable(hip_ops.duel_ghost_reset) and callable(hip_ops.duel_ghost_step)
    # a flag on --emulator duel, not a new emulator kind
    assert set(hip_ops.PAIRED_GAMES) == set(paac.PAIRED_KINDS) == set(environment_creator.PAIRED_GAMES) == {"duel"}
    source = open(os.path.join(ROOT, "paac_amd", "csrc", "games.hip")).read()
    assert "void ghost_step_kernel(" in source and "dim3(2 * N, PRE_BANDS)" in source
