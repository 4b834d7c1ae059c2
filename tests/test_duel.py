"""CPU: the duel spec (paac_amd/duel.py) against rally's, the pair invariants of its numpy twin, and the wiring of
--emulator duel through the parser, the creator, the tables and the C ABI.  The device side: tests/test_duel_gpu.py."""
import argparse
import os
import re

import numpy as np
import pytest

from paac_amd import duel, rally

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 3


def test_with_the_scripted_top_player_a_board_steps_like_rally():
    """Boards 0..7, 3000 uniform random bottom actions each, the states chained by rally's own result: with the rally script as
    the top player's action, step_board returns rally's reward, terminal and truncated flags on every step, rally's state on
    the non-terminal ones and start_board(k + 1) on the terminal ones."""
    rng = np.random.RandomState(0)
    terminals = moved = 0
    for g in range(8):
        s = rally.start_state(SEED, g, 0)
        for step in range(3000):
            a = int(rng.randint(6))
            a_top = duel.scripted_top_action(SEED, g, s)
            moved += a_top != rally.NOOP
            want_state, want_reward, want_terminal, want_truncated = rally.step_state_truncated(SEED, g, s, a)
            state, reward, terminal, truncated = duel.step_board(SEED, g, s, a, a_top)
            assert (reward, terminal, truncated) == (want_reward, want_terminal, want_truncated), (g, step, s, a)
            if want_terminal:
                assert state == duel.start_board(SEED, g, s[9] + 1), (g, step, s, a)
                terminals += 1
            else:
                assert state == want_state, (g, step, s, a)
            s = want_state
    assert terminals >= 100 and moved >= 1000          # episodes did end, and the script did move its paddle


def test_the_scripted_top_player_draws_an_episode_out_to_the_step_cap():
    """The same equivalence where it matters for truncation: return_action at the bottom reaches the step cap."""
    g, s, truncations = 0, rally.start_state(SEED, 0, 0), 0
    for step in range(2 * rally.MAX_STEPS):
        a = rally.return_action(s)
        want = rally.step_state_truncated(SEED, g, s, a)
        got = duel.step_board(SEED, g, s, a, duel.scripted_top_action(SEED, g, s))
        assert got[1:] == want[1:] and (got[0] == want[0] or want[2])
        truncations += want[3]
        s = want[0]
    assert truncations >= 1


def test_anchors_mirror_and_the_alternating_first_serve():
    assert duel.start_board(SEED, 0, 0)[:6] == (5, 6, -1, 1, 12, 3)
    assert duel.start_board(SEED, 1, 0)[:6] == (3, 6, -1, 1, 8, 0)
    assert duel.start_board(SEED, 0, 1)[:6] == (8, 7, -1, -1, 0, 5)
    assert duel.mirror((1, 2, 3, 4, 5, 6, 7, 8, 9, 10)) == (1, 11, 3, -4, 6, 5, 8, 7, 9, 10)
    rng = np.random.RandomState(1)
    for _ in range(200):
        s = tuple(int(v) for v in rng.randint(-1, 14, 10))
        assert duel.mirror(duel.mirror(s)) == s
    for g in range(4):
        for k in range(6):
            s, r = duel.start_board(SEED, g, k), rally.start_state(SEED, g, k)
            if k % 2 == 0:
                assert s == r
            else:
                assert (s[1], s[3]) == (7, -1) and (s[0], s[2], s[4], s[5]) == (r[0], r[2], r[4], r[5]) and s[6:] == r[6:]


def test_duel_boards_keep_the_pair_invariants():
    """DuelBoards(6, seed 3, env_offset 4) under random actions for 1500 steps: after every step the top record is the bottom
    one's mirror, the rewards are opposite with no -0.0 anywhere, terminals and truncated flags agree within a pair, the top
    row's newest plane is the bottom's flipped with 128 and 64 exchanged, and a terminal step leaves [0, 0, 0, plane]."""
    N, half = 6, 3
    boards = duel.DuelBoards(N, seed=SEED, env_offset=4)
    records, stacks = boards.reset()
    assert records.dtype == np.int32 and records.shape == (N, duel.STATE_WORDS) and stacks.shape == (N, 84, 84, 4)
    assert [tuple(records[b][:6]) for b in range(half)] == [duel.start_board(SEED, 4 + b, 0)[:6] for b in range(half)]
    assert not stacks[..., :3].any()
    exchange = np.zeros(256, dtype=np.uint8)
    exchange[[255, 128, 64]] = [255, 64, 128]
    rng = np.random.RandomState(2)
    terminal_steps, points = 0, 0
    for step in range(1500):
        previous = stacks
        actions = rng.randint(6, size=N)
        records, stacks, rewards, terminals, truncated = boards.step(actions)
        assert rewards.dtype == np.float32 and terminals.dtype == bool and truncated.dtype == bool
        for b in range(half):
            assert tuple(records[b + half][:10]) == duel.mirror(tuple(records[b][:10])), (step, b)
            assert not records[b, 10:].any() and not records[b + half, 10:].any()
            assert np.array_equal(stacks[b + half, ..., 3], exchange[np.flipud(stacks[b, ..., 3])]), (step, b)
            assert np.array_equal(stacks[b, ..., 3], rally.plane(tuple(records[b][:10])))
        assert np.array_equal(rewards[half:], -rewards[:half]) and not np.signbit(rewards[rewards == 0.0]).any()
        assert np.array_equal(terminals[half:], terminals[:half]) and np.array_equal(truncated[half:], truncated[:half])
        assert not (truncated & ~terminals).any()
        for e in range(N):
            if terminals[e]:
                assert not stacks[e, ..., :3].any()
            else:
                assert np.array_equal(stacks[e, ..., :3], previous[e, ..., 1:])
        terminal_steps += int(terminals[:half].sum())
        points += int((rewards[:half] != 0.0).sum())
    assert terminal_steps >= 10 and points >= 5 * terminal_steps
    with pytest.raises(ValueError):
        duel.DuelBoards(5, seed=SEED)
    with pytest.raises(ValueError):
        duel.DuelBoards(0, seed=SEED)


def test_the_step_cap_truncates_both_rows_and_a_fifth_point_does_not():
    boards = duel.DuelBoards(2, seed=SEED)
    boards.reset()
    capped = (5, 8, 1, 1, 9, 3, 2, 1, 999, 4)                    # steps = 999, the ball in the middle: no point pending
    boards.rows = [capped, duel.mirror(capped)]
    records, stacks, rewards, terminals, truncated = boards.step([0, 0])
    assert terminals.tolist() == [True, True] and truncated.tolist() == [True, True] and rewards.tolist() == [0.0, 0.0]
    assert tuple(records[0][:10]) == duel.start_board(SEED, 0, 5) and tuple(records[1][:10]) == duel.mirror(duel.start_board(SEED, 0, 5))
    assert not stacks[..., :3].any()
    won = (5, 1, 1, -1, 9, 4, 4, 3, 999, 2)                     # mine = 4, the ball about to pass the top paddle -- at the cap
    for state in (won, won[:8] + (500,) + won[9:]):
        boards.rows = [state, duel.mirror(state)]
        records, stacks, rewards, terminals, truncated = boards.step([0, 0])
        assert terminals.tolist() == [True, True] and truncated.tolist() == [False, False] and rewards.tolist() == [1.0, -1.0]
    boards.rows = [won, duel.mirror(won)]                        # the top player steps under the ball: the cap alone ends it
    _, _, rewards, terminals, truncated = boards.step([0, rally.RIGHT])
    assert terminals.tolist() == [True, True] and truncated.tolist() == [True, True] and rewards.tolist() == [0.0, 0.0]


def duel_args(*extra):
    from paac_amd import train
    return train.get_arg_parser().parse_args(["--emulator", "duel"] + list(extra))


def test_the_parser_and_the_creator_know_duel():
    from paac_amd import environment_creator, train
    args = duel_args("-ec", "8")
    assert args.emulator == "duel"
    with pytest.raises(SystemExit):
        train.get_arg_parser().parse_args(["--emulator", "duet"])
    creator = train.get_network_and_environment_creator(args)[1]
    assert creator.num_actions == 6 == args.num_actions == duel.NUM_ACTIONS
    assert creator.device_env_spec == dict(kind="duel", seed=3)
    host = creator.create_environment(2)
    assert type(host) is rally.RallyEnvironment and host.actor_id == 2 and host.seed == 3
    assert set(environment_creator.PAIRED_GAMES) == {"duel"}


def test_start_up_refusals_name_their_flag():
    from paac_amd import environment_creator
    with pytest.raises(ValueError, match="emulator_counts"):
        environment_creator.EnvironmentCreator(duel_args("-ec", "7"))
    with pytest.raises(ValueError, match="emulator_counts"):
        environment_creator.EnvironmentCreator(duel_args("-ec", "0"))
    with pytest.raises(ValueError, match="--host_environments"):
        environment_creator.EnvironmentCreator(duel_args("--host_environments", "true"))
    with pytest.raises(ValueError, match="--synthetic_raw_frames"):
        environment_creator.EnvironmentCreator(duel_args("--synthetic_raw_frames", "true"))
    environment_creator.EnvironmentCreator(duel_args("-ec", "2", "--sampler", "numpy"))      # both samplers are allowed
    environment_creator.EnvironmentCreator(duel_args("-ec", "2", "--sampler", "philox"))


def test_a_duel_run_is_evaluated_as_rally():
    from paac_amd import evaluation, paac
    assert evaluation.check_train_flags(duel_args("--eval_every", "1000")) is True
    assert evaluation.check_train_flags(duel_args()) is False
    with pytest.raises(ValueError, match="data-parallel"):
        evaluation.check_train_flags(duel_args("--eval_every", "1000"), 2)
    with pytest.raises(ValueError, match="--host_environments"):
        evaluation.check_train_flags(duel_args("--eval_every", "1000", "--host_environments", "true"))
    assert paac.eval_env_spec(dict(kind="duel", seed=3), seed=4, single_life=False) == dict(kind="rally", seed=4)
    assert paac.eval_env_spec(dict(kind="duel", seed=3)) == dict(kind="rally", seed=3)
    assert evaluation.check_env_spec(paac.eval_env_spec(dict(kind="duel", seed=3))) == "rally"
    with pytest.raises(ValueError):          # the paired game itself has no device evaluation
        evaluation.check_env_spec(dict(kind="duel", seed=3))
    # the other kinds' derived specs are what they were
    assert paac.eval_env_spec(dict(kind="bricks", seed=3, single_life=True), seed=4, single_life=False) == \
        dict(kind="bricks", seed=4, single_life=False)
    assert paac.eval_env_spec(dict(kind="rally", seed=3)) == dict(kind="rally", seed=3) and paac.eval_env_spec(None) is None


def test_the_paired_table_and_the_three_pinned_tables():
    from paac_amd import environment_creator, hip_ops, paac
    kind = paac.PAIRED_KINDS["duel"]
    assert set(paac.PAIRED_KINDS) == set(hip_ops.PAIRED_GAMES) == {"duel"}
    assert kind["words"] == duel.STATE_WORDS == hip_ops.PAIRED_GAMES["duel"]["words"] == hip_ops.DUEL_STATE_WORDS == 12
    assert kind["max_episode_steps"] == rally.MAX_STEPS == 1000 and kind["truncates"] is True
    assert kind["spec_kwargs"] == () and kind["eval_kind"] == "rally"
    assert kind["reset"] is hip_ops.duel_reset and kind["step"] is hip_ops.duel_step
    header = open(os.path.join(ROOT, "paac_amd", "csrc", "duel_dev.h")).read()
    assert re.search(r"kWords = 12;", header) and re.search(r"kPaired = true;", header)
    assert paac.device_kind(dict(kind="duel", seed=3)) is kind
    assert paac.device_kind(dict(kind="rally", seed=3)) is paac.STATEFUL_KINDS["rally"]
    assert paac.device_kind(dict(kind="synthetic")) is None and paac.device_kind(None) is None
    three = {"catch", "bricks", "rally"}
    assert set(hip_ops.DEVICE_GAMES) == set(hip_ops.EVAL_GAMES) == set(paac.STATEFUL_KINDS) == three
    assert set(environment_creator.DEVICE_GAMES) == three
    # duel_step takes game_step's positional list, without the kind
    with pytest.raises(AttributeError):          # None.shape: the arguments were accepted by name and position
        hip_ops.duel_step(*[None] * 11, finished=None, stack_out2=None, state_out2=None, truncs_out=None)


def test_the_c_entries_are_declared_and_exported():
    from paac_amd import _lib
    header = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for entry in ("paac_duel_reset", "paac_duel_step"):
        assert entry in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint %s\(uint64_t seed, uint32_t env_offset, int N," % entry, header)
    step = re.search(r"int paac_duel_step\(([^;]*)\);", header).group(1)
    assert "const paac_env_records* rec" in step and "const int32_t* actions" in step
    assert len(_lib._SIGNATURES["paac_duel_step"][1]) == len(step.split(","))
    assert len(_lib._SIGNATURES["paac_duel_reset"][1]) == 6
    # no evaluation id: the three of paac_eval_step stay
    assert (_lib.EVAL_CATCH, _lib.EVAL_BRICKS, _lib.EVAL_RALLY) == (0, 1, 2) and not hasattr(_lib, "EVAL_DUEL")
