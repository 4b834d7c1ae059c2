"""--sticky_action_p (spec and numpy twin: paac_amd/sticky.py), without a device: the draw, the wrapper of the host twins, the
batch function, the flag and its refusals, and that the constants and entries are spelled the same on both sides.  The GPU side
is tests/test_sticky_gpu.py."""
import argparse
import logging
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from paac_amd import bricks, catch, sticky
from paac_amd.sticky import EVAL_STREAM_STICKY, STICKY_STREAM, StickyEnvironment


def hashed_actions(steps, N, num_actions, salt=0):
    """Actions that depend on nothing but (step, environment): int32 [steps, N]."""
    t, e = np.meshgrid(np.arange(steps, dtype=np.uint64), np.arange(N, dtype=np.uint64), indexing="ij")
    h = (t * np.uint64(2654435761) + e * np.uint64(40503) + np.uint64(salt) * np.uint64(97)) >> np.uint64(7)
    return (h % np.uint64(num_actions)).astype(np.int32)


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def test_p_zero_never_sticks():
    for stream in (STICKY_STREAM, EVAL_STREAM_STICKY):
        for step in (0, 1, 77, 1 << 33):
            assert not sticky.sticks(0.0, 3, step, np.arange(512), stream).any()


@pytest.mark.parametrize("seed,stream,value", [(3, STICKY_STREAM, 0.24968), (4, EVAL_STREAM_STICKY, 0.24902)])
def test_a_quarter_of_the_draws_stick(seed, stream, value):
    """g = 0..4095, steps 0..63, P = 0.25: 262144 draws, a standard deviation of 0.00085 -- the bar of 0.005 is six of them."""
    stuck = sum(int(sticky.sticks(0.25, seed, step, np.arange(4096), stream).sum()) for step in range(64))
    fraction = stuck / (4096.0 * 64)
    print("seed %d stream 0x%08X: %.5f" % (seed, stream, fraction))
    assert abs(fraction - 0.25) < 0.005
    assert round(fraction, 5) == value


def test_the_step_entry_shape_has_87_sticking_draws():
    """N = 3, env_offset 5, 120 steps, seed 3: what tests/test_sticky_gpu.py's first case exercises."""
    assert sum(int(sticky.sticks(0.25, 3, t, 5 + np.arange(3), STICKY_STREAM).sum()) for t in range(120)) == 87


def test_the_draw_is_keyed_by_seed_step_environment_and_stream():
    base = sticky.sticks(0.5, 3, 9, np.arange(256), STICKY_STREAM)
    for other in (sticky.sticks(0.5, 4, 9, np.arange(256), STICKY_STREAM), sticky.sticks(0.5, 3, 10, np.arange(256), STICKY_STREAM),
                  sticky.sticks(0.5, 3, 9, 256 + np.arange(256), STICKY_STREAM),
                  sticky.sticks(0.5, 3, 9, np.arange(256), EVAL_STREAM_STICKY)):
        assert 64 < int((base != other).sum()) < 192
    # the 32 high bits of a step are part of the counter
    assert (sticky.sticks(0.5, 3, 9, np.arange(256), STICKY_STREAM) != sticky.sticks(0.5, 3, 9 + (1 << 32), np.arange(256),
                                                                                      STICKY_STREAM)).any()


def test_the_streams_are_none_in_use():
    from paac_amd import duel_pool, evaluation, match
    used = {0, evaluation.EVAL_STREAM_ACTION, evaluation.EVAL_STREAM_NOOP, match.MATCH_STREAM_TOP, duel_pool.GHOST_STREAM,
            0x44500001, 0x44500003} | {0x504D0000 + epoch for epoch in range(64)}
    assert STICKY_STREAM == 0x53544B01 and EVAL_STREAM_STICKY == 0x45560004
    assert STICKY_STREAM not in used and EVAL_STREAM_STICKY not in used and STICKY_STREAM != EVAL_STREAM_STICKY


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------
def run_twin(env, actions):
    """-> [(observation bytes, reward, terminal, state words)] of a twin stepped the way the runners step it."""
    out = [env.get_initial_state().tobytes()]
    for a in actions:
        obs, r, t = env.next(np.eye(env.num_actions)[int(a)])
        if t:
            obs = env.get_initial_state()
        out.append((obs.tobytes(), float(r), bool(t), env.state_words().tobytes()))
    return out


def test_a_wrapper_with_p_zero_is_transparent():
    actions = hashed_actions(200, 1, 3)[:, 0]
    plain = run_twin(bricks.BricksEnvironment(6, seed=3), actions)
    wrapped = run_twin(StickyEnvironment(bricks.BricksEnvironment(6, seed=3), 0.0, 3, 6), actions)
    assert plain == wrapped


def test_the_wrapper_forwards_the_twins_surface():
    twin = bricks.BricksEnvironment(2, seed=5)
    env = StickyEnvironment(twin, 0.25, 5, 2)
    assert env.num_actions == 3 and list(env.get_legal_actions()) == [0, 1, 2] and env.get_noop() == twin.get_noop()
    assert np.array_equal(env.state_words(), twin.state_words())
    assert env.last_step_truncated is False and env.seed == 5 and env.actor_id == 2
    frames = []
    env.on_new_frame = frames.append
    assert twin.on_new_frame == frames.append
    # a twin without a step cap keeps saying so through the wrapper (--bootstrap_truncated asks with hasattr)
    assert not hasattr(StickyEnvironment(catch.CatchEnvironment(0, seed=1), 0.25, 1, 0), "last_step_truncated")


def test_the_wrapper_executes_the_previous_action_where_the_draw_sticks():
    seed, g, p, steps = 3, 7, 0.25, 300
    actions = hashed_actions(steps, 1, 3, salt=1)[:, 0]
    env = StickyEnvironment(bricks.BricksEnvironment(g, seed=seed), p, seed, g)
    shadow = bricks.BricksEnvironment(g, seed=seed)          # stepped on the executed actions by hand
    env.get_initial_state()
    shadow.get_initial_state()
    prev, stuck_steps, terminals = 0, 0, 0
    for t in range(steps):
        stuck = bool(sticky.sticks(p, seed, t, np.array([g]), STICKY_STREAM)[0])
        executed = prev if stuck else int(actions[t])
        stuck_steps += stuck
        obs, r, term = env.next(np.eye(3)[actions[t]])
        want_obs, want_r, want_term = shadow.next(np.eye(3)[executed])
        assert env.last_executed == executed and np.array_equal(obs, want_obs) and (r, term) == (want_r, want_term)
        prev = 0 if term else executed
        assert env.prev == prev
        if term:
            terminals += 1
            env.get_initial_state()
            shadow.get_initial_state()
    assert stuck_steps > 50 and terminals >= 1


def test_prev_is_cleared_by_a_terminal_step_and_by_get_initial_state():
    env = StickyEnvironment(catch.CatchEnvironment(0, seed=1), 0.0, 1, 0)
    env.get_initial_state()
    env.next(np.eye(3)[2])
    assert env.prev == 2
    env.get_initial_state()
    assert env.prev == 0
    for t in range(catch_episode_steps(env) - 1):
        assert not env.next(np.eye(3)[1])[2] and env.prev == 1
    assert env.next(np.eye(3)[1])[2] and env.prev == 0


def catch_episode_steps(env):
    """Steps until the episode that just started ends (on a copy of the game: catch has no randomness after the start)."""
    twin = catch.CatchEnvironment(env.actor_id, seed=env.seed)
    twin.state = env.state
    steps = 1
    while not twin.next(np.eye(3)[0])[2]:
        steps += 1
    return steps


def test_apply_agrees_with_a_loop_of_wrappers():
    seed, env_offset, N, p, steps = 3, 5, 6, 0.25, 150
    actions = hashed_actions(steps, N, 3, salt=2)
    wrappers = [StickyEnvironment(bricks.BricksEnvironment(env_offset + e, seed=seed), p, seed, env_offset + e) for e in range(N)]
    for env in wrappers:
        env.get_initial_state()
    prev = np.zeros(N, dtype=np.int32)
    differs = 0
    for t in range(steps):
        executed, prev = sticky.apply(actions[t], prev, t, env_offset + np.arange(N), p, seed, STICKY_STREAM)
        assert executed.dtype == np.int32 and prev.dtype == np.int32
        terminals = np.zeros(N, dtype=bool)
        for e, env in enumerate(wrappers):
            terminals[e] = env.next(np.eye(3)[actions[t, e]])[2]
            assert env.last_executed == executed[e], (t, e)
            if terminals[e]:
                env.get_initial_state()
        prev[terminals] = 0
        assert [env.prev for env in wrappers] == prev.tolist()
        differs += int((executed != actions[t]).sum())
    assert differs > 50


# ---- the flag ---------------------------------------------------------------------------------------------------------------------
def parse(*argv):
    from paac_amd import train
    return train.get_arg_parser().parse_args(list(argv))


def test_parser_default_and_help():
    from paac_amd import train
    assert parse().sticky_action_p == 0.0 and parse("--sticky_action_p", "0.25").sticky_action_p == 0.25
    row = [f for f in train.BUILD_FLAGS if f[1] == "sticky_action_p"]
    assert len(row) == 1 and row[0][2] == 0.0 and row[0][3] is float and len(row[0][4]) > 40
    assert sticky.check_flags(parse()) == 0.0 and sticky.check_flags(parse("--emulator", "bricks", "--sticky_action_p", "0.25")) == 0.25


@pytest.mark.parametrize("p", ["-0.1", "1.0", "1.5", "nan", "inf"])
def test_p_outside_the_half_open_interval_is_refused(p):
    with pytest.raises(ValueError, match="sticky_action_p"):
        sticky.check_flags(parse("--emulator", "bricks", "--sticky_action_p", p))
    with pytest.raises(ValueError):
        StickyEnvironment(catch.CatchEnvironment(0), float(p), 0, 0)


def test_pool_match_and_versus_are_refused_beside_it():
    with pytest.raises(ValueError, match="duel_pool"):
        sticky.check_flags(parse("--emulator", "duel", "--sticky_action_p", "0.25", "--duel_pool", "4"))
    with pytest.raises(ValueError, match="eval_match"):
        sticky.check_flags(parse("--emulator", "duel", "--sticky_action_p", "0.25", "--eval_every", "1000", "--eval_match", "8"))
    with pytest.raises(ValueError, match="versus"):
        sticky.check_flags(parse("--emulator", "duel", "--sticky_action_p", "0.25"), versus="other/")
    # ... and accepted beside them when off
    assert sticky.check_flags(parse("--emulator", "duel", "--duel_pool", "4", "--eval_match", "8"), versus="other/") == 0.0


def test_train_main_refuses_before_a_learner_exists(monkeypatch):
    from paac_amd import parallel, train
    monkeypatch.setattr(parallel, "init_from_env", lambda args: 1)
    monkeypatch.setattr(train, "PAACLearner", lambda *a, **k: pytest.fail("a learner was built"))
    with pytest.raises(ValueError, match="sticky_action_p"):
        train.main(parse("--emulator", "bricks", "--sticky_action_p", "1.0"))


def test_test_py_takes_the_flag_and_refuses_versus(tmp_path):
    from paac_amd import logger_utils, test as paac_test
    cli = paac_test.get_arg_parser().parse_args(["-f", str(tmp_path)])
    assert cli.sticky_action_p is None
    logger_utils.save_args(parse("--emulator", "rally", "--sticky_action_p", "0.25"), str(tmp_path))
    assert paac_test.restore_settings(cli).sticky_action_p == 0.25                     # the run's own value
    cli = paac_test.get_arg_parser().parse_args(["-f", str(tmp_path), "--sticky_action_p", "0"])
    assert paac_test.restore_settings(cli).sticky_action_p == 0.0                      # given by hand
    cli = paac_test.get_arg_parser().parse_args(["-f", str(tmp_path), "--device_environments", "true", "--versus", str(tmp_path)])
    with pytest.raises(ValueError, match="versus"):
        paac_test.match_on_device(cli)


def test_args_json_round_trip_and_the_missing_key(tmp_path):
    import json
    from paac_amd import logger_utils
    logger_utils.save_args(parse("--emulator", "bricks", "--sticky_action_p", "0.25"), str(tmp_path))
    loaded = logger_utils.load_args(os.path.join(str(tmp_path), "args.json"))
    assert loaded["sticky_action_p"] == 0.25 and sticky.flag_of(argparse.Namespace(**loaded)) == 0.25
    del loaded["sticky_action_p"]                              # a file from before the flag
    with open(os.path.join(str(tmp_path), "args.json"), "w") as f:
        json.dump(loaded, f)
    old = argparse.Namespace(**logger_utils.load_args(os.path.join(str(tmp_path), "args.json")))
    assert sticky.flag_of(old) == 0.0 and sticky.check_flags(old) == 0.0


def test_synthetic_accepts_the_flag_with_one_log_line(caplog):
    with caplog.at_level(logging.INFO):
        assert sticky.check_flags(parse("--sticky_action_p", "0.25")) == 0.25
    lines = [r for r in caplog.records if "sticky_action_p" in r.getMessage()]
    assert len(lines) == 1 and "without effect" in lines[0].getMessage() and "synthetic" in lines[0].getMessage()
    caplog.clear()
    with caplog.at_level(logging.INFO):
        sticky.check_flags(parse("--emulator", "bricks", "--sticky_action_p", "0.25"))
        sticky.check_flags(parse())
    assert not [r for r in caplog.records if "sticky_action_p" in r.getMessage()]


def test_the_creator_wraps_the_twins_only_when_p_is_above_zero():
    from paac_amd.environment_creator import EnvironmentCreator
    for game, twin in (("catch", catch.CatchEnvironment), ("bricks", bricks.BricksEnvironment)):
        off = EnvironmentCreator(parse("--emulator", game))
        assert type(off.create_environment(2)) is twin and "sticky_p" not in off.device_env_spec
        on = EnvironmentCreator(parse("--emulator", game, "--sticky_action_p", "0.25"))
        env = on.create_environment(2)
        assert isinstance(env, StickyEnvironment) and type(env.env) is twin
        assert (env.sticky_p, env.sticky_seed, env.sticky_g, env.sticky_stream) == (0.25, 3, 2, STICKY_STREAM)
        assert on.device_env_spec["sticky_p"] == 0.25
        on.sticky_stream, on.sticky_seed = EVAL_STREAM_STICKY, 11                     # an evaluation's key
        env = on.create_environment(4)
        assert (env.sticky_seed, env.sticky_g, env.sticky_stream) == (11, 4, EVAL_STREAM_STICKY)
    assert EnvironmentCreator(parse("--emulator", "duel", "--sticky_action_p", "0.25")).device_env_spec["sticky_p"] == 0.25
    assert "sticky_p" not in EnvironmentCreator(parse("--sticky_action_p", "0.25")).device_env_spec       # synthetic: no effect


def test_the_user_games_twin_is_wrapped_too(monkeypatch):
    from paac_amd import environment_creator, user_game

    class Twin(catch.CatchEnvironment):
        pass

    module = type("Module", (), {"NUM_ACTIONS": 3, "Environment": Twin})
    monkeypatch.setattr(user_game, "load", lambda path: module)
    monkeypatch.setattr(user_game, "option_keys", lambda m: ())
    monkeypatch.setattr(user_game, "check_flags", lambda args: None)
    creator = environment_creator.EnvironmentCreator(parse("--emulator", "user", "--device_game", "x.py", "--sticky_action_p", "0.5"))
    env = creator.create_environment(1)
    assert isinstance(env, StickyEnvironment) and type(env.env) is Twin and env.sticky_p == 0.5


@pytest.mark.parametrize("argv,want", [(("--sticky_action_p", "0.25"), 0.25), ((), 0.0)])
def test_ale_gets_p_as_its_repeat_action_probability(argv, want):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fake_ale import FakeALE
    from paac_amd.atari_emulator import AtariEmulator
    args = parse("--emulator", "ale", *argv)
    args.random_seed = 3
    ale = FakeALE()
    AtariEmulator(0, args, ale=ale)
    assert ale.options[b"repeat_action_probability"] == want and isinstance(ale.options[b"repeat_action_probability"], float)


# ---- both sides spell it the same ------------------------------------------------------------------------------------------------
def test_the_stream_constants_are_the_kernels():
    source = open(os.path.join(ROOT, "paac_amd", "csrc", "games.hip")).read()
    assert int(re.search(r"constexpr uint32_t kStickyStream = (0x[0-9A-Fa-f]+)u;", source).group(1), 16) == STICKY_STREAM
    assert int(re.search(r"constexpr uint32_t kEvalStreamSticky = (0x[0-9A-Fa-f]+)u;", source).group(1), 16) == EVAL_STREAM_STICKY


def test_the_entries_are_declared_in_the_header_and_the_binding():
    from paac_amd import _lib, hip_ops
    header = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for entry, wrapper in (("paac_game_step_sticky", "game_step_sticky"), ("paac_duel_step_sticky", "duel_step_sticky"),
                           ("paac_eval_step_sticky", "eval_step_sticky")):
        assert re.search(r"^int %s\(" % entry, header, re.M), entry
        assert entry in _lib.EXPORTED_SYMBOLS and _lib._SIGNATURES[entry][0] is _lib.c_int
        assert callable(getattr(hip_ops, wrapper))
    block = re.search(r"typedef struct \{([^}]*)\} paac_sticky;", header).group(1)
    fields = re.findall(r"(\w+);", block)
    assert fields == [name for name, _ in _lib.Sticky._fields_] == ["p", "step_base_dev", "step_offset", "prev_in", "prev_out",
                                                                    "prev_out2"]
    # the block goes before the stream; the evaluation takes p and the two planes there
    assert _lib._SIGNATURES["paac_game_step_sticky"][1][:-2] == _lib._SIGNATURES["paac_game_step"][1][:-1]
    assert _lib._SIGNATURES["paac_duel_step_sticky"][1][:-2] == _lib._SIGNATURES["paac_duel_step"][1][:-1]
    assert _lib._SIGNATURES["paac_eval_step_sticky"][1][:-4] == _lib._SIGNATURES["paac_eval_step"][1][:-1]


def test_the_rollout_and_the_evaluator_default_to_no_plane():
    from paac_amd.paac import DeviceRollout, PAIRED_KINDS, STATEFUL_KINDS
    assert DeviceRollout.prev is None and DeviceRollout.sticky_p == 0.0
    assert all(callable(kind["step_sticky"]) for kind in list(STATEFUL_KINDS.values()) + list(PAIRED_KINDS.values()))
