"""The specification of GPU-resident evaluation (paac_amd/evaluation.py) on the CPU: the Philox restatement against the oracle's,
the action and accounting rules, the replay on the host twins, the flags of test.py / train.py and their refusals."""
import argparse
import json
import os
import tempfile

import numpy as np
import pytest

from oracle import sampler as osampler
from paac_amd import bricks, catch, evaluation
from paac_amd.evaluation import EVAL_STREAM_ACTION, EVAL_STREAM_NOOP

SEEDS = (0x1234ABCD00000007, (5 << 32) + 3)          # non-zero high words
STEPS = (0, 1, 2 ** 32 + 3, 2 ** 40 + 17)
ENVS = np.arange(7) + 11                             # N = 7, global environment indices


def test_stream_constants():
    assert EVAL_STREAM_ACTION != EVAL_STREAM_NOOP and EVAL_STREAM_ACTION != 0 and EVAL_STREAM_NOOP != 0
    for c in (EVAL_STREAM_ACTION, EVAL_STREAM_NOOP):
        assert 0 < c < 2 ** 32 and not 0x504D0000 <= c < 0x504D0040
    # ... and the kernel source holds the same two numbers
    src = open(os.path.join(os.path.dirname(evaluation.__file__), "csrc", "games.hip")).read()
    assert "kEvalStreamAction = 0x%08Xu" % EVAL_STREAM_ACTION in src and "kEvalStreamNoop = 0x%08Xu" % EVAL_STREAM_NOOP in src


@pytest.mark.parametrize("seed", SEEDS)
def test_noops_are_the_oracle_philox_word(seed):
    key = np.tile(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32), (len(ENVS), 1))
    ctr = np.zeros((len(ENVS), 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 3] = ENVS, EVAL_STREAM_NOOP
    word0 = osampler.philox4x32(ctr, key)[:, 0]
    for noops in (1, 3, 30):
        got = evaluation.eval_noops(seed, ENVS, noops)
        assert got.dtype == np.int32 and np.array_equal(got, (word0 % np.uint32(noops + 1)).astype(np.int32))
        assert got.min() >= 0 and got.max() <= noops
    assert np.array_equal(evaluation.eval_noops(seed, ENVS, 0), np.zeros(len(ENVS), dtype=np.int32))
    assert len(set(evaluation.eval_noops(seed, np.arange(64), 30).tolist())) > 8
    with pytest.raises(ValueError):
        evaluation.eval_noops(seed, ENVS, -1)


def inverse_cdf(p, u):
    """oracle.sampler.sample_philox's rule on given uniforms."""
    N, A = p.shape
    acts, chosen, c = np.full(N, A - 1, dtype=np.int32), np.zeros(N, dtype=bool), np.zeros(N, dtype=np.float32)
    for j in range(A - 1):
        c = (c + p[:, j]).astype(np.float32)
        hit = (~chosen) & (u < c)
        acts[hit] = j
        chosen |= hit
    return acts


@pytest.mark.parametrize("A", [3, 18])
@pytest.mark.parametrize("seed", SEEDS)
def test_sampled_action_is_the_oracle_rule_on_the_action_stream(A, seed):
    rs = np.random.RandomState(A)
    p = rs.dirichlet(np.ones(A), size=len(ENVS)).astype(np.float32)
    seen = set()
    for step in STEPS:
        u = osampler.philox_uniform(seed, step, ENVS, stream=EVAL_STREAM_ACTION)
        got = evaluation.eval_action(p, seed, step, ENVS, greedy=False)
        assert got.dtype == np.int32 and np.array_equal(got, inverse_cdf(p, u))
        # the rollout sampler's stream (0) gives other uniforms on the same counter
        assert not np.array_equal(u, osampler.philox_uniform(seed, step, ENVS))
        seen.update(got.tolist())
    assert len(seen) > 1
    # with env ids 0..N-1 and stream 0 the restated rule IS sample_philox
    u0 = osampler.philox_uniform(seed, 5, np.arange(len(ENVS)))
    assert np.array_equal(inverse_cdf(p, u0), osampler.sample_philox(p, seed, 5))


def test_a_running_sum_below_u_falls_through_to_the_last_action():
    p = np.zeros((7, 3), dtype=np.float32)          # sums stay 0 < u whenever u > 0
    seed = SEEDS[0]
    u = osampler.philox_uniform(seed, 9, ENVS, stream=EVAL_STREAM_ACTION)
    assert (u > 0).all()
    assert np.array_equal(evaluation.eval_action(p, seed, 9, ENVS, greedy=False), np.full(7, 2, dtype=np.int32))


def test_greedy_takes_the_lowest_index_on_ties():
    p = np.array([[0.2, 0.4, 0.4], [0.5, 0.5, 0.0], [1 / 3, 1 / 3, 1 / 3], [0.1, 0.2, 0.7], [0.0, 0.0, 1.0]], dtype=np.float32)
    got = evaluation.eval_action(p, 1, 0, np.arange(5), greedy=True)
    assert got.dtype == np.int32 and got.tolist() == [1, 0, 0, 2, 2]
    # ... whatever the seed and the step say
    assert np.array_equal(got, evaluation.eval_action(p, SEEDS[1], 2 ** 32 + 3, np.arange(5) + 9, greedy=True))


def test_accounting_rule_on_hand_written_traces():
    #            t:  0    1    2    3    4    5
    rewards = np.array([[1.0, 1.0, 1.0, 2.0, 5.0, 7.0],          # env 0: no no-ops, terminal at t = 2
                        [1.0, 1.0, 1.0, 2.0, 5.0, 7.0],          # env 1: 2 no-ops, a terminal INSIDE them (t = 1), then one at t = 4
                        [0.0, 0.0, 0.0, 0.0, 0.0, 3.0],          # env 2: never terminal
                        [4.0, 0.0, 0.0, 0.0, 0.0, 0.0]],         # env 3: terminal on its first scored step
                       dtype=np.float32).T
    terminals = np.array([[0, 0, 1, 0, 1, 0],
                          [0, 1, 0, 0, 1, 1],
                          [0, 0, 0, 0, 0, 0],
                          [1, 0, 0, 1, 0, 0]], dtype=bool).T
    noops = np.array([0, 2, 1, 0])
    score, length, done = evaluation.account(rewards, terminals, noops)
    assert score.dtype == np.float32 and length.dtype == np.int32 and done.dtype == np.int32
    assert score.tolist() == [3.0, 8.0, 3.0, 4.0]          # the terminal step's reward counts; nothing after done
    assert length.tolist() == [3, 3, 5, 1]
    assert done.tolist() == [1, 1, 0, 1]
    # max_steps ends the loop: env 1 has not finished by step 4
    score, length, done = evaluation.account(rewards, terminals, noops, max_steps=4)
    assert score.tolist() == [3.0, 3.0, 0.0, 4.0] and length.tolist() == [3, 2, 3, 1] and done.tolist() == [1, 0, 0, 1]
    # one no-op count for all
    assert evaluation.account(rewards, terminals, 6)[1].tolist() == [0, 0, 0, 0]


class Creator(object):
    def __init__(self, cls, seed, num_actions=3):
        self.cls, self.seed, self.num_actions = cls, seed, num_actions

    def create_environment(self, i):
        return self.cls(i, seed=self.seed)


def test_replay_catch_always_stay_reproduces_the_games_own_outcome():
    seed, N, offset = 3, 9, 4
    trace = np.zeros((13, N), dtype=np.int32)
    score, length = evaluation.replay_on_twins(Creator(catch.CatchEnvironment, seed), trace, 0, env_offset=offset)
    for e in range(N):
        state, steps = catch.start_state(seed, offset + e, 0), 0
        while True:
            state, r, over = catch.step_state(state, 0)
            steps += 1
            if over:
                break
        assert (score[e], length[e]) == (r, steps) and r in (-1.0, 1.0) and steps == 13 - catch.start_state(seed, offset + e, 0)[1]
    # no-ops: the first episode that is scored ends at the first terminal at t >= noops_e, wherever it started
    noops = np.array([0, 1, 2, 3, 5, 8, 12, 13, 4])
    trace = np.zeros((13 + 13, N), dtype=np.int32)
    score, length = evaluation.replay_on_twins(Creator(catch.CatchEnvironment, seed), trace, noops, env_offset=offset)
    for e in range(N):
        first = 13 - catch.start_state(seed, offset + e, 0)[1]           # the step count of episode 0
        ends = [first + 13 * k for k in range(3)]                         # terminal steps are t = ends - 1
        end = min(x for x in ends if x - 1 >= noops[e])
        assert length[e] == end - noops[e] and score[e] in (-1.0, 1.0)


def test_replay_bricks_tracking_policy_never_finishes_inside_60_steps():
    seed, N = 3, 3
    states = [bricks.start_state(seed, e, 0) for e in range(N)]
    trace = np.zeros((60, N), dtype=np.int32)
    for t in range(60):
        for e in range(N):
            trace[t, e] = bricks.track_action(states[e])
            states[e] = bricks.step_state(seed, e, states[e], trace[t, e])[0]
    score, length = evaluation.replay_on_twins(Creator(bricks.BricksEnvironment, seed), trace, 0)
    assert length.tolist() == [60] * N and (score >= 1.0).all()
    assert all(s[5] == bricks.LIVES and s[6] == 60 for s in states)
    # always-stay loses its three lives in 24 steps
    score, length = evaluation.replay_on_twins(Creator(bricks.BricksEnvironment, seed), np.zeros((60, N), dtype=np.int32), 0)
    assert length.min() >= 24 and length.max() < 60


def test_longest_episodes_and_bounds():
    from paac_amd.paac import STATEFUL_KINDS
    assert STATEFUL_KINDS["catch"]["max_episode_steps"] == 13 == catch.CELLS - 1
    assert STATEFUL_KINDS["bricks"]["max_episode_steps"] == 500 == bricks.MAX_STEPS
    assert evaluation.max_steps_of("catch", 30) == 43 and evaluation.max_steps_of("bricks", 0) == 500
    for spec in (None, dict(kind="synthetic", seed=3), dict(seed=3)):
        with pytest.raises(ValueError, match=r"--emulator catch\|bricks"):
            evaluation.check_env_spec(spec)
    assert evaluation.check_env_spec(dict(kind="bricks", seed=1, single_life=True)) == "bricks"
    for bad in (0, 4097, -1, 2.5, True):
        with pytest.raises(ValueError):
            evaluation.check_count(bad)
    assert evaluation.check_count(4096) == 4096 and evaluation.check_count(1) == 1


def test_one_table_of_device_games(monkeypatch):
    """A game's record width and evaluation id are stated once (hip_ops.DEVICE_GAMES); every other table and the named wrappers
    follow it, and the device trait and the spec module agree with it."""
    import re
    from paac_amd import _lib, hip_ops, rally
    from paac_amd.paac import STATEFUL_KINDS
    modules = dict(catch=catch, bricks=bricks, rally=rally)
    assert set(hip_ops.DEVICE_GAMES) == set(hip_ops.EVAL_GAMES) == set(STATEFUL_KINDS) == set(modules)
    eval_ids = dict(catch=_lib.EVAL_CATCH, bricks=_lib.EVAL_BRICKS, rally=_lib.EVAL_RALLY)
    csrc = os.path.join(os.path.dirname(evaluation.__file__), "csrc")
    for kind, module in modules.items():
        game = hip_ops.DEVICE_GAMES[kind]
        words = module.STATE_WORDS
        assert game["words"] == words == STATEFUL_KINDS[kind]["words"] == getattr(hip_ops, kind.upper() + "_STATE_WORDS")
        assert hip_ops.EVAL_GAMES[kind] == (eval_ids[kind], words) == (game["eval_id"], words)
        assert re.search(r"kWords = %d;" % words, open(os.path.join(csrc, kind + "_dev.h")).read())
        for entry in ("paac_%s_reset" % kind, "paac_%s_step" % kind):
            assert entry in _lib.EXPORTED_SYMBOLS
        assert STATEFUL_KINDS[kind]["spec_kwargs"] == ((game["step_option"],) if game["step_option"] else ())
    # the named step wrappers reach the game's entry point with its option: bricks_step keeps single_life= (default False), the
    # games without an option refuse one
    calls = []
    monkeypatch.setattr(hip_ops, "_stateful_step", lambda entry, words, *args, extra=(): calls.append((entry, words, extra)))
    hip_ops.bricks_step(*[None] * 11)
    hip_ops.bricks_step(*[None] * 11, single_life=True)
    STATEFUL_KINDS["bricks"]["step"](*[None] * 11, finished=None, stack_out2=None, state_out2=None, single_life=1)
    hip_ops.catch_step(*[None] * 11)
    hip_ops.rally_step(*[None] * 11, finished=None)
    assert calls == [("paac_bricks_step", 12, (False,)), ("paac_bricks_step", 12, (True,)), ("paac_bricks_step", 12, (True,)),
                     ("paac_catch_step", 8, ()), ("paac_rally_step", 12, ())]
    for step in (hip_ops.catch_step, hip_ops.rally_step):
        with pytest.raises(TypeError, match="single_life"):
            step(*[None] * 11, single_life=True)


# -- flags ---------------------------------------------------------------------------------------------------------------------
def test_test_flags_parse_and_refuse():
    from paac_amd import test as harness
    cli = harness.get_arg_parser().parse_args(["-f", "x"])
    assert cli.device_environments is False and cli.greedy is False and cli.eval_seed is None and cli.test_count == 1
    cli = harness.get_arg_parser().parse_args(["-f", "x", "--device_environments", "true", "--greedy", "True", "--eval_seed", "77",
                                               "-tc", "4096"])
    assert cli.device_environments is True and cli.greedy is True and cli.eval_seed == 77
    harness.check_device_flags(cli)
    for extra in (["-gn", "shot"], ["-tc", "4097"], ["-tc", "0"], ["-np", "-1"]):
        bad = harness.get_arg_parser().parse_args(["-f", "x", "--device_environments", "true"] + extra)
        with pytest.raises(ValueError):
            harness.check_device_flags(bad)
        with pytest.raises(ValueError):          # main() refuses before it looks at the folder or the GPU
            harness.main(["-f", "/nonexistent", "--device_environments", "true"] + extra)
    with pytest.raises(ValueError, match="no host screens"):
        harness.check_device_flags(harness.get_arg_parser().parse_args(["-f", "x", "--device_environments", "true", "-gn", "g"]))
    with pytest.raises(SystemExit):
        harness.get_arg_parser().parse_args(["-f", "x", "--greedy", "maybe"])


def test_train_flags_parse_and_refuse():
    from paac_amd import train
    parser = train.get_arg_parser()
    args = parser.parse_args([])
    assert (args.eval_every, args.eval_count, args.eval_greedy) == (0, 64, True)
    assert {"eval_every", "eval_count", "eval_greedy"} <= {dest for _, dest, _, _, _ in train.BUILD_FLAGS}
    assert train.check_eval_flags(args, 1) is False          # off: nothing else is looked at
    assert train.check_eval_flags(parser.parse_args(["--eval_count", "0"]), 4) is False
    on = ["--eval_every", "160", "--emulator", "catch"]
    args = parser.parse_args(on + ["--eval_count", "16", "--eval_greedy", "false"])
    assert (args.eval_every, args.eval_count, args.eval_greedy) == (160, 16, False)
    assert train.check_eval_flags(args, 1) is True
    assert train.check_eval_flags(parser.parse_args(["--eval_every", "1", "--emulator", "bricks", "--eval_count", "4096"]), 1)
    refusals = [(on + ["--host_environments", "true"], 1, "host_environments"),
                (["--eval_every", "160"], 1, r"catch\|bricks"),
                (["--eval_every", "160", "--emulator", "synthetic"], 1, r"catch\|bricks"),
                (["--eval_every", "160", "--emulator", "ale"], 1, r"catch\|bricks"),
                (on, 2, "data-parallel"),
                (["--eval_every", "-5", "--emulator", "catch"], 1, "eval_every"),
                (on + ["--eval_count", "0"], 1, "eval_count"),
                (on + ["--eval_count", "4097"], 1, "eval_count")]
    for argv, world, message in refusals:
        with pytest.raises(ValueError, match=message):
            train.check_eval_flags(parser.parse_args(argv), world)


def test_args_json_round_trip_and_old_runs():
    from paac_amd import logger_utils, train
    from paac_amd import test as harness
    folder = tempfile.mkdtemp(prefix="paac_evalflags_")
    args = train.get_arg_parser().parse_args(["--emulator", "catch", "--eval_every", "160", "--eval_count", "16"])
    logger_utils.save_args(args, folder)
    saved = json.load(open(os.path.join(folder, "args.json")))
    assert (saved["eval_every"], saved["eval_count"], saved["eval_greedy"]) == (160, 16, True)
    # an args.json from before the flags: the evaluation harness restores it, and a Namespace built from it means "off"
    for k in ("eval_every", "eval_count", "eval_greedy"):
        del saved[k]
    json.dump(saved, open(os.path.join(folder, "args.json"), "w"))
    cli = harness.get_arg_parser().parse_args(["-f", folder, "--device_environments", "true", "-tc", "48"])
    settings = harness.restore_settings(cli)
    assert settings.emulator == "catch" and settings.single_life_episodes is False and settings.test_count == 48
    assert settings.device_environments is True and not hasattr(settings, "eval_every")
    assert train.check_eval_flags(argparse.Namespace(**saved), 1) is False
