"""--emulator user --device_game (paac_amd/user_game.py) and its worked example examples/patrol, without a GPU: the twin
against its specification, the plugin surface's refusals, the build.  A process holds one kernel library, so whatever makes the
example's library the process's own runs in a child process."""
import argparse
import ctypes
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import user_game_checks as checks

ROOT = checks.ROOT
PATROL = checks.PATROL
SEED = checks.SEED


@pytest.fixture(scope="module")
def p():
    return checks.patrol()


def test_start_state_anchors(p):
    anchors = {(0, 0): (0, 11, -5, -30, -1, -27, -1, 1, -1, 1), (1, 0): (13, 10, -7, -14, -5, -12, 1, 1, -1, -1),
               (2, 0): (9, 0, -11, -7, -12, -12, -1, -1, 1, 1), (0, 1): (4, 4, -1, -31, -15, -1, 1, -1, -1, -1)}
    for (g, k), want in anchors.items():
        s = p.start_state(SEED, g, k)
        assert s[:2] + s[8:16] == want, (g, k)
        assert s[2:8] == (1, p.LIVES, 0, 0, 0, 0) and s[16] == k and len(s) == 17
        assert p.state_words(s).tolist() == list(s) + [0, 0, 0] and p.STATE_WORDS == 20


def test_the_eighteen_actions_differ_in_effect(p):
    assert len(p.ACTIONS) == p.NUM_ACTIONS == 18 and len(set(p.ACTIONS)) == 18
    assert p.ACTIONS[2] == (0, -1, 0) and p.ACTIONS[11] == (1, 0, 1) and p.ACTIONS[17] == (-1, 1, 1)          # UP, RIGHTFIRE, DOWNLEFTFIRE
    s = checks.S(5, 5, face=-1)
    after = {p.step_state(SEED, 0, s, a)[0] for a in range(18)}
    assert len(after) == 18
    assert p.step_state(SEED, 0, s, 18) == p.step_state(SEED, 0, s, 0) == p.step_state(SEED, 0, s, -1)


def test_twin_on_crafted_states(p):
    cases = checks.crafted()
    assert sorted(name for name, _, _, _ in cases) == sorted(checks.EXPECT)
    for e, (name, s, a, single_life) in enumerate(cases):
        state, r, term, trunc, events = p.step_events(SEED, e, s, a, single_life)
        want_r, want_term, want_trunc, want_events = checks.EXPECT[name]
        assert (r, term, trunc) == (want_r, want_term, want_trunc), name
        assert want_events <= events, (name, events)
        assert state == p.start_state(SEED, e, s[16] + 1) if term else state[7] == s[7] + 1, name
    by_name = {name: (e, s, a, sl) for e, (name, s, a, sl) in enumerate(cases)}

    def after(name):
        e, s, a, sl = by_name[name]
        return p.step_state(SEED, e, s, a, sl)[0]

    assert after("kill_flight")[6] == 0 and after("kill_flight")[9] < 0            # the shot is spent, the drone waits
    assert after("hit_walk")[:4] == (4, 5, 1, 2) and after("hit_move")[3] == 2
    assert after("escape")[8] < 0 and after("escape")[10] < 0                      # off either edge
    assert after("entry")[8] == 0 and after("entry")[9] == 13                      # at column 0 flying right, at 13 flying left
    assert after("reentry")[9] in (0, 13)                                          # shot down and back on the board in one step
    assert after("shot_off")[4:7] == (14, 0, 0)
    assert after("fire_ignored")[4:7] == (4, 0, 1)                                 # the old shot flew on; no new one at the craft
    assert after("kill_and_hit")[3] == 2 and after("kill_and_hit")[6] == 0
    assert after("hit_with_lives")[3] == 2
    assert after("diagonal_fire")[:7] == (6, 4, 1, 3, 8, 4, 1)                     # UPRIGHTFIRE: moved, turned, fired, flew 2


def test_twin_observations_are_the_planes(p):
    env = p.Environment(5, seed=SEED, single_life=True)
    obs = env.get_initial_state()
    assert obs.shape == (84, 84, 4) and not obs[..., :3].any() and np.array_equal(obs[..., 3], p.plane(env.state))
    rs = np.random.RandomState(2)
    planes, terminals = [obs[..., 3]], 0
    for _ in range(400):
        obs, r, term = env.next(np.eye(18)[rs.randint(18)])
        assert np.array_equal(obs[..., 3], p.plane(env.state)) and r in (-1.0, 0.0, 1.0)
        if term:
            terminals += 1
            assert not env.last_step_truncated
            obs = env.get_initial_state()
            planes = []
        planes.append(obs[..., 3])
        for c, want in enumerate(planes[-4:][::-1]):
            assert np.array_equal(obs[..., 3 - c], want)
    assert terminals >= 1 and env.state_words().shape == (20,) and env.k == terminals
    # what one plane shows: the shot over the craft over a drone, and the facing
    s = checks.S(3, 5, face=-1, shot=(3, 5, -1), x=(-1, 3, 7, -9))
    plane = p.plane(s)
    assert (plane[30:36, 18:24] == 255).all() and (plane[48:54, 42:48] == 64).all() and set(np.unique(plane)) == {0, 64, 255}
    plane = p.plane(checks.S(3, 5, face=-1, x=(-1, 3, 7, -9)))
    assert (plane[30:36, 18:20] == 224).all() and (plane[30:36, 20:24] == 128).all()
    plane = p.plane(checks.S(3, 5, face=1))
    assert (plane[30:36, 18:22] == 128).all() and (plane[30:36, 22:24] == 224).all() and int((plane > 0).sum()) == 36


def test_reference_policies_are_ordered(p):
    def mean_return(policy):
        total = 0.0
        for g in range(8):
            s = p.start_state(SEED, g, 0)
            for _ in range(2):
                term = False
                while not term:
                    s, r, term = p.step_state(SEED, g, s, policy(s))
                    total += r
        return total / 16

    rng = random.Random(0)
    chance, camper, hunter = mean_return(lambda s: rng.randrange(18)), mean_return(p.camper_action), mean_return(p.hunter_action)
    print("random %+.2f, camper %+.2f, hunter %+.2f" % (chance, camper, hunter))
    assert chance < 3.0 < 30.0 < camper < camper + 10.0 < hunter


def test_random_runs_reach_the_common_event_kinds():
    """From the twins' side, no GPU: the kernel-against-twin runs of tests/test_user_game_gpu.py contain a kill, a hit, an
    escape, an entry, a shot leaving the board and a lost-life terminal."""
    total = dict.fromkeys(checks.TRACE_KINDS, 0)
    for shape in checks.SHAPES:
        for kind, count in checks.random_run(*shape)[1].items():
            total[kind] += count
    print(total)
    assert all(total[kind] >= 1 for kind in checks.TRACE_KINDS), total


# -- the plugin surface ---------------------------------------------------------------------------------------------------

GOOD = """
from paac_amd.environment import BaseEnvironment
NUM_ACTIONS = 4
STATE_WORDS = 8
MAX_EPISODE_STEPS = 100
TRUNCATES = False
STEP_OPTION = None
DEVICE_HEADER = "game_dev.h"
DEVICE_TRAIT = "Game"
class Environment(BaseEnvironment):
    def state_words(self):
        return None
"""


def write_module(folder, name, text):
    path = os.path.join(str(folder), name)
    with open(path, "w") as f:
        f.write(text)
    return path


@pytest.mark.parametrize("change,message", [
    (("NUM_ACTIONS = 4", ""), "NUM_ACTIONS is missing"),
    (("NUM_ACTIONS = 4", "NUM_ACTIONS = 4.0"), "NUM_ACTIONS = 4.0 is float, expected int"),
    (("NUM_ACTIONS = 4", "NUM_ACTIONS = 40"), "NUM_ACTIONS = 40 is outside [2, 32]"),
    (("STATE_WORDS = 8", "STATE_WORDS = 10"), "STATE_WORDS = 10 is no positive multiple of 4"),
    (("MAX_EPISODE_STEPS = 100", "MAX_EPISODE_STEPS = True"), "MAX_EPISODE_STEPS = True is bool, expected int"),
    (("TRUNCATES = False", "TRUNCATES = 0"), "TRUNCATES = 0 is int, expected bool"),
    (("STEP_OPTION = None", ""), "STEP_OPTION is missing"),
    (("STEP_OPTION = None", "STEP_OPTION = 'lives'"), "STEP_OPTION = 'lives'"),
    (("DEVICE_HEADER = \"game_dev.h\"", ""), "DEVICE_HEADER is missing"),
    (("DEVICE_TRAIT = \"Game\"", "DEVICE_TRAIT = 3"), "DEVICE_TRAIT = 3 is int, expected str"),
    (("class Environment(BaseEnvironment):", "class Environment(object):"), "is no BaseEnvironment"),
    (("    def state_words(self):", "    def other(self):"), "has no state_words()"),
])
def test_a_module_that_misses_or_mistypes_an_attribute_is_refused(tmp_path, change, message):
    from paac_amd import user_game
    assert user_game.import_module(write_module(tmp_path, "good.py", GOOD)).NUM_ACTIONS == 4
    with pytest.raises(ValueError) as exc:
        user_game.import_module(write_module(tmp_path, "bad.py", GOOD.replace(*change)))
    assert message in str(exc.value) and "bad.py" in str(exc.value)


def test_bad_tag_and_missing_file_are_refused(tmp_path):
    from paac_amd import build, user_game
    with pytest.raises(ValueError) as exc:
        user_game.import_module(write_module(tmp_path, "my-game.py", GOOD))
    assert "[A-Za-z0-9_]+" in str(exc.value) and "my-game" in str(exc.value)
    for tag in ("", "a.b", "a/b", "a b"):
        with pytest.raises(ValueError):
            build.user_game_library(tag)
    assert build.user_game_library("Game_2")[0].endswith(os.path.join("paac_amd", "libpaac_hip_game_Game_2.so"))
    with pytest.raises(FileNotFoundError) as exc:
        user_game.import_module(os.path.join(str(tmp_path), "gone.py"))
    assert "gone.py" in str(exc.value) and "args.json" in str(exc.value)


def test_flag_combinations_are_refused():
    from paac_amd import environment_creator, train
    for argv, message in [
        (["--emulator", "rally", "--device_game", PATROL], "needs --emulator user"),
        (["--device_game", PATROL], "needs --emulator user"),
        (["--emulator", "user"], "--emulator user needs --device_game"),
        (["--emulator", "user", "--device_game", PATROL, "--user_arch", "16,32,32,256"], "cannot be combined with --user_arch"),
        (["--emulator", "user", "--device_game", PATROL, "--synthetic_raw_frames", "true"], "--synthetic_raw_frames"),
    ]:
        args = train.get_arg_parser().parse_args(argv)
        with pytest.raises(ValueError) as exc:
            environment_creator.EnvironmentCreator(args)
        assert message in str(exc.value), argv
    # old Namespaces without the field: no user game
    assert environment_creator.EnvironmentCreator(argparse.Namespace(emulator="rally")).num_actions == 6


def test_args_json_records_the_absolute_path(tmp_path, monkeypatch):
    from paac_amd import logger_utils, train
    monkeypatch.chdir(os.path.join(ROOT, "examples"))
    args = train.get_arg_parser().parse_args(["--emulator", "user", "--device_game", os.path.join("patrol", "patrol.py")])
    assert args.device_game == PATROL and os.path.isabs(args.device_game)
    assert train.get_arg_parser().parse_args([]).device_game == ""
    train.save_args(args, str(tmp_path))
    restored = logger_utils.load_args(os.path.join(str(tmp_path), "args.json"))
    assert restored["device_game"] == PATROL and restored["emulator"] == "user"


# -- the build ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def patrol_library(p):
    from paac_amd import build
    return build.build_user_game(os.path.join(os.path.dirname(PATROL), p.DEVICE_HEADER), p.DEVICE_TRAIT, "patrol")


def info(path):
    lib = ctypes.CDLL(path)
    numbers = [ctypes.c_int(-1) for _ in range(3)]
    rc = lib.paac_user_game_info(*[ctypes.byref(n) for n in numbers])
    return rc, tuple(n.value for n in numbers), lib


def test_build_user_game_compiles_the_example_and_both_libraries_export_the_entries(patrol_library, p):
    from paac_amd import build
    assert patrol_library == os.path.join(ROOT, "paac_amd", "libpaac_hip_game_patrol.so") and os.path.exists(patrol_library)
    assert os.path.exists(os.path.join(build.CSRC, "games_game_patrol.o"))
    rc, numbers, lib = info(patrol_library)
    assert rc == 1 and numbers == (p.STATE_WORDS, p.NUM_ACTIONS, p.MAX_EPISODE_STEPS) == (20, 18, 1000)
    rc, numbers, stock = info(build.build(verbose=False))
    assert rc == 0 and numbers == (0, 0, 0)
    for name in ("paac_user_game_info", "paac_user_game_reset", "paac_user_game_step", "paac_game_step", "paac_eval_step"):
        assert hasattr(lib, name) and hasattr(stock, name), name
    # without a device: the stock library's entries refuse by name, the example's refuse bad arguments
    stock.paac_last_error.restype = lib.paac_last_error.restype = ctypes.c_char_p
    assert stock.paac_user_game_reset(ctypes.c_uint64(1), 0, 1, None, None, None) < 0
    assert b"built without a user game" in stock.paac_last_error() and b"--device_game" in stock.paac_last_error()
    assert lib.paac_user_game_reset(ctypes.c_uint64(1), 0, 1, None, None, None) < 0
    assert b"paac_user_game_reset: bad arguments" in lib.paac_last_error()


def test_the_header_is_a_dependency_and_the_tag_is_one_headers(patrol_library, tmp_path):
    from paac_amd import build
    header = os.path.join(os.path.dirname(PATROL), "patrol_dev.h")
    assert open(patrol_library + ".header").read().split("\n")[:2] == [header, "PatrolGame"]
    # the same tag from another path: refused, nothing built
    copy = shutil.copy(header, os.path.join(str(tmp_path), "patrol_dev.h"))
    before = os.path.getmtime(patrol_library)
    with pytest.raises(ValueError) as exc:
        build.build_user_game(copy, "PatrolGame", "patrol")
    assert "is taken" in str(exc.value) and header in str(exc.value) and os.path.getmtime(patrol_library) == before
    # staleness: the object is stale against a newer header, current against an older one
    obj = os.path.join(build.CSRC, "games_game_patrol.o")
    assert not build._stale(obj, [header])
    os.utime(copy, (os.path.getmtime(obj) + 10, os.path.getmtime(obj) + 10))
    assert build._stale(obj, [copy])


def test_a_trait_that_declares_kpaired_does_not_compile(tmp_path):
    from paac_amd import build
    text = open(os.path.join(os.path.dirname(PATROL), "patrol_dev.h")).read()
    marker = "  static constexpr int kActions = PATROL_ACTIONS;\n"
    assert marker in text
    header = write_module(tmp_path, "paired_dev.h", text.replace(marker, marker + "  static constexpr bool kPaired = false;\n"))
    lib, suffix = build.user_game_library("kpaired_refusal")
    try:
        with pytest.raises(RuntimeError) as exc:
            build.build_user_game(header, "PatrolGame", "kpaired_refusal")
        assert "a user game must not declare kPaired" in str(exc.value)
        assert not os.path.exists(lib) and not os.path.exists(lib + ".header")
    finally:
        for leftover in (lib + ".lock", os.path.join(build.CSRC, "games%s.o" % suffix)):
            if os.path.exists(leftover):
                os.remove(leftover)


# -- registration, in a process of its own ---------------------------------------------------------------------------------

_REGISTRATION = r"""
import sys
sys.path.insert(0, %(root)r)
from paac_amd import _lib, environment_creator, evaluation, hip_ops, paac, train, user_game
args = train.get_arg_parser().parse_args(["--emulator", "user", "--device_game", %(patrol)r, "--single_life_episodes", "true",
                                          "--eval_every", "1000"])
creator = environment_creator.EnvironmentCreator(args)
assert creator.num_actions == 18 and creator.device_env_spec == dict(kind="user", seed=3, single_life=True)
twin = creator.create_environment(2)
assert type(twin).__name__ == "PatrolEnvironment" and twin.single_life and twin.actor_id == 2
# tables of its own: the pinned ones are what they were
assert set(hip_ops.DEVICE_GAMES) == set(hip_ops.EVAL_GAMES) == set(paac.STATEFUL_KINDS) == {"catch", "bricks", "rally"}
assert set(environment_creator.DEVICE_GAMES) == {"catch", "bricks", "rally"}
assert set(hip_ops.PAIRED_GAMES) == set(paac.PAIRED_KINDS) == {"duel"}
assert hip_ops.USER_GAMES == {"user": dict(words=20, eval_id=_lib.EVAL_USER, step_option="single_life")} and _lib.EVAL_USER == 3
kind = paac.USER_KINDS["user"]
assert (kind["words"], kind["spec_kwargs"], kind["max_episode_steps"], kind["truncates"]) == (20, ("single_life",), 1000, True)
assert kind["reset"] is hip_ops.user_game_reset and kind["step"] is hip_ops.user_game_step
assert paac.device_kind(creator.device_env_spec) is kind and paac.device_kind(dict(kind="rally"))["words"] == 12
assert _lib.LIB_PATH.endswith("libpaac_hip_game_patrol.so") and _lib.user_game() == (20, 18, 1000)
# everything that looks a kind up consults the user table after the built-in ones
assert evaluation.max_steps_of("user", 30) == 1030 and evaluation.max_steps_of("catch", 0) == 13
assert evaluation.check_env_spec(creator.device_env_spec) == "user"
assert evaluation.check_train_flags(args) is True
assert paac.eval_env_spec(creator.device_env_spec, seed=4, single_life=False) == dict(kind="user", seed=4, single_life=False)
try:
    evaluation.check_env_spec(dict(kind="synthetic"))
    raise SystemExit("synthetic accepted")
except ValueError as exc:
    assert "--emulator catch|bricks|rally" in str(exc)
# loading is idempotent; a second game in the process is refused
assert user_game.load(%(patrol)r) is user_game.load(%(patrol)r)
# a module whose numbers are not the trait's: refused, naming both sides
import os, shutil, tempfile
folder = tempfile.mkdtemp()
for name in ("patrol.py", "patrol_dev.h"):
    shutil.copy(os.path.join(os.path.dirname(%(patrol)r), name), folder)
try:
    user_game.load(os.path.join(folder, "patrol.py"))
    raise SystemExit("a second game accepted")
except ValueError as exc:
    assert "already holds" in str(exc)
print("REGISTRATION_OK")
"""

_MISMATCH = r"""
import os, shutil, sys, tempfile
sys.path.insert(0, %(root)r)
from paac_amd import user_game
folder = tempfile.mkdtemp()
text = open(%(patrol)r).read().replace("NUM_ACTIONS = 18", "NUM_ACTIONS = 17").replace(
    'DEVICE_HEADER = "patrol_dev.h"', "DEVICE_HEADER = %%r" %% os.path.join(os.path.relpath(os.path.dirname(%(patrol)r), folder), "patrol_dev.h"))
path = os.path.join(folder, "patrol.py")
open(path, "w").write(text)
try:
    user_game.load(path)
    raise SystemExit("a mismatch accepted")
except ValueError as exc:
    assert "(20, 17, 1000)" in str(exc) and "(20, 18, 1000)" in str(exc) and "PatrolGame" in str(exc), exc
print("MISMATCH_OK")
"""


@pytest.mark.parametrize("script,token", [(_REGISTRATION, "REGISTRATION_OK"), (_MISMATCH, "MISMATCH_OK")])
def test_registration_in_a_child_process(patrol_library, script, token):
    res = subprocess.run([sys.executable, "-c", script % dict(root=ROOT, patrol=PATROL)], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and token in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
