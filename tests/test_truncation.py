"""--bootstrap_truncated on the CPU: the games' notion of a truncated step (paac_amd/bricks.py, paac_amd/rally.py), the float64
restatement of both truncation-aware scans (the contract in include/paac_hip.h: paac_returns_truncs) that the GPU tests in
tests/test_truncation_gpu.py compare against bit for bit, and the flag's parsing."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from paac_amd import bricks, catch, rally      # noqa: E402
from test_gae import gae_restated, records      # noqa: E402  (the estimators' own CPU tests: their inputs, their numbers)


# -- the restatement ---------------------------------------------------------------------------------------------------
# float32 inputs promoted to float64, every operation a separate IEEE float64 operation in the contract's order; numpy float64
# arithmetic performs the same operations.  tr = 1: the step bootstraps from V_t, its own acting value.

def nstep_trunc_restated(v_boot, rewards, masks, values, truncs, gamma):
    """-> (y, adv) float32 [T, N].  A step with tr = 0 is paac.py:144-149 as numpy evaluates it: the first product is float32
    (python float x float32 network output), everything after it float64."""
    T = rewards.shape[0]
    r, m, V = rewards.astype(np.float64), masks.astype(np.float64), values.astype(np.float64)
    y, adv = np.zeros(rewards.shape, np.float32), np.zeros(rewards.shape, np.float32)
    R = None
    for t in reversed(range(T)):
        prod = (gamma * v_boot.astype(np.float32)).astype(np.float64) if t == T - 1 else np.float64(gamma) * R
        plain = r[t] + prod * m[t]
        boot = r[t] + np.float64(gamma) * V[t]
        R = np.where(truncs[t] != 0, boot, plain)
        y[t] = R.astype(np.float32)
        adv[t] = (R - V[t]).astype(np.float32)
    return y, adv


def gae_trunc_restated(v_boot, rewards, masks, values, truncs, gamma, lam):
    """-> (y, adv) float32 [T, N].  tr = 1: delta = (r + gamma V_t) - V_t, A = delta (the recursion is cut)."""
    T = rewards.shape[0]
    gamma, gl = np.float64(gamma), np.float64(float(gamma) * float(lam))
    r, m, V = rewards.astype(np.float64), masks.astype(np.float64), values.astype(np.float64)
    y, adv = np.zeros(rewards.shape, np.float32), np.zeros(rewards.shape, np.float32)
    A = np.zeros(rewards.shape[1], np.float64)
    Vn = v_boot.astype(np.float64)
    for t in reversed(range(T)):
        plain = ((r[t] + (gamma * Vn) * m[t]) - V[t]) + (gl * A) * m[t]
        boot = (r[t] + gamma * V[t]) - V[t]
        A = np.where(truncs[t] != 0, boot, plain)
        adv[t] = A.astype(np.float32)
        y[t] = (A + V[t]).astype(np.float32)
        Vn = V[t]
    return y, adv


def returns_restated(v_boot, rewards, masks, values, truncs, gamma, lam=None):
    """The routing rule of --gae_lambda (hip_ops.uses_gae): None and 1.0 are the n-step return."""
    if lam is None or float(lam) == 1.0:
        return nstep_trunc_restated(v_boot, rewards, masks, values, truncs, gamma)
    return gae_trunc_restated(v_boot, rewards, masks, values, truncs, gamma, lam)


def trunc_records(T, N, seed, both_signs=True):
    """Rollout records with a truncation plane as the issue sets it: ones at t = 0, at t = T - 1 and in the middle; environment
    0 has a real terminal and a truncation in the same rollout, environment 1 two truncations; a truncated step has mask 0;
    values of both signs."""
    rs = np.random.RandomState(seed)
    v_boot = (3.0 * rs.randn(N)).astype(np.float32)
    rewards = rs.choice([-1.0, 0.0, 1.0], size=(T, N)).astype(np.float32)
    values = (3.0 * rs.randn(T, N)).astype(np.float32)
    if not both_signs:
        values = np.abs(values)
    masks = np.ones((T, N), np.float32)
    truncs = np.zeros((T, N), np.float32)
    truncs[T // 2, 0] = 1.0
    masks[T - 2, 0] = 0.0                         # environment 0: a real terminal after its truncation
    truncs[0, 1] = truncs[T - 1, 1] = 1.0         # environment 1: two truncations, at both ends
    truncs[T - 1, 2] = 1.0                        # the last step: the v_boot term is not read
    if T > 8:
        truncs[1, 2] = 1.0                        # ... and one in the tail behind the 8-step preload
    masks[truncs != 0] = 0.0
    masks[1, N - 1] = 0.0                         # a plain terminal elsewhere
    assert values.min() < 0 < values.max() or not both_signs
    return v_boot, rewards, masks, values, truncs


# -- 1. the spec, exhaustive at the boundary -----------------------------------------------------------------------------

F = bricks.FULL_ROW


def B(bx, by, dx, dy, px, lives=3, steps=bricks.MAX_STEPS - 1, k=0, rows=(F, F, F)):
    return (bx, by, dx, dy, px, lives, steps, k) + tuple(rows)


# (state one step before the cap, action, single_life) -> (terminal, truncated, what happens)
BRICKS_AT_THE_CAP = [
    (B(5, 12, 1, 1, 9, lives=1), 0, False, True, False, "the last life is lost on the cap step: a real ending"),
    (B(5, 12, 1, 1, 9, lives=3), 0, True, True, False, "a life lost under single_life on the cap step: a real ending"),
    (B(5, 12, 1, 1, 9, lives=3), 0, False, True, True, "a life lost, two left: only the cap ends the episode"),
    (B(5, 12, 1, 1, 9, lives=2), 0, False, True, True, "a life lost, one left: only the cap ends the episode"),
    (B(5, 5, 1, -1, 9), 0, False, True, True, "a brick struck and play goes on: the cap alone"),
    (B(5, 5, 1, -1, 9), 0, True, True, True, "the same under single_life: no life was lost"),
    (B(5, 8, 1, 1, 9), 1, False, True, True, "the ball in flight: the cap alone"),
    (B(5, 12, 1, 1, 5, lives=1), 0, False, True, True, "a paddle hit with one life left: the cap alone"),
]


@pytest.mark.parametrize("state,a,single,terminal,truncated,what", BRICKS_AT_THE_CAP)
def test_bricks_truncated_only_where_the_cap_alone_ends_the_episode(state, a, single, terminal, truncated, what):
    nxt, r, t, tr = bricks.step_state_truncated(3, 2, state, a, single)
    assert (t, tr) == (terminal, truncated), what
    assert (nxt, r, t) == bricks.step_state(3, 2, state, a, single)            # terminal (and everything else) is what it was
    assert nxt == bricks.start_state(3, 2, state[7] + 1)                       # the environment still resets
    # the same state one step earlier in its episode: never truncated, whatever else happens
    early = state[:6] + (bricks.MAX_STEPS - 2,) + state[7:]
    _, _, t2, tr2 = bricks.step_state_truncated(3, 2, early, a, single)
    assert tr2 is False and t2 == (not truncated), what


def test_bricks_away_from_the_cap_is_never_truncated_and_the_twin_exposes_the_flag():
    env = bricks.BricksEnvironment(0, seed=3)
    assert env.last_step_truncated is False
    seen_terminal = 0
    for step in range(2 * bricks.MAX_STEPS + 5):
        state = env.state
        _, _, terminal = env.next(np.eye(3)[bricks.track_action(state)])
        want = bricks.step_state_truncated(3, 0, state, bricks.track_action(state))
        assert (terminal, env.last_step_truncated) == want[2:]
        assert env.last_step_truncated == (state[6] == bricks.MAX_STEPS - 1)   # the tracking policy never loses a life
        seen_terminal += terminal
    assert seen_terminal == 2
    # a random player loses its lives long before the cap: terminal steps, none truncated
    rs = np.random.RandomState(0)
    env, ended = bricks.BricksEnvironment(1, seed=3, single_life=True), 0
    for step in range(400):
        _, _, terminal = env.next(np.eye(3)[rs.randint(3)])
        assert not env.last_step_truncated
        ended += terminal
    assert ended >= 5


def R(bx, by, dx, dy, px, ox, mine=0, theirs=0, steps=rally.MAX_STEPS - 1, k=0):
    return (bx, by, dx, dy, px, ox, mine, theirs, steps, k)


RALLY_AT_THE_CAP = [
    (R(5, 1, 1, -1, 9, 9, mine=4), 0, True, False, "the agent's fifth point on the cap step: a real ending"),
    (R(5, 12, 1, 1, 9, 3, theirs=4), 0, True, False, "the opponent's fifth point on the cap step: a real ending"),
    (R(5, 1, 1, -1, 9, 9, mine=3), 0, True, True, "a fourth point on the cap step: only the cap ends the episode"),
    (R(5, 12, 1, 1, 9, 3, theirs=0), 0, True, True, "a first point for the opponent: only the cap"),
    (R(5, 7, 1, 1, 9, 3, mine=4, theirs=4), 0, True, True, "a rally in flight at 4 : 4: the cap alone"),
    (R(5, 12, 1, 1, 5, 3, theirs=4), 0, True, True, "the agent returns the ball: the cap alone"),
]


@pytest.mark.parametrize("state,a,terminal,truncated,what", RALLY_AT_THE_CAP)
def test_rally_truncated_only_where_the_cap_alone_ends_the_episode(state, a, terminal, truncated, what):
    nxt, r, t, tr = rally.step_state_truncated(3, 1, state, a)
    assert (t, tr) == (terminal, truncated), what
    assert (nxt, r, t) == rally.step_state(3, 1, state, a)
    assert nxt == rally.start_state(3, 1, state[9] + 1)
    early = state[:8] + (rally.MAX_STEPS - 2,) + state[9:]
    _, _, t2, tr2 = rally.step_state_truncated(3, 1, early, a)
    assert tr2 is False and t2 == (not truncated), what


def test_rally_twin_exposes_the_flag_and_catch_never_reports_it():
    env = rally.RallyEnvironment(0, seed=3)
    truncated = terminals = 0
    for step in range(3 * rally.MAX_STEPS):
        state = env.state
        _, _, terminal = env.next(np.eye(6)[rally.return_action(state)])
        assert (terminal, env.last_step_truncated) == rally.step_state_truncated(3, 0, state, rally.return_action(state))[2:]
        if env.last_step_truncated:
            assert terminal and state[8] == rally.MAX_STEPS - 1
        truncated += env.last_step_truncated
        terminals += terminal
    assert truncated >= 1 and terminals >= truncated          # return_action draws most episodes out to the cap
    # catch: 13 steps is the game's rule, not a limit -- the plugin has no such attribute, and the runner reads none
    from paac_amd import runners
    env = catch.CatchEnvironment(0, seed=3)
    assert not hasattr(env, runners.TRUNCATED_ATTRIBUTE)
    for step in range(30):
        _, _, terminal = env.next(np.eye(3)[0])
        assert runners.step_truncated(env, terminal) == 0.0


def test_runner_carries_the_flag_in_one_more_shared_array():
    from paac_amd import runners
    envs = [bricks.BricksEnvironment(e, seed=3) for e in range(3)]
    for env in envs[:2]:
        env.state = env.state[:6] + (bricks.MAX_STEPS - 1,) + env.state[7:]
    envs[1].state = B(5, 12, 1, 1, 9, lives=1)                # ends for a real reason on the cap step
    states = np.stack([e.get_initial_state() for e in envs])
    variables = [states, np.zeros(3, np.float32), np.zeros(3, np.float32), np.eye(3, dtype=np.float32)[[0, 0, 0]],
                 np.full(3, 7.0, np.float32)]
    runners.step_emulators(envs, variables)
    assert list(variables[2]) == [1.0, 1.0, 0.0] and list(variables[4]) == [1.0, 0.0, 0.0]
    # four arrays, as before the flag: nothing else is touched
    runners.step_emulators(envs, variables[:4])
    assert list(variables[4]) == [1.0, 0.0, 0.0]

    class Plugin(object):                                     # the optional attribute only qualifies a terminal step
        last_step_truncated = True
    assert runners.step_truncated(Plugin(), False) == 0.0 and runners.step_truncated(Plugin(), True) == 1.0
    assert runners.step_truncated(object(), True) == 0.0


# -- 2. the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,N,seed", [(5, 8, 9), (8, 64, 1), (20, 128, 5), (9, 32, 2)])
def test_restatement_with_a_zero_plane_is_the_estimators_own_numbers(T, N, seed):
    """The inputs of tests/test_gae.py; the n-step return against oracle.rollout.nstep_returns (what test_gae's n-step tests
    expect), GAE against test_gae's gae_restated -- bit for bit."""
    from oracle import rollout as oroll
    v_boot, r, m, V = records(T, N, seed)
    zero = np.zeros((T, N), np.float32)
    for gamma in (0.99, 1.0):
        ye, ae = oroll.nstep_returns(v_boot, r.astype(np.float64), m.astype(np.float64), V.astype(np.float64), gamma)
        y, adv = nstep_trunc_restated(v_boot, r, m, V, zero, gamma)
        assert np.array_equal(y, ye.astype(np.float32)) and np.array_equal(adv, ae.astype(np.float32))
        for lam in (0.0, 0.5, 0.95):
            ye, ae = gae_restated(v_boot, r, m, V, gamma, lam)
            y, adv = gae_trunc_restated(v_boot, r, m, V, zero, gamma, lam)
            assert np.array_equal(y, ye) and np.array_equal(adv, ae)


def test_restatement_at_a_truncated_step_is_the_bootstrapped_return():
    v_boot, r, m, V, tr = trunc_records(12, 3, 4)
    gamma = 0.99
    y, adv = nstep_trunc_restated(v_boot, r, m, V, tr, gamma)
    on = tr != 0
    want = r.astype(np.float64) + np.float64(gamma) * V.astype(np.float64)
    assert np.array_equal(y[on], want.astype(np.float32)[on])
    assert np.array_equal(adv[on], (want - V.astype(np.float64)).astype(np.float32)[on])
    # with the plane ignored those steps are worth r alone: the estimators differ exactly there and upstream of there
    y0, _ = nstep_trunc_restated(v_boot, r, m, V, np.zeros_like(tr), gamma)
    assert np.array_equal(y0[on], r[on]) and not np.array_equal(y0[on], y[on])
    for lam in (0.0, 0.95):
        yg, ag = gae_trunc_restated(v_boot, r, m, V, tr, gamma, lam)
        assert np.array_equal(ag[on], (want - V.astype(np.float64)).astype(np.float32)[on])
        assert np.array_equal(yg[on], ((want - V.astype(np.float64)) + V.astype(np.float64)).astype(np.float32)[on])
    # a step behind a truncation does not see through it
    y2, _ = nstep_trunc_restated(v_boot + 100.0, r, m, V, tr, gamma)
    assert np.array_equal(y2[:, 1], y[:, 1])                  # environment 1 is truncated at t = T - 1


# -- 3. the flag -------------------------------------------------------------------------------------------------------------

def test_cli_flag_default_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    assert p.parse_args([]).bootstrap_truncated is False
    a = p.parse_args(["--bootstrap_truncated", "true"])
    assert a.bootstrap_truncated is True and p.parse_args(["--bootstrap_truncated", "false"]).bootstrap_truncated is False
    text = [t for o, _, _, _, t in train.BUILD_FLAGS if o == ("--bootstrap_truncated",)][0]
    assert "bricks" in text and "rally" in text and "catch" in text
    logger_utils.save_args(a, str(tmp_path / "with"))
    assert logger_utils.load_args(str(tmp_path / "with" / "args.json"))["bootstrap_truncated"] is True
    b = p.parse_args([])
    del b.bootstrap_truncated                                   # an args.json from before the flag
    logger_utils.save_args(b, str(tmp_path / "without"))
    assert "bootstrap_truncated" not in logger_utils.load_args(str(tmp_path / "without" / "args.json"))
    from paac_amd import test as evaluation
    for folder, want in (("with", True), ("without", None)):
        cli = argparse.Namespace(folder=str(tmp_path / folder), device="/gpu:0", gif_name=None)
        settings = evaluation.restore_settings(cli)
        assert getattr(settings, "bootstrap_truncated", None) is want


def test_learner_reads_the_flag_and_a_namespace_without_it_means_off():
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    args.num_actions = 4
    args.bootstrap_truncated = "yes"
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_header_library_and_binding_agree_on_the_new_entries():
    from paac_amd import _lib, paac
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, nargs in (("paac_returns_scan", 2), ("paac_game_step", 14)):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m and len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs, name
    assert re.search(r"#define PAAC_RETURNS_TRUNCS 0x100\b", hdr) and _lib.RETURNS_TRUNCS == 0x100
    assert [f for f, _ in _lib.ReturnsTruncs._fields_] == ["ret", "truncs"] and _lib.ReturnsTruncs.ret.offset == 0
    records = re.search(r"typedef struct \{([^}]*)\} paac_env_records;", hdr).group(1)
    assert re.findall(r"(\w+)\s*;", records) == [f for f, _ in _lib.EnvRecords._fields_]
    # the games that can be cut off at a step cap
    assert {k: v["truncates"] for k, v in paac.STATEFUL_KINDS.items()} == dict(catch=False, bricks=True, rally=True)
