"""-m gpu: a user's device game (--emulator user --device_game, paac_amd/user_game.py) on the device -- the worked example
examples/patrol, an 18-action game, compiled into a library of its own: paac_user_game_reset / paac_user_game_step,
DeviceRollout with a kind == "user" spec, paac_eval_step with PAAC_EVAL_USER and the command-line tools, against the host twin
examples/patrol/patrol.py.  A process holds one kernel library, so every check runs in a child process
(tests/user_game_checks.py), as tests/test_user_arch_gpu.py does."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

import user_game_checks as checks

pytestmark = pytest.mark.gpu
ROOT = checks.ROOT
SCRIPT = os.path.join(ROOT, "tests", "user_game_checks.py")


def run_check(*argv, timeout=300):
    res = subprocess.run([sys.executable, SCRIPT] + [str(a) for a in argv], cwd=ROOT, capture_output=True, text=True,
                         timeout=timeout)
    print(res.stdout[-3000:])
    print(res.stderr[-3000:], file=sys.stderr)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("CHECK_OK"), (res.stdout[-2000:], res.stderr[-4000:])
    return res.stdout


@pytest.mark.parametrize("N,env_offset,steps", checks.SHAPES)
def test_kernel_matches_twin_bit_for_bit(N, env_offset, steps):
    # (what these runs contain is asserted without a GPU: tests/test_user_game.py)
    seen = checks.random_run(N, env_offset, steps)[1]
    assert seen["entry"] >= 1 and seen["shot_off"] >= 1
    run_check("kernel", N, env_offset, steps)


def test_crafted_records_step_like_the_twin():
    """The cap at steps = 999, cap-and-death, single_life, the same-step re-entry and kill-and-hit, with the truncation plane."""
    run_check("crafted")


def test_refusals_of_the_user_game_library():
    run_check("refusals")


def test_the_stock_library_has_no_user_game():
    run_check("stock_refusals")


@pytest.mark.parametrize("sampler", ["numpy", "philox"])
def test_device_loop_eager_captured_and_batched_agree_and_replay_through_the_twins(sampler):
    """The first learnable-game run of the A = 18 sampler paths."""
    run_check("device_loop", sampler)


def test_host_plugin_loop_matches_device_loop():
    run_check("host_loop")


def test_eval_step_matches_the_replay_on_the_twins():
    run_check("eval_step")


def test_the_test_tool_restores_the_game_and_repeats_itself():
    """python -m paac_amd.test --device_environments true -tc 8 on the folder of a 2-cycle training run: the game comes from
    args.json, and two runs print the same numbers."""
    folder = tempfile.mkdtemp(prefix="paac_patrol_cli_")
    train = subprocess.run([sys.executable, "-m", "paac_amd.train", "--emulator", "user", "--device_game", checks.PATROL, "-df",
                            folder, "-ec", "8", "-ew", "0", "--arch", "NIPS", "--max_global_steps", str(2 * 8 * 5)], cwd=ROOT,
                           capture_output=True, text=True, timeout=300)
    assert train.returncode == 0, (train.stdout[-2000:], train.stderr[-4000:])
    assert '"device_game": "%s"' % checks.PATROL in open(os.path.join(folder, "args.json")).read()
    outputs = []
    for _ in range(2):
        res = subprocess.run([sys.executable, "-m", "paac_amd.test", "-f", folder, "--device_environments", "true", "-tc", "8"],
                             cwd=tempfile.gettempdir(), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
        summary = res.stdout[res.stdout.index("Performed 8 tests"):]
        assert re.search(r"Mean: -?\d+\.\d\d", summary) and "Mean length:" in summary
        outputs.append(summary)
    print(outputs[0])
    assert outputs[0] == outputs[1]


LEARN_STEPS = 2 * 2457600     # twice the step count at which the default flags first cleared the bar (DESIGN.md has the curve)


def test_it_learns():
    """python -m paac_amd.train's main with --emulator user --device_game examples/patrol/patrol.py and the default flags (NIPS
    trunk, RMSProp, lr 0.0224, 32 environments, t_max 5, philox sampler, environment seed 3): the final greedy --eval_every
    evaluation on 64 held-out instances (seed 4, up to 30 no-ops) must reach a mean return of +3.0.  The bar comes from the host
    twin, not from the code under test: over 1024 episodes uniform random play scores -0.47 (std 2.16), always-NOOP -0.84 (std
    1.35) and always-FIRE -0.07 (std 1.38), so a 64-episode mean of a policy without skill has a standard error of at most
    0.28 and +3.0 lies more than ten of them above chance.  Measured on the MI355X, one seed, evaluated every 409,600 steps:
    -0.16, -0.70, -0.70, -0.41, +0.03, then +31.8 at 2,457,600 steps -- the first evaluation above the bar -- and +53.0 at
    2,867,200; the test trains twice 2,457,600 steps, where the evaluation gave +53.7."""
    out = run_check("learns", LEARN_STEPS, 3.0, timeout=600)
    assert "evaluation at %d steps" % LEARN_STEPS in out
