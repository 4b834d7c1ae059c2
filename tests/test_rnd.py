"""--explore_kind rnd on the host (spec and twin: paac_amd/rnd.py): the flags, the twin's gradient against finite differences of
its own float64 loss, and its pooling on a stack stated by hand."""
import json
import os

import numpy as np
import pytest

from paac_amd import rnd, train


def test_flags_defaults_refusals_and_args_json(tmp_path):
    parser = train.get_arg_parser()
    assert rnd.check_flags(parser.parse_args([])) == ("simhash", 1e-4)
    assert rnd.check_flags(parser.parse_args(["--explore_kind", "rnd", "--rnd_lr", "0.003", "--explore_bonus", "0.1"])) == ("rnd", 0.003)
    # off (BETA = 0), or simhash: nothing of rnd's to refuse
    assert rnd.check_flags(parser.parse_args(["--explore_kind", "rnd", "--host_environments", "true"]), world=2) == ("rnd", 1e-4)
    on = ["--explore_kind", "rnd", "--explore_bonus", "0.1"]
    for argv, world, message in ((["--rnd_lr", "0"], 1, "finite value > 0"), (["--rnd_lr=-1e-4"], 1, "finite value > 0"),
                                 (["--rnd_lr", "inf"], 1, "finite value > 0"), (["--rnd_lr", "nan"], 1, "finite value > 0"),
                                 (on + ["--host_environments", "true"], 1, "needs the device loop"), (on, 2, "one GPU")):
        with pytest.raises(ValueError) as err:
            rnd.check_flags(parser.parse_args(argv), world)
        assert message in str(err.value), (argv, err.value)
    with pytest.raises(SystemExit):
        parser.parse_args(["--explore_kind", "icm"])
    args = parser.parse_args(on + ["--rnd_lr", "0.002"])
    args.debugging_folder = str(tmp_path)
    train.save_args(args, str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "args.json")))
    assert saved["explore_kind"] == "rnd" and saved["rnd_lr"] == 0.002


@pytest.mark.parametrize("at", [rnd.W1 + 5 * rnd.HIDDEN + 7, rnd.B1 + 8, rnd.W2 + 32 * rnd.OUT + 9, rnd.B2 + 63])
def test_twin_gradient_equals_central_differences_of_its_loss(at):
    """One element of each of the four tensors, 3 rows (hidden units 7, 8 and 32 are active on all three).  The loss is piecewise quadratic in the predictor, so a central
    difference that crosses no relu kink is exact up to rounding: |error| ~ eps(float64) * L / h = 2e-16 * 0.1 / 1e-6."""
    twin = rnd.Twin(3)
    u = rnd.pool(np.random.RandomState(0).randint(0, 256, (3, 84, 84, 4)).astype(np.uint8)).astype(np.float64)
    _, g = rnd.gradient(u, twin.target, twin.predictor)
    h, plus, minus = 1e-6, twin.predictor.copy(), twin.predictor.copy()
    plus[at] += h
    minus[at] -= h
    numeric = (rnd.loss(u, twin.target, plus) - rnd.loss(u, twin.target, minus)) / (2 * h)
    assert g[at] != 0.0 and abs(numeric - g[at]) < 1e-9, (numeric, g[at])


def test_twin_pooling_on_a_stack_stated_by_hand():
    """One pixel of 255 in the newest plane at (y, x) = (17, 40) lies in cell (2, 6); a full cell (13, 13); the older planes are
    never read."""
    x = np.zeros((2, 84, 84, 4), dtype=np.uint8)
    x[0, 17, 40, 3] = 255
    x[0, 78:84, 78:84, 3] = 255
    x[1, :, :, :3] = 200
    u = rnd.pool(x)
    want = np.zeros((2, rnd.D), dtype=np.float32)
    want[0, 14 * 2 + 6] = np.float32(255) / np.float32(9180)
    want[0, 14 * 13 + 13] = 1.0
    assert u.dtype == np.float32 and np.array_equal(u, want)
