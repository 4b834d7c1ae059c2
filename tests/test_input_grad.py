"""No GPU: the flag refusals of paac_amd.test --attack_eps and paac_amd.saliency, and the numpy statement of the FGSM rule."""
import numpy as np
import pytest

from paac_amd import evaluation


def test_fgsm_perturb_at_the_clamp_edges():
    x = np.array([0, 0, 3, 255, 255, 250, 100, 100], dtype=np.uint8)
    g = np.array([1.0, -1.0, 2.0, -1e-30, 1e30, -5.0, 0.0, np.nan], dtype=np.float32)
    assert evaluation.fgsm_perturb(x, g, 8).tolist() == [0, 8, 0, 255, 247, 255, 100, 100]
    assert evaluation.fgsm_perturb(x, g, 255).tolist() == [0, 255, 0, 255, 0, 255, 100, 100]
    assert evaluation.fgsm_perturb(x, g, 0).tolist() == x.tolist() and evaluation.fgsm_perturb(x, g, 1).dtype == np.uint8


@pytest.mark.parametrize("argv", [["--attack_eps", "256"], ["--attack_eps", "-1"], ["--attack_eps", "8"],
                                  ["--attack_eps", "8", "--device_environments", "true", "--versus", "other"]])
def test_attack_flag_refusals(argv):
    from paac_amd import test as harness
    with pytest.raises(ValueError, match="attack_eps"):
        harness.main(["-f", "no_such_folder"] + argv)          # refused before the folder is read
    assert evaluation.check_attack_eps(0, device_environments=False) == 0 and evaluation.check_attack_eps(255) == 255


@pytest.mark.parametrize("argv,message", [(["-tc", "33", "--steps", "32"], "1056 observations"), (["--target", "policy"], "target"),
                                          (["--steps", "0"], "positive"), (["-np", "-1"], "negative")])
def test_saliency_flag_refusals(argv, message):
    from paac_amd import saliency
    with pytest.raises(ValueError, match=message):
        saliency.main(["-f", "no_such_folder", "-o", "maps.npz"] + argv)
    saliency.check_flags(saliency.get_arg_parser().parse_args(["-f", "x", "-o", "y", "-tc", "32", "--steps", "32"]))
