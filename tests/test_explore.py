"""--explore_bonus on the host (spec and twin: paac_amd/explore.py): the flags, and the twin on a case stated by hand."""
import numpy as np
import pytest

from paac_amd import evaluation, explore, train


def test_flags_defaults_and_refusals():
    parser = train.get_arg_parser()
    assert explore.check_flags(parser.parse_args([])) == (0.0, 32, 20)
    assert explore.check_flags(parser.parse_args(["--explore_bonus", "0.1", "--explore_bits", "64", "--explore_table_bits", "4"])) == (0.1, 64, 4)
    assert explore.check_flags(parser.parse_args(["--host_environments", "true"]), world=2) == (0.0, 32, 20)      # off: nothing to refuse
    for argv, world, message in ((["--explore_bonus", "-0.5"], 1, "finite value >= 0"), (["--explore_bonus", "inf"], 1, "finite value >= 0"),
                                 (["--explore_bonus", "nan"], 1, "finite value >= 0"), (["--explore_bits", "0"], 1, "[1, 64]"),
                                 (["--explore_bits", "65"], 1, "[1, 64]"), (["--explore_table_bits", "3"], 1, "[4, 26]"),
                                 (["--explore_table_bits", "27"], 1, "[4, 26]"),
                                 (["--explore_bonus", "0.1", "--host_environments", "true"], 1, "needs the device loop"),
                                 (["--explore_bonus", "0.1"], 2, "one GPU")):
        with pytest.raises(ValueError) as err:
            explore.check_flags(parser.parse_args(argv), world)
        assert message in str(err.value), (argv, err.value)


@pytest.mark.parametrize("bits", [1, 17, 64])
def test_twin_on_a_case_stated_by_hand(bits):
    """Row 0 is all 128: P = 0 everywhere and every bit is set.  Row 1 differs from it by +1 at one byte k0, row 2 by -1: P is row
    k0 of S and its negation, so the codes are the Philox words of k0 and their complement."""
    seed, k0 = 3, 12345
    x = np.full((3, explore.K), 128, dtype=np.uint8)
    x[1, k0], x[2, k0] = 129, 127
    words = [int(evaluation.philox_word0(seed, half, np.array([k0]), explore.STREAM)[0]) for half in (0, 1)]
    mask = (1 << bits) - 1
    want = [mask, (words[0] | words[1] << 32) & mask, ~(words[0] | words[1] << 32) & mask]
    twin = explore.Twin(seed, bits, 4)
    assert set(np.unique(twin.S)) == {-1, 1} and twin.S.shape == (explore.K, 64)
    rewards = np.array([1.0, 0.0, -1.0], dtype=np.float32)
    code, bonus = twin.bonus(x, 0.5, rewards)
    assert [int(c) for c in code] == want
    # by hand: the finaliser of 0 is 0, so code 0 lives in slot 0; the three codes differ, and rows that share a slot share n
    assert explore.slots(np.array([0], dtype=np.uint64), 4)[0] == 0
    at = explore.slots(code, 4)
    n = np.array([(at == s).sum() for s in at])
    assert twin.counts.sum() == 3 and np.array_equal(twin.counts[at], n)
    assert np.array_equal(bonus, np.float32(0.5) / np.sqrt(n.astype(np.float32))) and np.array_equal(rewards, np.array([1.0, 0.0, -1.0], dtype=np.float32) + bonus)
    _, again = twin.bonus(x, 0.5)          # the table persists: every n doubles
    assert np.array_equal(again, np.float32(0.5) / np.sqrt((2 * n).astype(np.float32)))
