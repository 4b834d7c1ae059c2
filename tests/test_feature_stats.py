"""--feature_stats on the host: the numpy twin's record on hand-made blocks, and the flags' refusals (spec:
paac_amd/feature_stats.py)."""
import argparse

import numpy as np
import pytest

from paac_amd import feature_stats as fs

H = 64
LAYOUT = fs.Layout((16, 0, 0, H))


def folded(h, conv=None):
    conv = np.ones((h.shape[0], 2, 2, 16), dtype=np.float32) if conv is None else conv
    return fs.fold(fs.Block(LAYOUT), [conv, None, None, h.astype(np.float32)])


def record(block, tau=0.025):
    return fs.summary(LAYOUT, fs.finish(block, tau), tau, gram=block.gram())


def test_rank_one_features_have_srank_and_participation_one():
    h = np.outer(np.arange(1, 41), np.linspace(0.5, 2.0, H))
    r = record(folded(h))
    assert r["fc_srank"] == 1 and r["fc_participation_ratio"] == pytest.approx(1.0, rel=1e-6)
    assert r["fc_top_eigen_share"] == pytest.approx(1.0, rel=1e-6) and r["rows"] == 40 and r["cycles"] == 1


def test_orthogonal_features_have_full_rank():
    r = record(folded(3.0 * np.eye(H)))
    assert r["fc_srank"] == H and r["fc_participation_ratio"] == pytest.approx(H, rel=1e-12)
    assert r["layers"]["fc"] == dict(units=H, dormant_fraction=0.0, dead_fraction=0.0, active_fraction=1.0 / H)


def test_all_zero_layer_is_fully_dormant():
    r = record(folded(np.zeros((5, H)), conv=np.zeros((5, 3, 3, 16), dtype=np.float32)))
    assert r["layers"]["conv1"] == dict(units=16, dormant_fraction=1.0, dead_fraction=1.0, active_fraction=0.0)
    assert r["layers"]["fc"]["dormant_fraction"] == 1.0 and r["fc_participation_ratio"] is None and r["fc_srank"] is None


def test_tau_zero_counts_exactly_the_zero_means():
    h = np.abs(np.random.RandomState(0).randn(33, H))
    h[:, [3, 17, 40]] = 0.0
    h[:, 5] *= 1e-6                                   # tiny, not zero: dormant at the default tau, not at 0
    block = folded(h)
    at_zero, default = record(block, 0.0)["layers"]["fc"], record(block)["layers"]["fc"]
    assert at_zero["dormant_fraction"] == at_zero["dead_fraction"] == 3.0 / H and default["dormant_fraction"] == 4.0 / H


def test_two_folds_accumulate_and_the_gram_stays_symmetric():
    rng = np.random.RandomState(1)
    a, b = (np.maximum(rng.randn(n, H), 0.0).astype(np.float32) for n in (2 * fs.CHUNK_ROWS + 5, 7))
    block = fs.fold(folded(a), [None, None, None, b])
    both = np.concatenate([a, b]).astype(np.float64)
    assert np.array_equal(block.gram(), block.gram().T) and block.get("rows") == a.shape[0] + 7
    np.testing.assert_allclose(block.gram(), both.T @ both, rtol=1e-5)
    np.testing.assert_allclose(block.get("sum")[16:], both.sum(axis=0), rtol=1e-12)


@pytest.mark.parametrize("flags", [dict(feature_stats="maybe"), dict(dormant_tau=2.0), dict(dormant_tau=float("nan")),
                                   dict(feature_rank_every=-1), dict(feature_stats=True, world=2)])
def test_flags_are_refused(flags):
    world = flags.pop("world", 1)
    with pytest.raises(ValueError):
        fs.check_flags(argparse.Namespace(**flags), world)
    assert fs.check_flags(argparse.Namespace()) == (False, 0.025, 64)
