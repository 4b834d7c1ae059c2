"""--window_stats on the CPU: the specification module paac_amd/window_stats.py (the block, the fold's twin, the summary) and
the flag.  Nothing here needs a GPU or the library."""
import argparse
import json
import os

import numpy as np
import pytest

from paac_amd import window_stats as ws

RING_WORDS = 2 + 2 * ws.RING


def make_cycle(rs, T, N, A, steps=1, truncs=False, stats_cols=0, stats_first=0, applied=None, ring=None, loss0=False):
    B = T * N
    values = (rs.randn(T, N) * 10.0 ** rs.uniform(-3, 2, (T, N))).astype(np.float32)
    y = (rs.randn(B) * 10.0 ** rs.uniform(-3, 2, B)).astype(np.float32)
    cycle = dict(T=T, N=N, A=A, values=values, y=y, adv=(y - values.reshape(-1)).astype(np.float32),
                 rewards=rs.choice([-1.0, 0.0, 0.0, 0.5, 1.0], (T, N)).astype(np.float32),
                 masks=(rs.rand(T, N) > 0.2).astype(np.float32), actions=rs.randint(0, A, (T, N)).astype(np.int32),
                 truncs=(rs.rand(T, N) > 0.9).astype(np.float32) if truncs else None,
                 loss=rs.randn(steps, 4).astype(np.float32), loss0=rs.randn(4).astype(np.float32) if loss0 else None,
                 ppo_stats=rs.rand(steps, stats_cols).astype(np.float32) if stats_cols else None, stats_first=stats_first,
                 applied=applied, gnorm=np.abs(rs.randn(1)).astype(np.float32), ring=ring)
    return cycle


def make_ring(count, returns, lengths, first_entry):
    """A ring whose entries first_entry, first_entry + 1, ... hold the given episodes, with `count` entries written in all."""
    ring = np.zeros(RING_WORDS, dtype=np.int32)
    ring[0] = count
    slots = (first_entry + np.arange(len(returns))) & (ws.RING - 1)
    ring[2:2 + ws.RING].view(np.float32)[slots] = np.asarray(returns, dtype=np.float32)
    ring[2 + ws.RING:][slots] = np.asarray(lengths, dtype=np.int32)
    return ring


def close(a, b, rel=1e-12):
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-300)


def test_summary_matches_the_straightforward_formulas():
    rs = np.random.RandomState(3)
    T, N, A = 20, 97, 18                                   # 1940 rows per cycle, five cycles: under 10^4 terms
    acc, cycles = ws.Block(), []
    for c in range(5):
        cycles.append(make_cycle(rs, T, N, A, steps=6, truncs=True, stats_cols=3, stats_first=0,
                                 applied=np.array([1, 1, 1, 0, 0, 0], dtype=np.int32)))
        ws.fold(acc, cycles[-1])
    out = ws.summary(acc, num_actions=A, truncation=True, ppo=True, vclip=True)
    cat = lambda k: np.concatenate([np.asarray(c[k]).reshape(-1) for c in cycles]).astype(np.float64)
    v, y, adv, r, m, tr = (cat(k) for k in ("values", "y", "adv", "rewards", "masks", "truncs"))
    assert out["cycles"] == 5 and out["rows"] == 5 * T * N
    for name, want in (("value_mean", v.mean()), ("value_std", v.std()), ("return_mean", y.mean()), ("return_std", y.std()),
                       ("adv_mean", adv.mean()), ("adv_std", adv.std()), ("adv_abs_max", np.abs(adv).max()),
                       ("reward_mean", r.mean()), ("reward_nonzero_fraction", (r != 0).mean()),
                       ("terminal_fraction", (m == 0).mean()), ("truncated_fraction", (tr != 0).mean()),
                       ("explained_variance", 1.0 - np.var(y - v) / np.var(y)),
                       ("grad_norm_mean", np.mean([float(c["gnorm"][0]) for c in cycles])),
                       ("grad_norm_max", np.max([float(c["gnorm"][0]) for c in cycles]))):
        assert close(out[name], want), (name, out[name], want)
    hist = np.bincount(cat("actions").astype(np.int64), minlength=A) / float(5 * T * N)
    assert len(out["action_freq"]) == A and all(close(a, b) for a, b in zip(out["action_freq"], hist))
    loss = np.concatenate([c["loss"] for c in cycles]).astype(np.float64)
    for k, name in enumerate(ws.LOSS_NAMES):
        assert close(out[name], loss[:, k].mean()), name
    stats = np.concatenate([c["ppo_stats"] for c in cycles]).astype(np.float64)
    for k, name in enumerate(ws.STAT_NAMES):
        assert close(out[name], stats[:, k].mean()), name
    assert out["opt_steps"] == 30 and out["opt_steps_applied"] == 15
    assert out["episodes"] == 0 and out["episode_return_mean"] is None


def test_full_batch_ppo_reports_row_zero_through_loss0_and_skips_its_stats_row():
    rs = np.random.RandomState(5)
    cycle = make_cycle(rs, 5, 4, 4, steps=3, stats_cols=2, stats_first=1, loss0=True)
    out = ws.summary(ws.fold(ws.Block(), cycle), ppo=True)
    rows = np.vstack([cycle["loss0"][None], cycle["loss"][1:]]).astype(np.float64)
    assert close(out["loss"], rows[:, 0].mean()) and close(out["entropy"], rows[:, 3].mean())
    assert close(out["approx_kl"], cycle["ppo_stats"][1:, 1].astype(np.float64).mean())
    assert "value_clip_fraction" not in out and out["opt_steps"] == out["opt_steps_applied"] == 3
    plain = ws.summary(ws.fold(ws.Block(), make_cycle(rs, 5, 4, 4)))
    assert "approx_kl" not in plain and "opt_steps" not in plain and "truncated_fraction" not in plain


def test_explained_variance_one_zero_and_undefined():
    rs = np.random.RandomState(7)
    cycle = make_cycle(rs, 5, 8, 3)
    ev = lambda **kw: ws.summary(ws.fold(ws.Block(), dict(cycle, **kw)))["explained_variance"]
    assert ev(values=cycle["y"].reshape(5, 8)) == 1.0
    y = np.arange(40, dtype=np.float32)                    # mean 19.5: a float32
    assert ev(y=y, values=np.full((5, 8), 19.5, dtype=np.float32)) == 0.0
    assert ev(y=np.full(40, 0.25, dtype=np.float32)) is None


def test_an_empty_window_has_zero_counts_and_no_means():
    out = ws.summary(ws.Block(), num_actions=4, truncation=True, ppo=True, vclip=True)
    for name, value in out.items():
        if name in ("cycles", "rows", "episodes", "episodes_dropped", "opt_steps", "opt_steps_applied"):
            assert value == 0, name
        elif name == "action_freq":
            assert value == [None] * 4
        else:
            assert value is None, name
    assert not ws.Block().f.any() and not ws.Block().i.any()


def test_ring_cursor_wraps_across_slot_4095():
    rs = np.random.RandomState(9)
    returns, lengths = rs.randn(10).astype(np.float32), rs.randint(1, 50, 10)
    acc = ws.Block()
    acc.set("ring_cursor", 4090)
    ring = make_ring(4100, returns, lengths, first_entry=4090)
    ring[2 + 100] = np.float32(99.0).view(np.int32)        # an old entry: not read
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=ring))
    out = ws.summary(acc)
    assert out["episodes"] == 10 and out["episodes_dropped"] == 0 and acc.get("ring_cursor") == 4100
    r64 = returns.astype(np.float64)
    assert close(out["episode_return_mean"], r64.mean()) and close(out["episode_return_std"], r64.std())
    assert out["episode_return_min"] == float(returns.min()) and out["episode_return_max"] == float(returns.max())
    assert out["episode_length_min"] == lengths.min() and out["episode_length_max"] == lengths.max()
    assert close(out["episode_length_mean"], lengths.mean())
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=ring))       # nothing new: nothing changes
    assert ws.summary(acc)["episodes"] == 10


def test_more_new_entries_than_the_ring_holds_are_counted_as_dropped():
    rs = np.random.RandomState(11)
    returns, lengths = rs.randn(ws.RING).astype(np.float32), rs.randint(1, 50, ws.RING)
    acc = ws.Block()
    acc.set("ring_cursor", 1000)
    ring = make_ring(6000, returns, lengths, first_entry=6000 - ws.RING)
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=ring))
    out = ws.summary(acc)
    assert out["episodes"] == ws.RING and out["episodes_dropped"] == 5000 - ws.RING and acc.get("ring_cursor") == 6000
    assert close(out["episode_return_mean"], returns.astype(np.float64).mean())


def test_min_and_max_come_from_the_first_episode_not_from_the_zeroing():
    rs = np.random.RandomState(13)
    acc = ws.Block()
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=make_ring(1, [-3.0], [7], 0)))
    out = ws.summary(acc)
    assert out["episode_return_max"] == -3.0 and out["episode_return_min"] == -3.0 and out["episode_length_min"] == 7
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=make_ring(3, [-5.0, -1.0], [9, 2], 1)))
    out = ws.summary(acc)
    assert (out["episode_return_min"], out["episode_return_max"]) == (-5.0, -1.0)
    assert (out["episode_length_min"], out["episode_length_max"]) == (2, 9) and out["episodes"] == 3
    # a readout keeps the cursor and forgets the extremes
    acc.reset()
    assert acc.get("ring_cursor") == 3 and not acc.f.any() and acc.i.sum() == 3
    ws.fold(acc, make_cycle(rs, 2, 3, 3, ring=make_ring(4, [2.0], [4], 3)))
    assert ws.summary(acc)["episode_return_min"] == 2.0
    # the host loop's form
    host = ws.fold_episodes(ws.Block(), [-3.0], [7])
    assert ws.summary(host)["episode_return_max"] == -3.0


def test_strided_sum_is_the_stated_order():
    rs = np.random.RandomState(15)
    x = rs.randn(700) * 10.0 ** rs.uniform(-3, 3, 700)
    partial = [0.0] * ws.THREADS
    for i, v in enumerate(x):
        partial[i % ws.THREADS] += v
    total = 0.0
    for p in partial:
        total += p
    assert ws.strided_sum(x) == total and ws.strided_sum([]) == 0.0


def test_field_tables_are_disjoint_and_dense():
    for table, n in ((ws.FIELDS_F, ws.N_F), (ws.FIELDS_I, ws.N_I)):
        taken = sorted(i for at, length in table.values() for i in range(at, at + length))
        assert taken == list(range(n))
    assert ws.FIELDS_I["action_count"][1] == 32 and ws.FIELDS_I["ring_cursor"][0] == ws.N_I - 1
    for name in ("cycles", "rows", "terminals", "truncated", "nonzero_rewards", "opt_steps", "opt_steps_applied", "episodes",
                 "episodes_dropped"):
        assert name in ws.FIELDS_I
    assert not set(ws.FIELDS_F) & set(ws.FIELDS_I)


def test_flag_default_refusals_and_args_json_round_trip(tmp_path):
    from paac_amd import train
    parser = train.get_arg_parser()
    args = parser.parse_args([])
    assert args.window_stats is False and ws.check_flags(args) is False
    assert ws.check_flags(parser.parse_args(["--window_stats", "true"])) is True
    assert "window_stats" in [flag[1] for flag in train.BUILD_FLAGS]
    with pytest.raises(SystemExit):
        parser.parse_args(["--window_stats", "yes"])
    for bad in ("true", 1, None, 0.0):
        with pytest.raises(ValueError, match="--window_stats .*: expected true or false"):
            ws.check_flags(argparse.Namespace(window_stats=bad))
    assert ws.check_flags(argparse.Namespace()) is False                # a Namespace from before the flag
    # one GPU only: on with more than one data-parallel rank is refused, off is not
    with pytest.raises(ValueError, match="not built into the data-parallel cycle.*got 2 ranks"):
        ws.check_flags(argparse.Namespace(window_stats=True), 2)
    assert ws.check_flags(argparse.Namespace(window_stats=False), 2) is False and ws.check_flags(args, 8) is False
    on = parser.parse_args(["--window_stats", "true", "-df", str(tmp_path)])
    train.save_args(on, str(tmp_path))
    saved = json.load(open(os.path.join(str(tmp_path), "args.json")))
    assert saved["window_stats"] is True and ws.check_flags(argparse.Namespace(**saved)) is True
    del saved["window_stats"]
    assert ws.check_flags(argparse.Namespace(**saved)) is False


def test_evaluation_does_not_read_the_flag():
    src = open(os.path.join(os.path.dirname(os.path.abspath(ws.__file__)), "test.py")).read()
    assert "window_stats" not in src
