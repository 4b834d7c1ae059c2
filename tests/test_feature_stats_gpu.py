"""-m gpu: --feature_stats (spec and twin: paac_amd/feature_stats.py; contract: include/paac_hip.h, paac_feature_fold).  The
Gram kernel and the unit statistics against float64 numpy, the context route against the copied activations, the loops."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from paac_amd import feature_stats as fs

GEOMETRY = {"NIPS": ((16, 32, 0, 256), ((20, 20), (9, 9))), "NATURE": ((32, 64, 64, 512), ((20, 20), (9, 9), (7, 7)))}
EPS = 2.0 ** -24


def features(rows, H, seed):
    """ReLU of normal draws (about half exact zeros), one column forced to zero and one to a constant."""
    h = np.maximum(np.random.RandomState(seed).randn(rows, H), 0.0).astype(np.float32)
    h[:, 7], h[:, H - 3] = 0.0, 1.25
    return h


def device_fold(lay, block, activations):
    import torch
    from paac_amd import hip_ops
    dev = block[0].device
    hip_ops.feature_fold(lay, block[0], block[1], [None if a is None else torch.from_numpy(a).to(dev) for a in activations])
    torch.cuda.synchronize()
    return fs.Block(lay, block[0].cpu().numpy(), block[1].cpu().numpy())


def assert_gram(got, h, chunk):
    h64 = h.astype(np.float64)
    bound = 4 * (min(h.shape[0], chunk) + 2) * EPS * (np.abs(h64).T @ np.abs(h64))
    err = np.abs(got - h64.T @ h64)
    print("gram %s: worst error / bound %.3g" % (h.shape, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all() and np.array_equal(got, got.T)
    assert not got[7].any() and not got[:, 7].any()


def chunk_rows():
    from paac_amd import hip_ops
    return int(hip_ops.FEATURE_CHUNK_ROWS)


@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("rows", [1, 3, 33, 160, "2 chunks + 5"])
def test_gram_against_float64(H, rows):
    import torch
    from paac_amd import hip_ops
    rows = 2 * chunk_rows() + 5 if isinstance(rows, str) else rows
    lay = fs.Layout((0, 0, 0, H))
    h = features(rows, H, rows)
    got = device_fold(lay, hip_ops.feature_block(torch.device("cuda"), units=lay.units), [None, None, None, h])
    assert_gram(got.gram(), h, chunk_rows())
    assert got.get("rows") == rows and got.get("cycles") == 1 and got.get("samples")[3] == rows
    assert np.array_equal(got.get("pos"), (h > 0).sum(axis=0))


@pytest.mark.parametrize("arch", sorted(GEOMETRY))
@pytest.mark.parametrize("rows", [3, 33])
def test_unit_statistics_and_accumulation(arch, rows):
    """Two folds (rows, then 2 chunks + 5 rows of fc features alone) against the reference of the concatenation; then finish,
    empty, and the first fold again: bit for bit a fresh block's."""
    import torch
    from paac_amd import hip_ops
    units, planes = GEOMETRY[arch]
    lay, rs = fs.Layout(units), np.random.RandomState(rows)
    n_terms = int(hip_ops.FEATURE_UNIT_FP32_TERMS)
    acts = [np.maximum(rs.randn(rows, oh, ow, c), 0.0).astype(np.float32) for (oh, ow), c in zip(planes, units)]
    acts += [None] * (3 - len(acts)) + [features(rows, units[3], rows + 1)]
    block = hip_ops.feature_block(torch.device("cuda"), units=units)
    first = device_fold(lay, block, acts)
    for l, _, c, at in lay.layers():
        a = acts[l].reshape(-1, c).astype(np.float64)
        assert np.array_equal(first.get("pos")[at:at + c], (a > 0).sum(axis=0)) and first.get("samples")[l] == a.shape[0]
        assert (np.abs(first.get("sum")[at:at + c] - a.sum(axis=0)) <= 4 * (n_terms + 2) * EPS * np.abs(a).sum(axis=0)).all()
    more = features(2 * chunk_rows() + 5, units[3], 5)
    both = device_fold(lay, block, [None, None, None, more])
    assert_gram(both.gram(), np.concatenate([acts[3], more]), chunk_rows())
    assert both.get("rows") == rows + more.shape[0] and both.get("cycles") == 2 and both.get("samples")[0] == rows * 400
    # the finish launch against its twin, to the bit; then a fold into the emptied block
    scalars = torch.zeros(fs.FINISH_SCALARS, dtype=torch.float64, device="cuda")
    hip_ops.feature_finish(lay, block[0], block[1], 0.025, scalars)
    got, want = scalars.cpu().numpy(), fs.finish(both, 0.025)
    print("finish scalars that differ:", [(int(k), repr(got[k]), repr(want[k])) for k in np.nonzero(got != want)[0]])
    assert np.array_equal(got, want)
    block[0][:lay.LIVE_F].zero_()
    block[1][:lay.LIVE_I].zero_()
    again = device_fold(lay, block, acts)
    assert np.array_equal(again.f, first.f) and np.array_equal(again.i, first.i)


@pytest.mark.parametrize("arch,rows", [("NIPS", 8), ("NATURE", 40)])
def test_context_route_equals_the_copied_activations(arch, rows):
    import torch
    from paac_amd import _lib, hip_ops
    arch_id = {"NIPS": _lib.ARCH_NIPS, "NATURE": _lib.ARCH_NATURE}[arch]
    dev = torch.device("cuda")
    ctx = hip_ops.Context(arch_id, 4, max_batch=80)
    rs = np.random.RandomState(rows)
    params = torch.from_numpy((0.05 * rs.randn(ctx.layout["total"])).astype(np.float32)).to(dev)
    states = torch.from_numpy(rs.randint(0, 256, (80, 84, 84, 4)).astype(np.uint8)).to(dev)
    lay = hip_ops.feature_layout(arch_id)
    assert lay.units == GEOMETRY[arch][0]
    block = hip_ops.feature_block(dev, arch_id)
    ctx.train_forward_trunk(params, states)          # (80 rows: above the small-batch tail, the heads stay pending)
    with pytest.raises(_lib.PaacHipError, match="pending"):
        ctx.feature_fold(lay, block[0], block[1], rows)
    states = states[:rows]
    ctx.train_forward(params, states)
    with pytest.raises(_lib.PaacHipError, match="max_batch"):
        ctx.feature_fold(lay, block[0], block[1], 81)
    ctx.feature_fold(lay, block[0], block[1], rows)
    copies = [ctx.debug_activation(21 + l, rows).view(rows, -1, lay.units[l]) if lay.units[l] else None for l in range(3)]
    copies.append(ctx.debug_activation(24, rows).view(rows, lay.H))
    other = hip_ops.feature_block(dev, arch_id)
    hip_ops.feature_fold(lay, other[0], other[1], copies)
    torch.cuda.synchronize()
    a, b = (fs.Block(lay, k[0].cpu().numpy(), k[1].cpu().numpy()) for k in (block, other))
    assert np.array_equal(a.f, b.f) and np.array_equal(a.i, b.i) and a.get("rows") == rows and a.gram().any()
    assert a.get("pos")[-lay.H:].sum() == (copies[3] > 0).sum().item()
    ctx.close()


def test_entry_refusals_launch_nothing():
    import torch
    from paac_amd import _lib, hip_ops
    lay = fs.Layout((0, 0, 0, 256))
    block = hip_ops.feature_block(torch.device("cuda"), units=lay.units)
    h = torch.ones((4, 256), dtype=torch.float32, device="cuda")
    inside = block[0].view(torch.float32)[:4 * 256].view(4, 256)
    with pytest.raises(_lib.PaacHipError, match="overlaps"):
        hip_ops.feature_fold(lay, block[0], block[1], [None, None, None, inside])
    with pytest.raises(_lib.PaacHipError, match="tau"):
        hip_ops.feature_finish(lay, block[0], block[1], 2.0, torch.zeros(fs.FINISH_SCALARS, dtype=torch.float64, device="cuda"))
    for units, message in (((0, 0, 0, 96), "multiple of 64"), ((24, 0, 0, 256), "multiple of 16")):
        raw = _lib.FeatureInputs()
        raw.rows, raw.act[3] = 4, h.data_ptr()
        for l in range(4):
            raw.units[l], raw.positions[l] = units[l], 1
        assert _lib.load().paac_feature_fold(ctypes.byref(raw), block[0].data_ptr(), block[1].data_ptr(), None) == -1
        assert message in _lib.load().paac_last_error().decode()
    torch.cuda.synchronize()
    assert not block[0].any() and not block[1].any()


def loop_run(use_graph, cycles=4, **flags):
    from paac_amd.paac import DeviceRollout
    from test_window_stats_gpu import catch_args, seeded_learner
    on = flags.pop("on", "true")
    L, env_creator = seeded_learner(catch_args(["--feature_stats", on], **flags))
    L.global_step = L.init_network()
    ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=use_graph)
    assert (ro.features is not None) == (on == "true")
    if use_graph:
        ro.run_cycles(cycles)
    else:
        for _ in range(cycles):
            ro.run_cycle()
    ro.synchronize()
    state = [t.cpu().numpy().copy() for _, t in L.update_state] + [t.cpu().numpy().copy() for t in (ro.actions, ro.values, ro.y, ro.tick)]
    block = record = None
    if ro.features is not None:
        block = fs.Block(ro.features[2], ro.features[0].cpu().numpy(), ro.features[1].cpu().numpy())
        record = L._feature_read(ro.features)[0]
        assert not ro.features[0][:block.layout.LIVE_F].any().item()
    ro.close()
    L.ctx.close()
    return state, block, record


@pytest.mark.parametrize("flags", [{}, dict(ppo_epochs=2, ppo_minibatches=2)], ids=["a3c", "minibatch ppo"])
def test_device_loop_is_neutral_deterministic_and_recorded(flags):
    off, _, _ = loop_run(True, on="false", **flags)
    on, captured, record = loop_run(True, **flags)
    _, eager, _ = loop_run(False, **flags)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))
    assert np.array_equal(captured.f, eager.f) and np.array_equal(captured.i, eager.i)
    assert captured.get("cycles") == 4 and captured.get("rows") == 80 and captured.gram().any()
    assert record == fs.summary(captured.layout, fs.finish(captured, 0.025), 0.025)
    assert set(record["layers"]) == {"conv1", "conv2", "fc"} and 0.0 < record["layers"]["fc"]["active_fraction"] < 1.0
    assert 1.0 <= record["fc_participation_ratio"] <= 256.0


def test_host_loop_writes_the_same_record_fields():
    from test_window_stats_gpu import N, T, catch_args, seeded_learner
    args = catch_args(["--feature_stats", "true", "--host_environments", "true", "--feature_rank_every", "1"],
                      max_global_steps=3 * N * T)
    learner, _ = seeded_learner(args)
    np.random.seed(9)
    learner.train()
    record = learner._feature_read(learner.host_features)[0]
    assert record["cycles"] == 3 and record["rows"] == 3 * N * T and record["tau"] == 0.025
    assert set(record) == {"cycles", "rows", "tau", "layers", "fc_participation_ratio", "fc_srank", "fc_top_eigen_share"}
    assert 1 <= record["fc_srank"] <= 256 and set(record["layers"]["conv1"]) == {"units", "dormant_fraction", "dead_fraction",
                                                                                 "active_fraction"}


@pytest.mark.parametrize("argv,world", [(["--feature_stats", "true"], 2), (["--feature_stats", "true", "--dormant_tau", "2"], 1)])
def test_flags_are_refused_at_start_up(argv, world):
    from paac_amd import train
    with pytest.raises(ValueError):
        fs.check_flags(train.get_arg_parser().parse_args(["--emulator", "catch"] + argv), world)
    with pytest.raises(SystemExit):
        train.get_arg_parser().parse_args(["--feature_stats", "maybe"])
