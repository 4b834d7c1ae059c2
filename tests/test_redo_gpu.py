"""-m gpu: --redo_every (spec and twin: paac_amd/redo.py; contract: include/paac_hip.h, paac_redo).  A process holds one
library, so the user-architecture cases run the same checks in a child process."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from paac_amd import _lib, feature_stats as fs, redo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, ROWS = 3, 8


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def kernel_case(arch_id, optimizer):
    """Checks 1 to 3 of one (architecture, optimizer) on one managed context and one fresh unmanaged one."""
    import torch
    from paac_amd import hip_ops
    dev = torch.device("cuda")
    ctx = hip_ops.Context(arch_id, A, max_batch=ROWS)
    layout, n = ctx.layout, ctx.layout["total"]
    acc_f, acc_i, lay = hip_ops.feature_block(dev, arch_id)
    rs = np.random.RandomState(7)
    host = [np.zeros(n, dtype=np.float32) for _ in range(3)]          # params, slot0, slot1 with zero pads
    for t in layout["tensors"]:
        for h, scale in zip(host, (0.05, 1.0, 1.0)):
            h[t["offset"]:t["offset"] + t["size"]] = scale * rs.randn(t["size"])
    params, s0, s1 = (torch.from_numpy(h).to(dev) for h in host)
    states = torch.from_numpy(rs.randint(0, 256, (ROWS, 84, 84, 4)).astype(np.uint8)).to(dev)
    mask_out, counts_out = (torch.full((k,), -1, dtype=torch.int32, device=dev) for k in (lay.U, 12))
    scalars = torch.zeros(fs.FINISH_SCALARS, dtype=torch.float64, device=dev)
    ctx.set_managed_weights(True)
    ctx.pack_weights(params)
    # 2. a block folded from real activations: the recycled counts are paac_feature_finish's dormant counts
    ctx.train_forward(params, states)
    ctx.feature_fold(lay, acc_f, acc_i, ROWS)
    hip_ops.feature_finish(lay, acc_f, acc_i, 0.5, scalars)
    keep = [t.clone() for t in (params, s0, s1)]
    ctx.redo(*keep, optimizer, lay, acc_f, 0.5, 3, 1, mask_out, counts_out)
    finish, layers = scalars.cpu().numpy(), redo.layers_of_counts(lay, counts_out.cpu().numpy())
    for l, name, units, _ in lay.layers():
        assert layers[name]["units"] == units and layers[name]["recycled"] == (0 if layers[name]["skipped"] else int(finish[2 + 3 * l])), (name, layers, finish)
    assert np.array_equal(mask_out.cpu().numpy(), redo.masks(lay, fs.Block(lay, acc_f.cpu().numpy()), 0.5)[0])
    # 1. hand-set sums: no dormant unit in conv1, unit 0 and the last unit of the other layers and a few between; every unit of
    # the last conv layer fans out to fc rows p * C + c of every position p, across the apply kernel's workgroup spans
    sums, present = 1.0 + rs.rand(lay.U), lay.layers()
    for (_, _, units, at), picks in zip(present[1:], ((0, 5, -1), (0, -1), (0, 5, 6, 7, -1))[3 - len(present[1:]):]):
        sums[at + np.array(picks) % units] = 0.0
    acc_f[:lay.U] = torch.from_numpy(sums).to(dev)
    ctx.redo(params, s0, s1, optimizer, lay, acc_f, 0.025, 3, 2, mask_out, counts_out)
    want_mask, want_layers = redo.masks(lay, fs.Block(lay, acc_f.cpu().numpy()), 0.025)
    counts = redo.recycle(layout, host[0], host[1:], want_mask, 3, 2, optimizer)
    assert want_layers["conv1"]["recycled"] == 0 and want_layers["fc"]["recycled"] == 5 and counts["parameters_redrawn"] > 0
    assert np.array_equal(mask_out.cpu().numpy(), want_mask) and redo.layers_of_counts(lay, counts_out.cpu().numpy()) == want_layers
    for got, want in zip((params, s0, s1), host):          # touched and untouched elements and the pads alike
        assert np.array_equal(bits(got), want.view(np.uint32))
    acc_f[:lay.U] = 0.0          # an empty window: every layer skipped, nothing rewritten
    ctx.redo(params, s0, s1, optimizer, lay, acc_f, 1.0, 3, 3, mask_out, counts_out)
    assert not mask_out.any().item() and counts_out.cpu().numpy().reshape(4, 3)[[l for l, _, _, _ in present], 2].all()
    assert all(np.array_equal(bits(got), want.view(np.uint32)) for got, want in zip((params, s0, s1), host))
    # 3. the managed context's derived copies describe the recycled weights; a recycled fc unit feeds nothing into the heads
    fresh = hip_ops.Context(arch_id, A, max_batch=ROWS)
    out = lambda: (torch.zeros((ROWS, A), device=dev), torch.zeros(ROWS, device=dev))
    (p_m, v_m), (p_f, v_f), (p_x, v_x) = out(), out(), out()
    ctx.forward(params, states, probs=p_m, values=v_m)
    fresh.forward(params, states, probs=p_f, values=v_f)
    assert np.array_equal(bits(p_m), bits(p_f)) and np.array_equal(bits(v_m), bits(v_f)) and p_f.sum().item() > 0
    fc_w = layout["tensors"][2 * len(present) - 2]
    params[fc_w["offset"]:fc_w["offset"] + fc_w["size"]].view(fc_w["shape"])[:, 5] += 0.5          # fc unit 5 was recycled
    fresh.forward(params, states, probs=p_x, values=v_x)
    assert np.array_equal(bits(p_x), bits(p_f)) and np.array_equal(bits(v_x), bits(v_f))
    ctx.close(), fresh.close()


@pytest.mark.parametrize("optimizer", sorted(redo.OPTIMIZERS))
@pytest.mark.parametrize("arch", ["NIPS", "NATURE", "USER"])
def test_recycle_is_the_twins_and_the_copies_follow(arch, optimizer):
    if arch != "USER":
        return kernel_case({"NIPS": _lib.ARCH_NIPS, "NATURE": _lib.ARCH_NATURE}[arch], redo.OPTIMIZERS[optimizer])
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "from paac_amd import _lib, build, networks\n"
              "networks.define_architecture('USER', *build.parse_user_arch(%r))\n"
              "import test_redo_gpu\ntest_redo_gpu.kernel_case(_lib.ARCH_USER, %d)\nprint('REDO_USER_OK')\n"
              % (ROOT, os.path.join(ROOT, "tests"), "16,32,32,256", redo.OPTIMIZERS[optimizer]))          # a geometry the build holds
    res = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "REDO_USER_OK" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])


def test_refusals_launch_nothing():
    import torch
    from paac_amd import hip_ops
    dev = torch.device("cuda")
    ctx = hip_ops.Context(_lib.ARCH_NATURE, 4, max_batch=ROWS)
    acc_f, _, lay = hip_ops.feature_block(dev, _lib.ARCH_NATURE)
    acc_f[1:lay.U] = 1.0                                             # a call that ran would recycle conv1's unit 0
    params, s0, s1, grad = (torch.full((ctx.layout["total"],), 0.01, device=dev) for _ in range(4))
    mask, counts = torch.full((lay.U,), -1, dtype=torch.int32, device=dev), torch.full((12,), -1, dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    units = lambda u: (ctypes.c_int32 * 4)(*u)

    def raw(message, p=params, tau=0.025, optimizer=0, event=1, u=lay.units):
        rc = ctx.lib.paac_redo(ctx.handle, vp(p), vp(s0), vp(s1), optimizer, units(u), vp(acc_f), tau, 3, event, vp(mask), vp(counts),
                               hip_ops._stream())
        assert rc < 0 and message in _lib.load().paac_last_error().decode(), (message, _lib.load().paac_last_error())

    raw("null argument", p=None)
    raw("tau", tau=1.5)
    raw("optimizer 2", optimizer=2)
    raw("counted from 1", event=0)
    raw("do not match the context's geometry", u=(16, 32, 0, 256))
    states = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (ROWS, 84, 84, 4)).astype(np.uint8)).to(dev)
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    ctx.loss_backward(params, states, torch.zeros(ROWS, dtype=torch.int32, device=dev), f32(ROWS), f32(ROWS), 0.02, grad, phase=3)
    raw("slab reduction is still pending")
    ctx.clip_rmsprop(params, grad, s0, s1, f32(1), 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)          # (learning rate 0) consumes it
    ctx.set_managed_weights(True)
    ctx.pack_weights(params)
    mt, N = hip_ops.mt_state_from_numpy(np.random.RandomState(0).get_state(), ctx.device), 4
    ctx.act_step_pipe(params, states[:N], mt, torch.zeros(N, dtype=torch.int32, device=dev), f32(N, 4), f32(N), 1, 0, 0,
                      torch.zeros(1, dtype=torch.int64, device=dev), 0, torch.zeros_like(states[:N]), f32(N), f32(N), f32(N),
                      torch.zeros(N, dtype=torch.int32, device=dev))
    raw("sample is still pending")
    ctx.act_step_flush()
    assert (mask == -1).all().item() and (counts == -1).all().item() and (params == 0.01).all().item()
    ctx.redo(params, s0, s1, 0, lay, acc_f, 0.025, 3, 1, mask, counts)          # ... and the same call, once nothing is in the way
    assert mask[0].item() == 1 and counts[0].item() == 1 and not (params == 0.01).all().item()
    ctx.close()


def loop_records(redo_every):
    from test_window_stats_gpu import catch_args, seeded_learner
    flags = ["--feature_stats", "true", "--dormant_tau", "1.0"] + (["--redo_every", "1"] if redo_every else [])
    learner, _ = seeded_learner(catch_args(flags, emulator_counts=8, max_global_steps=2 * 256 * 8 * 5))
    np.random.seed(9)
    learner.train()
    with open(os.path.join(learner.args.debugging_folder, "metrics.jsonl")) as f:
        return [json.loads(line) for line in f]


def test_device_loop_recycles_at_the_window_boundary():
    on, off = loop_records(True), loop_records(False)
    pick = lambda records, kind: [{k: v for k, v in r.items() if k != "time"} for r in records if r["kind"] == kind]
    redos, features = pick(on, "redo"), pick(on, "features")
    assert len(redos) == 2 and [r["event"] for r in redos] == [1, 2] and not pick(off, "redo")
    for r, f in zip(redos, features):
        assert r["global_step"] == f["global_step"] and r["tau"] == 1.0 and set(r["layers"]) == {"conv1", "conv2", "fc"}
        for layer, got in r["layers"].items():
            dormant = round(f["layers"][layer]["dormant_fraction"] * got["units"])
            assert got["recycled"] == (0 if got["skipped"] else dormant) and (got["skipped"] or got["recycled"] > 0)
        assert r["parameters_redrawn"] > 0 and r["skipped_layers"] == [k for k, v in r["layers"].items() if v["skipped"]]
    first_on, first_off = pick(on, "progress")[0], pick(off, "progress")[0]
    assert set(first_on) == set(first_off) and all(first_on[k] == first_off[k] for k in ("loss", "actor_loss", "critic_loss", "entropy", "grad_norm", "lr"))
    assert pick(on, "features")[0] == pick(off, "features")[0] and pick(on, "features")[1] != pick(off, "features")[1]
