"""--adv_norm: each rollout's advantages normalised by their own mean and population standard deviation before the actor term
reads them.  The reference has no counterpart, so the checker is this file's float64 restatement of the contract in
include/paac_hip.h.  Bars: adv_n within 1 fp32 ulp per element and mean / std within 1e-12 relative -- an fp64 sum of at most
2688 terms, reordered, moves the quotient by far less than 2^-24, so only the final rounding to fp32 can flip; y, raw adv and the
schedule bookkeeping of the one-launch form equal the existing entries' bit for bit."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


# -- the restatement ---------------------------------------------------------------------------------------------------

def adv_norm_restated(adv):
    """fp32 adv -> (adv_n fp32, mean, std): fp64, population form, two passes; std == 0 gives zeros."""
    a = np.asarray(adv, dtype=np.float32).astype(np.float64).reshape(-1)
    mean = a.sum() / a.size
    std = np.sqrt(((a - mean) ** 2).sum() / a.size)
    if std == 0.0:
        return np.zeros(a.size, dtype=np.float32), mean, std
    return ((a - mean) / (std + 1e-8)).astype(np.float32), mean, std


def ulps(got, want):
    """Distance in fp32 units in the last place of `want` (0 where both are equal, sign of zero included)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def norm_cases():
    """name -> fp32 advantages: the sizes and the two designed inputs the contract names."""
    rs = np.random.RandomState(0)
    cases = {"B%d" % B: (2.0 * rs.randn(B) + 0.3).astype(np.float32) for B in (1, 15, 40, 160, 2688)}
    cases["all_equal"] = np.full(40, np.float32(0.7), dtype=np.float32)
    cases["offset_1e4"] = (1e4 + 1e-3 * rs.randn(160)).astype(np.float32)
    return cases


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_flag_defaults_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    d = p.parse_args([])
    assert d.adv_norm is False
    a = p.parse_args(["--adv_norm", "true"])
    assert a.adv_norm is True and p.parse_args(["--adv_norm", "False"]).adv_norm is False
    flag = [f for f in train.BUILD_FLAGS if f[0] == ("--adv_norm",)][0]
    assert flag[3] is train.bool_arg and flag[2] is False
    logger_utils.save_args(a, str(tmp_path))
    assert logger_utils.load_args(str(tmp_path / "args.json"))["adv_norm"] is True


def test_cli_refuses_a_non_bool_string():
    from paac_amd import train
    with pytest.raises(SystemExit):
        train.get_arg_parser().parse_args(["--adv_norm", "yes"])


def test_evaluation_reads_neither_flag():
    src = open(os.path.join(ROOT, "paac_amd", "test.py")).read()
    assert "adv_norm" not in src and "ppo_vclip" not in src


@pytest.mark.parametrize("bad", ["true", 1, None, 0.5])
def test_actor_learner_refuses_a_non_bool(bad):
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    args.adv_norm = bad
    args.num_actions = 4
    with pytest.raises(ValueError, match="adv_norm"):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_header_declares_the_entries():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, nargs, must in (("paac_adv_normalize", 5, ("const float* adv", "int B", "float* adv_n_out", "double* stats_out")),
                              ("paac_returns_norm_tick", 6, ("const paac_returns* ret", "float* adv_n_out", "double* stats_out"))):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name + " missing from the header"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs
        assert all(t in m.group(1) for t in must) and name in _lib.EXPORTED_SYMBOLS
    assert _lib.Returns._fields_[-1][0] == "gae_lambda"                # paac_returns itself is unchanged
    for text in ("std + 1e-8", "sum((adv - mean)^2) / B", "std == 0", "Only the actor term reads adv_n"):
        assert text in hdr, text


def test_restatement_properties():
    cases = norm_cases()
    for name in ("B1", "all_equal"):
        out, _, std = adv_norm_restated(cases[name])
        assert std == 0.0 and not out.any(), name
    out, mean, std = adv_norm_restated(cases["B2688"])
    assert abs(out.astype(np.float64).mean()) < 1e-6 and abs(out.astype(np.float64).std() - 1.0) < 1e-6
    # the designed offset case is one where the two-pass form matters: the one-pass E[x^2] - mean^2 in fp64 loses the spread
    a = cases["offset_1e4"].astype(np.float64)
    one_pass = np.sqrt(max((a * a).sum() / a.size - (a.sum() / a.size) ** 2, 0.0))
    _, _, two_pass = adv_norm_restated(cases["offset_1e4"])
    assert two_pass > 0 and abs(one_pass - two_pass) > 1e-9 * two_pass
    assert np.isnan(adv_norm_restated(np.array([1.0, np.nan, 2.0], dtype=np.float32))[0]).all()


# -- GPU: the two entries ----------------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(norm_cases()))
def test_adv_normalize_against_the_restatement(name):
    import torch
    from paac_amd import hip_ops
    adv = norm_cases()[name]
    want, mean, std = adv_norm_restated(adv)
    a = dev(adv)
    out, stats = [torch.full_like(a, 7.0) for _ in range(2)], [torch.zeros(2, dtype=torch.float64, device="cuda") for _ in range(2)]
    for o, s in zip(out, stats):
        hip_ops.adv_normalize(a, o, s)
    torch.cuda.synchronize()
    got, st = out[0].cpu().numpy(), stats[0].cpu().numpy()
    print("%s: B %d mean %r / %r std %r / %r max ulps %g" % (name, adv.size, st[0], mean, st[1], std, ulps(got, want).max()))
    assert torch.equal(out[0], out[1]) and torch.equal(stats[0], stats[1])         # two launches: the same bits
    assert abs(st[0] - mean) <= 1e-12 * abs(mean) and abs(st[1] - std) <= 1e-12 * abs(std)
    assert ulps(got, want).max() <= 1.0
    if name in ("B1", "all_equal"):
        assert st[1] == 0.0 and not got.any()
    # in place, and without the statistics
    hip_ops.adv_normalize(a, a)
    assert torch.equal(a, out[0])


@pytest.mark.gpu
def test_adv_normalize_propagates_non_finite_inputs():
    import torch
    from paac_amd import hip_ops
    for bad in (np.nan, np.inf):
        adv = np.arange(40, dtype=np.float32)
        adv[7] = bad
        out = torch.zeros(40, device="cuda")
        hip_ops.adv_normalize(dev(adv), out)
        assert not torch.isfinite(out).any(), bad


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(5, 8), (20, 4)])
@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_returns_norm_tick_equals_the_tick_entries_and_adv_normalize(T, N, lam):
    import torch
    from paac_amd import hip_ops
    from test_gae import records
    v_boot, r, m, V = [dev(a) for a in records(T, N, 3)]
    B = T * N

    def fresh():
        return dict(y=torch.zeros(B, device="cuda"), adv=torch.zeros(B, device="cuda"),
                    gs=torch.tensor([12345], dtype=torch.int64, device="cuda"), lr=torch.zeros(1, device="cuda"),
                    tick=torch.tensor([77], dtype=torch.int64, device="cuda"))
    a, b = fresh(), fresh()
    if hip_ops.uses_gae(lam):
        hip_ops.gae_returns_tick(v_boot, r, m, V, 0.99, lam, a["y"], a["adv"], a["gs"], B, 0.0224, 80000000, a["lr"], a["tick"], T)
    else:
        hip_ops.nstep_returns_tick(v_boot, r, m, V, 0.99, a["y"], a["adv"], a["gs"], B, 0.0224, 80000000, a["lr"], a["tick"], T)
    adv_n, stats = torch.zeros(B, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    hip_ops.returns_norm_tick(v_boot, r, m, V, 0.99, b["y"], b["adv"], adv_n, stats, global_step_dev=b["gs"], increment=B,
                              initial_lr=0.0224, lr_annealing_steps=80000000, lr_out_dev=b["lr"], tick_dev=b["tick"],
                              tick_inc=T, gae_lambda=lam)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(b["gs"].item()) == 12345 + B and int(b["tick"].item()) == 77 + T and float(b["lr"].item()) > 0
    want_n, want_s = torch.zeros(B, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    hip_ops.adv_normalize(a["adv"], want_n, want_s)
    assert torch.equal(adv_n, want_n) and torch.equal(stats, want_s) and float(stats[1].item()) > 0
    # without the bookkeeping (every pointer of it NULL): the same returns and normalisation, nothing else written
    c = fresh()
    adv_n2 = torch.zeros(B, device="cuda")
    hip_ops.returns_norm_tick(v_boot, r, m, V, 0.99, c["y"], c["adv"], adv_n2, gae_lambda=lam)
    assert torch.equal(c["y"], a["y"]) and torch.equal(adv_n2, adv_n) and int(c["gs"].item()) == 12345


# -- GPU: the loops ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_flags_off_is_the_parent_behaviour():
    """Both flags at their defaults against a Namespace that never had the attributes: one cycle's weights bit for bit."""
    from test_gae import run_device_loop

    def run(strip):
        from test_learner_gpu import build_learner
        from test_gae import learner_state, loop_args
        from paac_amd.paac import DeviceRollout
        args = loop_args(game="breakout", arch="NATURE", emulator_counts=8, emulator_workers=0, max_local_steps=5,
                         max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="numpy", test_seed=11, ppo_epochs=2)
        if strip:
            del args.adv_norm, args.ppo_vclip
        learner, _, env_creator = build_learner(args)
        np.random.seed(args.test_seed)
        learner.global_step = learner.init_network()
        assert learner.adv_norm is False and learner.vclip_on is False and learner.adv_n is None and learner.v_old is None
        assert tuple(learner.ppo_stats.shape) == (2, 2)
        ro = DeviceRollout(learner, env_creator.device_env_spec, sampler="numpy", use_graph=True)
        ro.run_cycle()
        ro.synchronize()
        out = learner_state(learner)
        ro.close()
        return out
    assert all(np.array_equal(a, b) for a, b in zip(run(False), run(True)))
    a = run_device_loop(8, 5, "numpy", 1)
    b = run_device_loop(8, 5, "numpy", 1, adv_norm=True)
    assert not np.array_equal(a["state"][0], b["state"][0])            # the flag reaches the update
    assert all(np.array_equal(x, y) for x, y in zip(a["y"][0], b["y"][0]))      # ... and leaves y and the recorded adv alone


@pytest.mark.gpu
@pytest.mark.parametrize("lam", [1.0, 0.95])
def test_adv_norm_alone_in_the_device_loop(lam):
    """--adv_norm true at K = 1: graph replay equals eager over 3 cycles; after each cycle adv_n is the restatement of the
    loop's own recorded advantages (1 ulp), the statistics are theirs, and global_step advances as without the flag."""
    from test_gae import run_device_loop
    N, T, cycles = 32, 5, 3

    def check(learner, ro, c):
        want, mean, std = adv_norm_restated(ro.adv.cpu().numpy())
        st = learner.adv_stats.cpu().numpy()
        assert abs(st[0] - mean) <= 1e-12 * abs(mean) and abs(st[1] - std) <= 1e-12 * abs(std) and std > 0
        assert ulps(learner.adv_n.cpu().numpy(), want).max() <= 1.0

    graph = run_device_loop(N, T, "numpy", cycles, use_graph=True, check=check, adv_norm=True, gae_lambda=lam)
    eager = run_device_loop(N, T, "numpy", cycles, use_graph=False, adv_norm=True, gae_lambda=lam)
    assert all(np.array_equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    assert all(np.isfinite(a).all() for a in graph["state"])
    assert graph["global_step"] == eager["global_step"] == cycles * N * T and graph["lr"] == eager["lr"]


@pytest.mark.gpu
def test_adv_norm_in_the_host_loop():
    """The host-plugin loop: the feed keeps y and the raw adv (they equal the run without the flag on the first cycle, whose
    weights are the same), the actor term read their normalisation, and the weights differ from the run without the flag."""
    from test_gae import run_host_loop
    la, fa, a = run_host_loop(2)
    lb, fb, b = run_host_loop(2, adv_norm=True)
    assert np.array_equal(fa[0]["adv"], fb[0]["adv"]) and np.array_equal(fa[0]["y"], fb[0]["y"])
    assert not np.array_equal(a[0], b[0]) and all(np.isfinite(x).all() for x in b)
    want, mean, std = adv_norm_restated(fb[-1]["adv"])
    assert ulps(lb.adv_n.cpu().numpy(), want).max() <= 1.0
    st = lb.adv_stats.cpu().numpy()
    assert abs(st[0] - mean) <= 1e-12 * abs(mean) and abs(st[1] - std) <= 1e-12 * abs(std)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [False, True])
def test_metrics_record_appears_only_with_the_flag(tmp_path, on):
    import json
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    N, T = 32, 5
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=64 * N * T, synthetic_terminal_p=0.1, sampler="philox", adv_norm=on,
                     debugging_folder=str(tmp_path))
    L, _, _ = build_learner(args)
    L.train()
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    norm = [r for r in recs if "std" in r and "mean" in r and "steps_per_s" not in r and "max" not in r]
    progress = [r for r in recs if "steps_per_s" in r]
    assert len(progress) >= 1 and len(norm) == (len(progress) if on else 0)
    assert all(np.isfinite(r["mean"]) and r["std"] > 0 for r in norm)
    assert all({"lr", "grad_norm", "loss", "actor_loss", "critic_loss", "entropy"} <= set(r) for r in progress)
