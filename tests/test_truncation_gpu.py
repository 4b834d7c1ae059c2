"""--bootstrap_truncated on the GPU: the truncation-aware scans against the float64 restatement of tests/test_truncation.py (bit
for bit: every operation is individually rounded, the bar test_nstep_returns_bit_exact holds the n-step scan to), the game
step's truncation plane against the games' specs, and the loops with the flag on and off."""
import os
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from paac_amd import bricks, rally                                                          # noqa: E402
from test_adv_norm import adv_norm_restated, ulps                                             # noqa: E402  (--adv_norm's own bar)
from test_truncation import returns_restated, trunc_records, B as BS, R as RS                # noqa: E402

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SHAPES = [(5, 4), (12, 3)]                  # T = 12 exceeds the 8-step preload / chunk: the tail behind it runs
LAMBDAS = [(None, None), ("gae", 0.0), ("gae", 0.95), ("gae", 1.0), (None, 1.0)]      # (forced estimator, lambda)
TICK = dict(increment=160, initial_lr=0.0224, lr_annealing_steps=80000000, tick_inc=5)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def restated(host, est, lam):
    """The restatement for a (forced estimator, lambda) pair: forced GAE runs GAE at lambda = 1 too."""
    from test_truncation import gae_trunc_restated
    if est == "gae":
        return gae_trunc_restated(*host, GAMMA, lam)
    return returns_restated(*host, GAMMA, lam)


def new_tick():
    import torch
    return dict(global_step_dev=torch.tensor([1000], dtype=torch.int64, device="cuda"), lr_out_dev=torch.zeros(1, device="cuda"),
                tick_dev=torch.tensor([7], dtype=torch.int64, device="cuda"), **TICK)


# -- the scans: standalone entry, with and without the tick --------------------------------------------------------------

@pytest.mark.parametrize("T,N", SHAPES)
@pytest.mark.parametrize("est,lam", LAMBDAS)
def test_returns_scan_bit_exact_with_and_without_the_tick(T, N, est, lam):
    import torch
    from oracle import rollout as oroll
    from paac_amd import hip_ops
    for seed in (1, 2):
        host = trunc_records(T, N, 10 * T + seed)
        v_boot, r, m, V, tr = [dev(a) for a in host]
        ye, ae = restated(host, est, lam)
        y, adv = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
        hip_ops.returns_scan(v_boot, r, m, V, GAMMA, y, adv, lam, tr, estimator=est)
        assert np.array_equal(y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(adv.cpu().numpy(), ae.reshape(-1))
        y2, adv2, tick = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda"), new_tick()
        hip_ops.returns_scan(v_boot, r, m, V, GAMMA, y2, adv2, lam, tr, estimator=est, **tick)
        assert torch.equal(y, y2) and torch.equal(adv, adv2)
        assert int(tick["global_step_dev"].item()) == 1160 and int(tick["tick_dev"].item()) == 12
        assert tick["lr_out_dev"].item() == np.float32(oroll.get_lr(1160, 0.0224, 80000000))
        # the plane matters: the same records without it give other numbers at and upstream of the truncated steps
        hip_ops.returns_scan(v_boot, r, m, V, GAMMA, y2, adv2, lam, None, estimator=est)
        assert not torch.equal(y, y2)


@pytest.mark.parametrize("T,N", SHAPES + [(20, 130)])
def test_zero_plane_and_no_plane_give_the_old_entries_bits(T, N):
    """An all-zero plane through the truncation-aware kernels, and no plane through the plain ones, against
    paac_nstep_returns[_tick] / paac_gae_returns[_tick] on the same inputs."""
    import torch
    from paac_amd import hip_ops
    host = trunc_records(T, N, 3)
    v_boot, r, m, V, _ = [dev(a) for a in host]
    zero = torch.zeros((T, N), device="cuda")
    for lam in (None, 0.0, 0.95):
        want = [torch.zeros(T * N, device="cuda") for _ in range(2)]
        hip_ops.returns(v_boot, r, m, V, GAMMA, want[0], want[1], lam)
        t_old = new_tick()
        want_t = [torch.zeros(T * N, device="cuda") for _ in range(2)]
        hip_ops.returns_tick(v_boot, r, m, V, GAMMA, want_t[0], want_t[1], lam, **t_old)
        for plane in (zero, None):
            got = [torch.zeros(T * N, device="cuda") for _ in range(2)]
            hip_ops.returns_scan(v_boot, r, m, V, GAMMA, got[0], got[1], lam, plane)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (lam, plane is None)
            t_new = new_tick()
            hip_ops.returns_scan(v_boot, r, m, V, GAMMA, got[0], got[1], lam, plane, **t_new)
            assert torch.equal(got[0], want_t[0]) and torch.equal(got[1], want_t[1]), (lam, plane is None)
            for k in ("global_step_dev", "lr_out_dev", "tick_dev"):
                assert torch.equal(t_new[k], t_old[k]), k
        # --adv_norm's launch
        old = [torch.zeros(T * N, device="cuda") for _ in range(3)]
        hip_ops.returns_norm_tick(v_boot, r, m, V, GAMMA, *old, gae_lambda=lam)
        new = [torch.zeros(T * N, device="cuda") for _ in range(3)]
        hip_ops.returns_norm_tick(v_boot, r, m, V, GAMMA, *new, gae_lambda=lam, truncs=zero)
        assert all(torch.equal(a, b) for a, b in zip(old, new)), lam


@pytest.mark.parametrize("T,N", SHAPES)
@pytest.mark.parametrize("lam", [None, 0.0, 0.95])
def test_adv_norm_launch_with_a_plane(T, N, lam):
    """paac_returns_norm_tick with a plane: y / adv are the standalone scan's bits, adv_n the bits paac_adv_normalize gives on
    them and what the restatement of --adv_norm computes from them (to the bar of tests/test_adv_norm.py: fp64 division and
    square root are not bitwise numpy's, so 1e-12 relative on the statistics and one fp32 ulp on adv_n), the bookkeeping the
    tick's."""
    import torch
    from paac_amd import hip_ops
    host = trunc_records(T, N, 40 + T)
    v_boot, r, m, V, tr = [dev(a) for a in host]
    y, adv, adv_n = [torch.zeros(T * N, device="cuda") for _ in range(3)]
    stats, tick = torch.zeros(2, dtype=torch.float64, device="cuda"), new_tick()
    hip_ops.returns_norm_tick(v_boot, r, m, V, GAMMA, y, adv, adv_n, stats, gae_lambda=lam, truncs=tr, **tick)
    y2, adv2 = torch.zeros(T * N, device="cuda"), torch.zeros(T * N, device="cuda")
    hip_ops.returns_scan(v_boot, r, m, V, GAMMA, y2, adv2, lam, tr)
    assert torch.equal(y, y2) and torch.equal(adv, adv2)
    ye, ae = returns_restated(*host, GAMMA, lam)
    assert np.array_equal(y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(adv.cpu().numpy(), ae.reshape(-1))
    alone, stats2 = torch.zeros(T * N, device="cuda"), torch.zeros(2, dtype=torch.float64, device="cuda")
    hip_ops.adv_normalize(adv2, alone, stats2)
    assert torch.equal(adv_n, alone) and torch.equal(stats, stats2)
    want, mean, sd = adv_norm_restated(ae)
    st = stats.cpu().numpy()
    assert abs(st[0] - mean) <= 1e-12 * abs(mean) and abs(st[1] - sd) <= 1e-12 * abs(sd) and sd > 0
    assert ulps(adv_n.cpu().numpy(), want).max() <= 1.0
    assert int(tick["global_step_dev"].item()) == 1160 and int(tick["tick_dev"].item()) == 12


# -- the returns inside the backward's first launch ----------------------------------------------------------------------

def upload(ctx, params):
    import torch
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = params[t["name"]].reshape(-1)
    return torch.from_numpy(flat).cuda()


@pytest.mark.parametrize("T,N", [(5, 4), (12, 3)])           # T*N = 20; and T = 12: the tail behind the preloaded steps
@pytest.mark.parametrize("lam", [None, 0.95])
def test_in_launch_rescan_equals_the_standalone_scan(T, N, lam):
    """NIPS, 20 rows (and 36, where T = 12 exceeds the preload): y / adv written by the loss-backward's first launch on the three routes to it (v_boot given after a whole
    training forward; bootstrap rows of a trunk-only forward; kept acting rows), with and without the p_old record, equal the
    standalone scan's bits on the same records -- and, with a zero plane, the launch without one: y, adv, gradient, loss."""
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    A, Bn = 4, T * N
    rs = np.random.RandomState(5)
    ctx = hip_ops.Context(0, A, max_batch=Bn + N)
    p = upload(ctx, onet.init_params("NIPS", A, rs, dtype=np.float32))
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    states = dev(rs.randint(0, 256, (Bn + N, 84, 84, 4)).astype(np.uint8))
    acts = dev(rs.randint(0, A, Bn).astype(np.int32))
    _, r, m, _, tr = trunc_records(T, N, 77)
    r, m, tr = dev(r), dev(m), dev(tr)
    n = ctx.layout["total"]
    values, probs = torch.zeros((T, N), device="cuda"), torch.zeros((N, A), device="cuda")

    def prepare(route):
        if route == "given":
            vt = torch.zeros(Bn + N, device="cuda")
            ctx.train_forward(p, states, values=vt)
            return vt[Bn:].clone()
        for t in range(T):
            if route == "kept":
                ctx.keep_next_forward(t * N)
            ctx.forward(p, states[t * N:(t + 1) * N], probs=probs, values=values[t])
        if route == "kept":
            ctx.bootstrap_forward_trunk(p, states[Bn:], Bn)
        else:
            ctx.train_forward_trunk(p, states)
        return None

    def backward(route, plane, record):
        out = dict(y=torch.zeros(Bn, device="cuda"), adv=torch.zeros(Bn, device="cuda"), grad=torch.zeros(n, device="cuda"),
                   loss=torch.zeros(4, device="cuda"), p_old=torch.zeros(Bn, device="cuda") if record else None, tick=new_tick())
        vb = prepare(route)
        ctx.loss_backward_returns(p, states[:Bn], acts, vb, r, m, values, GAMMA, out["y"], out["adv"], 0.02, out["grad"],
                                  out["loss"], forward_done=True, gae_lambda=lam, p_old_out=out["p_old"], truncs=plane,
                                  **out["tick"])
        torch.cuda.synchronize()
        out["vb"] = vb if vb is not None else ctx.debug_activation(25, Bn + N)[Bn:].clone()
        return out

    prepare("trunk")                            # fills `values`
    ctx.loss_backward(p, states[:Bn], acts, torch.zeros(Bn, device="cuda"), torch.zeros(Bn, device="cuda"), 0.02,
                      torch.zeros(n, device="cuda"), forward_done=True)
    assert float(values.min()) < 0 or float(values.abs().max()) > 0
    for route in ("given", "trunk", "kept"):
        for record in (False, True):
            got = backward(route, tr, record)
            y2, adv2 = torch.zeros(Bn, device="cuda"), torch.zeros(Bn, device="cuda")
            hip_ops.returns_scan(got["vb"], r, m, values, GAMMA, y2, adv2, lam, tr)
            assert torch.equal(got["y"], y2) and torch.equal(got["adv"], adv2), (route, record)
            ye, ae = returns_restated(got["vb"].cpu().numpy(), r.cpu().numpy(), m.cpu().numpy(), values.cpu().numpy(),
                                      tr.cpu().numpy(), GAMMA, lam)
            assert np.array_equal(y2.cpu().numpy(), ye.reshape(-1)) and np.array_equal(adv2.cpu().numpy(), ae.reshape(-1))
            assert int(got["tick"]["global_step_dev"].item()) == 1160 and int(got["tick"]["tick_dev"].item()) == 12
            # the gradient is the plain backward's on those y / adv
            prepare(route)
            grad2, loss2 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            ctx.loss_backward(p, states[:Bn], acts, y2, adv2, 0.02, grad2, loss2, forward_done=True)
            torch.cuda.synchronize()
            assert torch.equal(got["grad"], grad2) and torch.equal(got["loss"], loss2), (route, record)
            # a zero plane (truncation-aware kernels) == no plane (the kernels from before the flag)
            zero, none = backward(route, torch.zeros_like(tr), record), backward(route, None, record)
            for k in ("y", "adv", "grad", "loss") + (("p_old",) if record else ()):
                assert torch.equal(zero[k], none[k]), (route, record, k)
            assert not torch.equal(none["y"], got["y"])
    ctx.close()


# -- the game step ---------------------------------------------------------------------------------------------------------

def game_buffers(kind, records, history):
    import torch
    from paac_amd import hip_ops
    N, W = len(records), hip_ops.DEVICE_GAMES[kind]["words"]
    words = np.array([list(s) + [0] * (W - len(s)) for s in records], dtype=np.int32)
    return dict(state=[dev(words), torch.zeros((N, W), dtype=torch.int32, device="cuda")],
                stack=[dev(history), torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")],
                rew=torch.zeros(N, device="cuda"), msk=torch.zeros(N, device="cuda"), ep_r=torch.zeros(N, device="cuda"),
                ep_l=torch.zeros(N, dtype=torch.int32, device="cuda"),
                fin=torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device="cuda"))


def drained(fin):
    """The finished-episode ring as (count, sorted (reward, length) pairs): environments that end on the same step take their
    slots in whatever order their workgroups reach the counter."""
    host = fin.cpu().numpy()
    n = int(host[0])
    return n, sorted(zip(host[2:2 + n].view(np.float32).tolist(), host[2 + 4096:2 + 4096 + n].tolist()))


CAP_STATES = {
    "bricks": (bricks, [BS(5, 8, 1, 1, 9, steps=bricks.MAX_STEPS - 2),                     # the cap alone
                        BS(5, 11, 1, 1, 9, lives=1, steps=bricks.MAX_STEPS - 2),           # the last life goes on the cap step
                        BS(5, 6, 1, -1, 9, steps=bricks.MAX_STEPS - 2, k=3),               # a brick struck on the cap step
                        BS(5, 8, 1, 1, 9, steps=10)], {}),                                 # far from the cap
    "rally": (rally, [RS(5, 7, 1, 1, 9, 3, steps=rally.MAX_STEPS - 2),                     # a rally in flight: the cap alone
                      RS(5, 11, 1, 1, 9, 3, theirs=4, steps=rally.MAX_STEPS - 2),          # the fifth point on the cap step
                      RS(5, 11, 1, 1, 9, 3, theirs=1, steps=rally.MAX_STEPS - 2, k=2),     # a point on the cap step, not the fifth
                      RS(5, 7, 1, 1, 9, 3, steps=10)], {}),
}


@pytest.mark.parametrize("kind,single_life", [("bricks", False), ("bricks", True), ("rally", False)])
def test_stepping_across_the_cap_writes_the_specs_plane_and_nothing_else_changes(kind, single_life):
    """State records two steps before the cap, written straight into the state buffer; three steps.  The plane equals the
    spec's `truncated` for every step and environment; rewards, masks, states and observations equal what the game's own
    entry writes from the same inputs, with a plane and with a null plane."""
    import torch
    from paac_amd import hip_ops
    spec, states, _ = CAP_STATES[kind]
    option = dict(single_life=single_life) if kind == "bricks" else {}
    step_spec = (lambda e, s, a: spec.step_state_truncated(3, 5 + e, s, a, single_life)) if kind == "bricks" else \
                (lambda e, s, a: spec.step_state_truncated(3, 5 + e, s, a))
    N = len(states)
    history = np.random.RandomState(4).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    runs = {name: game_buffers(kind, states, history) for name in ("old", "plane", "null")}
    plane = torch.full((N,), 7.0, device="cuda")
    cur, seen = list(states), set()
    for step in range(3):
        actions = dev(np.full(N, step % 2, dtype=np.int32))
        for name, b in runs.items():
            args = (3, 5, actions, b["state"][0], b["state"][1], b["stack"][0], b["stack"][1], b["rew"], b["msk"], b["ep_r"],
                    b["ep_l"], b["fin"])
            if name == "old":
                hip_ops.game_step(kind, *args, **option)
            else:
                hip_ops.game_step_records(kind, *args, truncs_out=plane if name == "plane" else None, **option)
            b["state"].reverse()
            b["stack"].reverse()
        torch.cuda.synchronize()
        want = [step_spec(e, s, step % 2) for e, s in enumerate(cur)]
        assert list(plane.cpu().numpy()) == [1.0 if w[3] else 0.0 for w in want], (step, want)
        old = runs["old"]
        assert list(old["msk"].cpu().numpy()) == [0.0 if w[2] else 1.0 for w in want]
        assert [tuple(s)[:len(w[0])] for s, w in zip(old["state"][0].cpu().numpy(), want)] == [w[0] for w in want]
        for name in ("plane", "null"):
            for k in ("rew", "msk", "ep_r", "ep_l"):
                assert torch.equal(runs[name][k], old[k]), (name, k, step)
            assert drained(runs[name]["fin"]) == drained(old["fin"]), (name, step)
            assert torch.equal(runs[name]["state"][0], old["state"][0]) and torch.equal(runs[name]["stack"][0], old["stack"][0])
        seen |= {(w[2], w[3]) for w in want}
        cur = [w[0] for w in want]
    assert seen == {(False, False), (True, False), (True, True)}      # play goes on; a real ending at the cap; the cap alone


def test_catch_writes_zeros():
    import torch
    from paac_amd import catch, hip_ops
    N = 4
    envs = [catch.CatchEnvironment(e, seed=3) for e in range(N)]
    b = game_buffers("catch", [tuple(env.state_words()) for env in envs], np.stack([env.get_initial_state() for env in envs]))
    plane = torch.full((N,), 7.0, device="cuda")
    terminals = 0
    for step in range(14):                      # a whole episode: the 13th step is terminal
        plane.fill_(7.0)
        hip_ops.game_step_records("catch", 3, 0, dev(np.zeros(N, np.int32)), b["state"][0], b["state"][1], b["stack"][0],
                                  b["stack"][1], b["rew"], b["msk"], b["ep_r"], b["ep_l"], b["fin"], truncs_out=plane)
        b["state"].reverse()
        b["stack"].reverse()
        assert list(plane.cpu().numpy()) == [0.0] * N
        over = [env.next(np.eye(3)[0])[2] for env in envs]              # the twins: which steps were terminal
        assert list(b["msk"].cpu().numpy()) == [0.0 if t else 1.0 for t in over]
        terminals += sum(over)
    assert terminals >= N


# -- the loops ---------------------------------------------------------------------------------------------------------------

def make_args(emulator="bricks", **kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", emulator])
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_test_")
    args.emulator_workers = 0
    args.max_global_steps = 1 << 40
    args.arch = "NIPS"
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def build_learner(args, params_seed=0):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(params_seed))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


N_ENVS, T_STEPS, CAP_AT = 4, 5, 2           # the cap falls on step CAP_AT of the first rollout


def twins_near_the_cap(kind="bricks"):
    """The host twins of environments 0..3, their episodes moved to CAP_AT + 1 steps before the cap (what test_bricks_gpu's
    tracking runs reach after 500 steps): with three lives nothing else can end an episode that soon."""
    mod, cls, at = (bricks, bricks.BricksEnvironment, 6) if kind == "bricks" else (rally, rally.RallyEnvironment, 8)
    twins = [cls(e, seed=3) for e in range(N_ENVS)]
    for env in twins:
        env.state = env.state[:at] + (mod.MAX_STEPS - CAP_AT - 1,) + env.state[at + 1:]
    return twins


def rollout_near_the_cap(learner, kind="bricks", **kw):
    from paac_amd.paac import DeviceRollout
    ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, **kw)
    twins = twins_near_the_cap(kind)
    ro.env_state[0].copy_(dev(np.stack([env.state_words() for env in twins])))
    ro.states[0].copy_(dev(np.stack([env.get_initial_state() for env in twins])))
    learner.rollout = ro
    return ro


def cap_row_check(ro):
    """The rollout that contains the cap: the plane has ones exactly at row CAP_AT, and y there is r + gamma V_t."""
    tr, r, V = ro.truncs.cpu().numpy(), ro.rewards.cpu().numpy(), ro.values.cpu().numpy()
    want = np.zeros((T_STEPS, N_ENVS), np.float32)
    want[CAP_AT] = 1.0
    assert np.array_equal(tr, want) and np.array_equal(ro.masks.cpu().numpy()[CAP_AT], np.zeros(N_ENVS))
    y = ro.y.cpu().numpy().reshape(T_STEPS, N_ENVS)
    assert np.array_equal(y[CAP_AT], (r[CAP_AT].astype(np.float64) + np.float64(GAMMA) * V[CAP_AT].astype(np.float64)).astype(np.float32))
    assert np.abs(V[CAP_AT]).min() > 0


def test_device_loop_against_host_loop():
    """Bricks, NIPS, N = 4, T = 5, flag on, the cap inside the first rollout: the device loop and --host_environments true
    agree record for record -- the plane exactly, y / adv / the weights to the bar test_bricks_gpu's host-against-device test
    sets (the two loops reach the same values through different forward launches)."""
    cycles = 2
    feeds = []
    host = build_learner(make_args(emulator_counts=N_ENVS, max_local_steps=T_STEPS, max_global_steps=cycles * N_ENVS * T_STEPS,
                                   sampler="numpy", host_environments=True, record_feeds=True, feed_callback=feeds.append,
                                   bootstrap_truncated=True))
    for env, twin in zip(host.emulators, twins_near_the_cap()):
        env.state = twin.state
    np.random.seed(7)
    host.train()
    assert len(feeds) == cycles and host.host_truncated_steps == 0          # (the last rollout's count)
    devl = build_learner(make_args(emulator_counts=N_ENVS, max_local_steps=T_STEPS, sampler="numpy", bootstrap_truncated=True))
    np.random.seed(7)
    devl.global_step = devl.init_network()
    ro = rollout_near_the_cap(devl, sampler="numpy", use_graph=True)
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        assert np.array_equal(ro.truncs.cpu().numpy(), feeds[c]["truncs"]), "cycle %d" % c
        assert np.array_equal(ro.actions.view(-1).cpu().numpy(), feeds[c]["actions"]), "cycle %d" % c
        assert np.array_equal(ro.rewards.cpu().numpy(), feeds[c]["rewards"]) and np.array_equal(ro.masks.cpu().numpy(), feeds[c]["masks"])
        assert np.array_equal(ro.rollout_states().cpu().numpy(), feeds[c]["states"]), "cycle %d" % c
        assert np.allclose(ro.y.cpu().numpy(), feeds[c]["y"], atol=1e-5) and np.allclose(ro.adv.cpu().numpy(), feeds[c]["adv"], atol=1e-5)
        if c == 0:
            assert devl.truncated_steps() == N_ENVS >= 1 and feeds[0]["truncs"].sum() == N_ENVS
            cap_row_check(ro)
            # the host loop's own records give the same return at the cap, bit for bit
            f = feeds[0]
            want = (f["rewards"][CAP_AT].astype(np.float64) + np.float64(GAMMA) * f["values"][CAP_AT].astype(np.float64))
            assert np.array_equal(f["y"].reshape(T_STEPS, N_ENVS)[CAP_AT], want.astype(np.float32))
        else:
            assert devl.truncated_steps() == 0
    gh, gd = host.network.get_parameters(), devl.network.get_parameters()
    for k in gh:
        assert np.abs(gh[k] - gd[k]).max() < 1e-5, k
    ro.close()


@pytest.mark.parametrize("kind,sampler", [("bricks", "philox"), ("rally", "numpy")])
def test_graph_replay_equals_eager_across_the_cap(kind, sampler):
    outs = []
    for mode in ("eager", "captured", "batched"):
        learner = build_learner(make_args(kind, emulator_counts=N_ENVS, max_local_steps=T_STEPS, sampler=sampler,
                                          bootstrap_truncated=True))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        ro = rollout_near_the_cap(learner, kind, sampler=sampler, use_graph=mode != "eager")
        assert ro.truncs is not None and tuple(ro.truncs.shape) == (T_STEPS, N_ENVS)
        planes = []
        if mode == "batched":
            ro.run_cycles(4)
        else:
            for _ in range(4):
                ro.run_cycle()
                ro.synchronize()
                planes.append((ro.truncs.cpu().numpy().copy(), ro.y.cpu().numpy().copy(), ro.adv.cpu().numpy().copy()))
                if len(planes) == 1:
                    cap_row_check(ro)
        ro.synchronize()
        outs.append(dict(params=learner.network.get_parameters(), planes=planes, truncs=ro.truncs.cpu().numpy().copy(),
                         y=ro.y.cpu().numpy().copy(), masks=ro.masks.cpu().numpy().copy(), states=ro.env_state.cpu().numpy().copy()))
        ro.close()
    assert outs[0]["planes"][0][0].sum() == N_ENVS and outs[0]["planes"][1][0].sum() == 0
    for a, b in zip(outs[0]["planes"], outs[1]["planes"]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for other in outs[1:]:
        for k in ("truncs", "y", "masks", "states"):
            assert np.array_equal(outs[0][k], other[k]), k
        for k, v in outs[0]["params"].items():
            assert np.array_equal(v, other["params"][k]), k


@pytest.mark.parametrize("options", [dict(gae_lambda=0.95, ppo_epochs=2, ppo_minibatches=2), dict(adv_norm=True),
                                     dict(adv_norm=True, gae_lambda=0.95, ppo_epochs=2)])
def test_option_combinations_freeze_the_restated_returns(options):
    """One cycle across the cap under the update options that compute the returns elsewhere than in the backward's first
    launch: the frozen y / adv equal the restatement on the recorded rollout."""
    learner = build_learner(make_args(emulator_counts=N_ENVS, max_local_steps=T_STEPS, sampler="philox", bootstrap_truncated=True,
                                      **options))
    learner.global_step = learner.init_network()
    ro = rollout_near_the_cap(learner, sampler="philox", use_graph=False)
    ro.run_cycle()
    ro.synchronize()
    Bn = N_ENVS * T_STEPS
    if learner.minibatch_on:
        v_boot = learner.v_rec[Bn:Bn + N_ENVS].cpu().numpy()
    else:
        v_boot = learner.ctx.debug_activation(25, Bn + N_ENVS)[Bn:].cpu().numpy()
    host = (v_boot, ro.rewards.cpu().numpy(), ro.masks.cpu().numpy(), ro.values.cpu().numpy(), ro.truncs.cpu().numpy())
    assert host[4].sum() == N_ENVS
    ye, ae = returns_restated(*host, learner.gamma, options.get("gae_lambda"))
    assert np.array_equal(ro.y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(ro.adv.cpu().numpy(), ae.reshape(-1))
    if learner.adv_norm:
        assert ulps(learner.adv_n.cpu().numpy(), adv_norm_restated(ae)[0]).max() <= 1.0
    # ... and not what the same records give without the plane
    y0, _ = returns_restated(*host[:4], np.zeros_like(host[4]), learner.gamma, options.get("gae_lambda"))
    assert not np.array_equal(y0, ye)
    ro.close()


@pytest.mark.parametrize("emulator,flag", [("bricks", False), ("rally", False), ("catch", True), ("synthetic", True)])
def test_no_plane_without_the_flag_or_without_a_step_cap(emulator, flag):
    learner = build_learner(make_args(emulator, emulator_counts=N_ENVS, max_local_steps=T_STEPS, bootstrap_truncated=flag))
    learner.global_step = learner.init_network()
    from paac_amd.paac import DeviceRollout
    ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, use_graph=False)
    learner.rollout = ro
    assert ro.truncs is None and learner.truncated_steps() is None
    assert learner._truncation_applies() is False
    ro.run_cycle()
    ro.synchronize()
    assert learner.truncated_steps() is None and all(t is not None for t in ro._cycle_state())
    ro.close()
