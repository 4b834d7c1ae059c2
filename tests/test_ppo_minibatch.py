"""--ppo_minibatches: K epochs of M shuffled minibatches (arXiv 1707.06347) on one rollout.  The reference has no PPO, so the
checker is this file's numpy restatement of the contract in include/paac_hip.h: the shuffle is the stable argsort of
philox4x32-10 keys (oracle/sampler.py), the surrogate's gradient is tests/test_ppo.py's restatement on the unmodified oracle
network.  Kernel-level results (permutations, gather, record) are held bit for bit; the gradients to tests/test_ppo.py's bars --
1e-4 of max(|want|.max(), 1e-3 * global norm) per tensor, 1e-4 on the loss scalars."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARCH_ID = {"NIPS": 0, "NATURE": 1}
DOMAIN = 0x504D0000


# -- the restatement ---------------------------------------------------------------------------------------------------

def perm_keys(B, epoch, seed, step):
    from oracle.sampler import philox4x32
    ctr = np.zeros((B, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(B, dtype=np.uint32)
    ctr[:, 1] = np.uint32(step & 0xFFFFFFFF)
    ctr[:, 2] = np.uint32((step >> 32) & 0xFFFFFFFF)
    ctr[:, 3] = np.uint32(DOMAIN + epoch)
    key = np.zeros((B, 2), dtype=np.uint32)
    key[:, 0] = np.uint32(seed & 0xFFFFFFFF)
    key[:, 1] = np.uint32((seed >> 32) & 0xFFFFFFFF)
    return philox4x32(ctr, key)[:, 0]


def perms_restated(B, K, seed, step):
    """int32 [K, B]: row e = the row indices in ascending (key, index) order."""
    return np.stack([np.argsort(perm_keys(B, e, seed, step), kind="stable") for e in range(K)]).astype(np.int32)


# -- CPU ---------------------------------------------------------------------------------------------------------------

def test_cli_flag_default_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    assert p.parse_args([]).ppo_minibatches == 1
    a = p.parse_args(["--ppo_epochs", "4", "--ppo_minibatches", "4"])
    assert a.ppo_minibatches == 4
    assert ("--ppo_minibatches",) in {f[0] for f in train.BUILD_FLAGS}
    logger_utils.save_args(a, str(tmp_path))
    assert logger_utils.load_args(str(tmp_path / "args.json"))["ppo_minibatches"] == 4


@pytest.mark.parametrize("fields,text", [
    (dict(ppo_minibatches=0), "ppo_minibatches"), (dict(ppo_minibatches=-2), "ppo_minibatches"),
    (dict(ppo_minibatches=17), "ppo_minibatches"), (dict(ppo_minibatches=2.5), "ppo_minibatches"),
    (dict(ppo_minibatches=float("nan")), "ppo_minibatches"), (dict(ppo_minibatches=True), "ppo_minibatches"),
    (dict(ppo_minibatches=3, ppo_epochs=2), "does not divide"),                                   # 32 x 5 = 160 rows
    (dict(ppo_minibatches=16, ppo_epochs=5), "optimizer steps"),                                  # 80 > 64
    (dict(ppo_minibatches=2, ppo_epochs=2, emulator_counts=2048, max_local_steps=5), "at most 8192 rows"),
])
def test_actor_learner_refuses_bad_flags(fields, text):
    from paac_amd import _lib, train
    from paac_amd.actor_learner import ActorLearner
    assert (_lib.PPO_MINIBATCHES_MAX, _lib.PPO_STEPS_MAX, _lib.MINIBATCH_MAX_ROWS) == (16, 64, 8192)
    args = train.get_arg_parser().parse_args([])
    for k, v in fields.items():
        setattr(args, k, v)
    args.num_actions = 4
    with pytest.raises(ValueError, match=text):
        ActorLearner(None, None, args)          # refused before anything touches a device


def test_divisibility_and_step_limits_are_read_only_above_one_epoch():
    """Like --ppo_clip, the flag is read only when --ppo_epochs is above 1: M = 3 on 160 rows passes the checks at K = 1 (the
    constructor then fails later, on the missing environment creator)."""
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    args.ppo_minibatches, args.num_actions = 3, 4
    with pytest.raises(AttributeError):
        ActorLearner(None, None, args)


def test_header_declares_the_entries():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, nargs, must in (("paac_minibatch_perms", 7, ("const uint64_t* step_base_dev", "uint64_t step_offset",
                                                            "int32_t* perms_out")),
                              ("paac_gather_minibatch", 15, ("const int32_t* perm", "uint8_t* states_out", "float* v_old_out")),
                              ("paac_record_policy", 8, ("paac_ctx* ctx", "float* p_old_out", "float* v_out"))):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name + " missing from the header"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs
        assert all(t in m.group(1) for t in must) and name in _lib.EXPORTED_SYMBOLS
    for text in (r"#define\s+PAAC_PPO_MINIBATCHES_MAX\s+16", r"#define\s+PAAC_PPO_STEPS_MAX\s+64",
                 r"#define\s+PAAC_MINIBATCH_MAX_ROWS\s+8192", "0x504D0000", r"perm_e\[j\*b : \(j\+1\)\*b\]"):
        assert re.search(text, hdr), text


@pytest.mark.parametrize("B", [1, 5, 40, 1000, 8192])
def test_restatement_returns_permutations(B):
    P = perms_restated(B, 3, 42, 7)
    assert P.shape == (3, B) and P.dtype == np.int32
    for e in range(3):
        assert np.array_equal(np.sort(P[e]), np.arange(B))
    if B >= 40:
        assert not np.array_equal(P[0], P[1]) and not np.array_equal(P[0], np.arange(B))
        assert not np.array_equal(P[0], perms_restated(B, 1, 42, 8)[0])            # the step reaches the keys
        assert not np.array_equal(P[0], perms_restated(B, 1, 43, 7)[0])            # ... and so does the seed


# -- GPU: kernel level -------------------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 5, 40, 160, 1000, 4097, 8192])
def test_permutations_equal_the_restatement(B):
    """(1) bit for bit: sizes around and between powers of two (where a padded bitonic network fails), K = 1 / 3 / 16, two
    seeds, and a step whose base + offset carries into the counter's high word."""
    import torch
    from paac_amd import hip_ops
    base = torch.tensor([2 ** 32 - 1], dtype=torch.int64, device="cuda")
    for K in (1, 3, 16):
        for seed in (42, 0x9E3779B97F4A7C15):
            out = torch.full((K, B), -1, dtype=torch.int32, device="cuda")
            hip_ops.minibatch_perms(B, seed, base, 2, out)
            assert np.array_equal(out.cpu().numpy(), perms_restated(B, K, seed, 2 ** 32 + 1)), (B, K, seed)
    out = torch.full((2, B), -1, dtype=torch.int32, device="cuda")
    hip_ops.minibatch_perms(B, 42, None, 5, out)                                    # no base in memory: base 0
    assert np.array_equal(out.cpu().numpy(), perms_restated(B, 2, 42, 5))


@pytest.mark.gpu
def test_a_replayed_graph_draws_the_next_cycles_permutation():
    import torch
    from paac_amd import hip_ops
    B, K, T = 40, 3, 5
    tick = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = hip_ops.Graph()
        g.begin()
        hip_ops.counter_add(tick, T)
        hip_ops.minibatch_perms(B, 42, tick, 0, out)
        g.end()
        seen = []
        for c in range(3):
            g.launch()
            stream.synchronize()
            seen.append(out.cpu().numpy().copy())
            assert np.array_equal(seen[-1], perms_restated(B, K, 42, (c + 1) * T)), c
        g.close()
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


@pytest.mark.gpu
def test_perms_entry_refuses_bad_sizes():
    import torch
    from paac_amd import _lib
    lib = _lib.load()
    out = torch.zeros(16, dtype=torch.int32, device="cuda")
    for B, K in ((0, 1), (8193, 1), (4, 0), (4, 17)):
        assert lib.paac_minibatch_perms(B, K, 1, None, 0, out.data_ptr(), None) < 0
        assert b"paac_minibatch_perms" in lib.paac_last_error()
    assert lib.paac_minibatch_perms(4, 1, 1, None, 0, None, None) < 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [40, 1000])
def test_gather_equals_index_select(B):
    """(2) states and every small array bit for bit, with some arrays absent, and an output that aliases its input refused."""
    import torch
    from paac_amd import _lib, hip_ops
    rs = np.random.RandomState(B)
    perm = dev(rs.permutation(B).astype(np.int32))
    states = dev(rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8))
    acts = dev(rs.randint(0, 18, B).astype(np.int32))
    y, adv, p_old, v_old = [dev(rs.randn(B).astype(np.float32)) for _ in range(4)]
    idx = perm.long()
    so = torch.zeros_like(states)
    outs = [torch.full_like(t, 7) for t in (acts, y, adv, p_old, v_old)]
    hip_ops.gather_minibatch(perm, states, so, acts, outs[0], y, outs[1], adv, outs[2], p_old, outs[3], v_old, outs[4])
    assert torch.equal(so, states.index_select(0, idx))
    for got, src in zip(outs, (acts, y, adv, p_old, v_old)):
        assert torch.equal(got, src.index_select(0, idx))
    # some arrays absent: what is absent stays untouched, what is given is gathered
    so2, yo, po = torch.zeros_like(states), torch.full_like(y, 7), torch.full_like(p_old, 7)
    hip_ops.gather_minibatch(perm, states, so2, y=y, y_out=yo, p_old=p_old, p_old_out=po)
    assert torch.equal(so2, so) and torch.equal(yo, outs[1]) and torch.equal(po, outs[3])
    ao = torch.full_like(acts, 7)
    hip_ops.gather_minibatch(perm, actions=acts, actions_out=ao)                    # small arrays alone
    assert torch.equal(ao, outs[0])
    # in place / overlapping / half a pair: refused by the wrapper and by the entry itself
    with pytest.raises(ValueError, match="overlaps"):
        hip_ops.gather_minibatch(perm, states, states)
    with pytest.raises(ValueError, match="overlaps"):
        hip_ops.gather_minibatch(perm, y=y, y_out=y)
    with pytest.raises(ValueError, match="both"):
        hip_ops.gather_minibatch(perm, states, so, y=y)
    lib, z = _lib.load(), None
    rc = lib.paac_gather_minibatch(perm.data_ptr(), B, states.data_ptr(), states.data_ptr(), z, z, z, z, z, z, z, z, z, z, None)
    assert rc < 0 and b"overlaps" in lib.paac_last_error()
    rc = lib.paac_gather_minibatch(perm.data_ptr(), B, z, z, z, z, y.data_ptr(), y.data_ptr() + 4 * (B - 1), z, z, z, z, z, z, None)
    assert rc < 0 and b"y_out overlaps y" in lib.paac_last_error()
    rc = lib.paac_gather_minibatch(perm.data_ptr(), B, z, z, z, z, z, z, z, z, z, z, z, z, None)
    assert rc < 0 and b"nothing to gather" in lib.paac_last_error()
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("arch,A,T,N", [("NIPS", 6, 5, 8), ("NATURE", 4, 5, 32)])
def test_record_policy_reads_the_finished_heads_and_leaves_the_backward_alone(arch, A, T, N):
    """(3) after a trunk-only training forward and after kept acting rows + the bootstrap forward: p_old == the training set's
    probability of the action taken, the values == the training set's values (bootstrap rows included), and the backward that
    follows computes the gradient it computes without the record call -- all bit for bit."""
    import torch
    from oracle import network as onet
    from paac_amd import hip_ops
    from test_ppo import upload
    B = T * N
    rs = np.random.RandomState(31 + A)
    params = onet.init_params(arch, A, rs, dtype=np.float32)
    states = dev(rs.randint(0, 256, (B + N, 84, 84, 4)).astype(np.uint8))
    acts, y, adv = dev(rs.randint(0, A, B).astype(np.int32)), dev(rs.randn(B).astype(np.float32)), dev(rs.randn(B).astype(np.float32))
    ctx = hip_ops.Context(ARCH_ID[arch], A, max_batch=B + N)
    p = upload(ctx, params)
    ctx.set_managed_weights(True)
    ctx.pack_weights(p)
    n = ctx.layout["total"]
    probs, values = torch.zeros((N, A), device="cuda"), torch.zeros(N, device="cuda")

    def prepare(route):
        if route == "trunk":
            ctx.train_forward_trunk(p, states)
            return
        for t in range(T):
            ctx.keep_next_forward(t * N)
            ctx.forward(p, states[t * N:(t + 1) * N], probs=probs, values=values)
        ctx.bootstrap_forward_trunk(p, states[B:], B)

    for route in ("trunk", "kept"):
        for phase in (0, 3):
            g0, l0 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            prepare(route)
            ctx.loss_backward(p, states[:B], acts, y, adv, 0.02, g0, l0, forward_done=True, phase=phase)
            g1, l1 = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
            p_old, v = torch.zeros(B, device="cuda"), torch.zeros(B + N, device="cuda")
            prepare(route)
            ctx.record_policy(p, acts, B, p_old, v, B + N)
            torch.cuda.synchronize()
            pi = ctx.debug_activation(26, B).view(B, A)
            what = (arch, route, phase)
            assert torch.equal(p_old, pi[torch.arange(B), acts.long()]) and float(p_old.min()) > 0, what
            assert torch.equal(v, ctx.debug_activation(25, B + N)) and float(v.abs().min()) > 0, what
            ctx.loss_backward(p, states[:B], acts, y, adv, 0.02, g1, l1, forward_done=True, phase=phase)
            torch.cuda.synchronize()
            assert torch.equal(g0, g1) and torch.equal(l0, l1), what
            assert float(g0.abs().max()) > 0
    # p_old alone / values alone, and what the entry refuses
    prepare("trunk")
    p2, v2 = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    ctx.record_policy(p, acts, B, p2, None)
    ctx.record_policy(p, None, B, None, v2)
    torch.cuda.synchronize()
    assert torch.equal(p2, ctx.debug_activation(26, B).view(B, A)[torch.arange(B), acts.long()])
    assert torch.equal(v2, ctx.debug_activation(25, B))
    rc = ctx.lib.paac_record_policy(ctx.handle, p.data_ptr(), acts.data_ptr(), B, None, None, B, None)
    assert rc < 0 and b"nothing to record" in ctx.lib.paac_last_error()
    ctx.train_forward_trunk(p, states[:B])
    if B > 64:                                   # (smaller batches run the whole forward: nothing is pending)
        rc = ctx.lib.paac_record_policy(ctx.handle, p.data_ptr(), acts.data_ptr(), B, p2.data_ptr(), v.data_ptr(), B + N, None)
        assert rc < 0 and b"pending training forward covers" in ctx.lib.paac_last_error()
    torch.cuda.synchronize()
    ctx.close()


# -- GPU: the loops ----------------------------------------------------------------------------------------------------

# The first optimizer step of an M > 1 cycle runs on the weights p_old was recorded on, so nothing is clipped there
# (clip_fraction == 0 exactly).  Its approx_kl is exactly 0 only where the record pass and the step's forward run the same
# kernels: with the acting rows kept (PAAC_REUSE_ACTING, the default) p_old comes out of the acting forwards and the step
# recomputes the trunk, and the two differ by the summation order of their fp32 contractions (include/paac_hip.h).  A
# re-associated fp32 dot product of K terms moves by about sqrt(K) * 2^-24 of its operands' scale -- 3e-6 for the fc layer's
# 3136 terms at initialisation-scale activations of order 1 -- a row's log ratio by at most twice the logits' difference, and
# approx_kl is a mean of those signed differences: the bar is 1e-5.
FIRST_STEP_KL = 1e-5

def compose_cycle(L, s_rows, acts, y, adv, K, M, step, seed, phase):
    """One M > 1 cycle behind its returns, by hand from the public entries: record was run by the caller (p_old / v_old given
    in L), here perms, then per epoch the gather and per minibatch trunk forward + surrogate backward + update.
    -> (perms, stats [K*M, 2 or 3], losses [K*M, 4])"""
    import torch
    from paac_amd import hip_ops
    B = s_rows.shape[0]
    b = B // M
    tick = torch.tensor([step], dtype=torch.int64, device="cuda")
    perms = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    hip_ops.minibatch_perms(B, seed, tick, 0, perms)
    sp = torch.zeros_like(s_rows)
    ap, yp, dp, pp, vp = torch.zeros_like(acts), torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
    st = torch.zeros((K * M, 3 if L.vclip_on else 2), device="cuda")
    lo = torch.zeros((K * M, 4), device="cuda")
    p = L.network.params
    for e in range(K):
        hip_ops.gather_minibatch(perms[e], s_rows, sp, acts, ap, y, yp, adv, dp, L.p_old, pp,
                                 L.v_old if L.vclip_on else None, vp if L.vclip_on else None)
        for j in range(M):
            r, s = slice(j * b, (j + 1) * b), e * M + j
            L.ctx.train_forward_trunk(p, sp[r])
            if L.vclip_on:
                L.ctx.loss_backward_ppo_vclip(p, sp[r], ap[r], yp[r], dp[r], pp[r], vp[r], L.ppo_clip, L.ppo_vclip, L.entropy_beta,
                                              L.grad, lo[s], st[s], forward_done=True, phase=phase)
            else:
                L.ctx.loss_backward_ppo(p, sp[r], ap[r], yp[r], dp[r], pp[r], L.ppo_clip, L.entropy_beta, L.grad, lo[s], st[s],
                                        forward_done=True, phase=phase)
            L.apply_gradients()
    return perms, st, lo


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("loop", ["device", "host"])
def test_cycle_equals_the_hand_composition(monkeypatch, loop, both):
    """(4), (8): K = 2, M = 2 on NIPS, N = 8, T = 5, --adv_norm and --ppo_vclip both off / both on, in the device loop and in the
    host-plugin loop, against the same cycle composed from the public entries on the loop's own rollout records: record,
    returns, perms, gather, then per minibatch trunk forward, paac_loss_backward_ppo[_vclip], update.  y, adv, p_old, the
    permutations, the per-step statistics, weights and optimizer slots bit for bit.  Both loops draw the restated permutation
    of the same step, so on the same records they take the same optimizer steps.  (Device loop on its recomputed-trunk route,
    like tests/test_ppo.py's composition.)"""
    import torch
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    from paac_amd import hip_ops
    from paac_amd.paac import DeviceRollout
    monkeypatch.setenv("PAAC_REUSE_ACTING", "0")
    K, M, N, T, seed = 2, 2, 8, 5, 42
    B = T * N
    flags = dict(ppo_epochs=K, ppo_minibatches=M, ppo_clip=0.1, gae_lambda=0.95)
    if both:
        flags.update(adv_norm=True, ppo_vclip=0.05)
    if loop == "device":
        args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                         max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="philox", test_seed=11, **flags)
        L, _, env_creator = build_learner(args)
        L.global_step = L.init_network()
        ro = DeviceRollout(L, env_creator.device_env_spec, sampler="philox", sampler_seed=seed, use_graph=True)
        ro.run_cycle()
        ro.synchronize()
        before = [t.clone() for _, t in L.update_state]
        ro.run_cycle()                                # parity 1: the cycle that is composed by hand below
        ro.synchronize()
        s_all = ro.states[T:2 * T + 1].view((T + 1) * N, 84, 84, 4)
        s, acts = s_all[:B], ro.actions.view(-1)
        rec = dict(r=ro.rewards, m=ro.masks, V=ro.values, y=ro.y.clone(), adv=ro.adv.clone())
        assert int(ro.global_step_dev.item()) == 2 * B and int(ro.tick.item()) == 2 * T
    else:
        feeds, befores = [], []
        args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                         max_global_steps=2 * B, host_environments=True, record_feeds=True, synthetic_terminal_p=0.1,
                         test_seed=42, sampler_seed=seed, **flags)
        L, _, _ = build_learner(args)
        args.feed_callback = feeds.append
        args.cycle_callback = lambda step: befores.append([t.clone() for _, t in L.update_state])
        np.random.seed(args.test_seed)
        L.train()
        assert len(feeds) == 2
        before, f = befores[0], feeds[1]
        s, acts = dev(f["states"]), dev(f["actions"])
        rec = dict(r=dev(f["rewards"]), m=dev(f["masks"]), V=dev(f["values"]), y=dev(f["y"]).view(-1), adv=dev(f["adv"]).view(-1),
                   v_boot=dev(f["v_boot"]), lr=float(np.float32(f["lr"])))
    assert L.minibatch_on and L.ppo_steps == K * M and tuple(L.ppo_stats.shape) == (K * M, 3 if both else 2)
    after = [t.clone() for _, t in L.update_state]
    want = dict(stats=L.ppo_stats.clone(), losses=L.ppo_loss.clone(), lr=L.lr_dev.clone(), p_old=L.p_old.clone(),
                perms=L.mb["perms"].clone(), v_rec=L.v_rec.clone(), adv_n=L.adv_n.clone() if both else None)
    # -- by hand, from the weights before that cycle and the records it left
    for (_, t), b in zip(L.update_state, before):
        t.copy_(b)
    L.ctx.pack_weights(L.network.params)
    p = L.network.params
    y, adv, adv_n = [torch.zeros(B, device="cuda") for _ in range(3)]
    L.p_old.zero_()
    L.v_rec.zero_()
    if loop == "device":
        gstep = torch.tensor([B], dtype=torch.int64, device="cuda")
        L.lr_dev.zero_()
        L.ctx.train_forward_trunk(p, s_all)
        L.ctx.record_policy(p, acts, B, L.p_old, L.v_rec, B + N)
        v_boot = L.v_rec[B:]
        tick = dict(global_step_dev=gstep, increment=B, initial_lr=L.initial_lr, lr_annealing_steps=L.lr_annealing_steps,
                    lr_out_dev=L.lr_dev)
        if both:
            hip_ops.returns_norm_tick(v_boot, rec["r"], rec["m"], rec["V"], L.gamma, y, adv, adv_n, gae_lambda=0.95, **tick)
        else:
            hip_ops.gae_returns_tick(v_boot, rec["r"], rec["m"], rec["V"], L.gamma, 0.95, y, adv, **tick)
        phase = 3
    else:
        hip_ops.returns(rec["v_boot"], rec["r"], rec["m"], rec["V"], L.gamma, y, adv, 0.95)
        if both:
            hip_ops.adv_normalize(adv, adv_n)
        L.lr_dev.fill_(rec["lr"])
        L.ctx.train_forward_trunk(p, s)
        L.ctx.record_policy(p, acts, B, L.p_old, L.v_rec, B)
        phase = 0
    assert torch.equal(L.p_old, L.ctx.debug_activation(26, B).view(B, -1)[torch.arange(B), acts.long()])
    assert torch.equal(L.v_rec[:B], L.ctx.debug_activation(25, B))
    perms, st, lo = compose_cycle(L, s, acts, y, adv_n if both else adv, K, M, 2 * T, seed, phase)
    torch.cuda.synchronize()
    assert torch.equal(L.lr_dev, want["lr"])
    assert torch.equal(y, rec["y"]) and torch.equal(adv, rec["adv"])              # the recorded arrays are the raw ones
    assert torch.equal(L.p_old, want["p_old"]) and torch.equal(L.v_rec, want["v_rec"])
    if both:
        assert torch.equal(adv_n, want["adv_n"]) and not torch.equal(adv_n, adv)
    assert np.array_equal(perms.cpu().numpy(), perms_restated(B, K, seed, 2 * T)) and torch.equal(perms, want["perms"])
    assert torch.equal(st, want["stats"]) and torch.equal(lo, want["losses"])
    for (name, t), a in zip(L.update_state, after):
        assert torch.equal(t, a), name
    stats = want["stats"].cpu().numpy()
    assert stats[0, 0] == 0 and stats[0, 1] == 0               # recomputed-trunk route: the first step's ratio is identically 1
    assert np.abs(stats[1:, 1]).max() > 0 and np.isfinite(want["losses"].cpu().numpy()).all()
    if loop == "device":
        ro.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,M", [(32, 5, 4), (8, 20, 2)])
@pytest.mark.parametrize("optimizer", ["rmsprop", "adam"])
def test_graph_replay_equals_eager(N, T, M, optimizer):
    """(5) three cycles, weights and optimizer slots bit for bit, on three distinct permutations (each the restatement's for
    the cycle's frame counter); Adam's powers advance K * M times per cycle."""
    from test_gae import run_device_loop
    cycles, K = 3, 2
    seen = []

    def check(learner, ro, c):
        perms = learner.mb["perms"].cpu().numpy().copy()
        assert np.array_equal(perms, perms_restated(N * T, K, ro.sampler_seed, (c + 1) * T)), c
        seen.append((perms, learner.ppo_stats.cpu().numpy().copy(), learner.ppo_loss.cpu().numpy().copy()))
        if optimizer == "adam":
            want = np.float32(learner.beta1)
            for _ in range(K * M * (c + 1)):
                want = np.float32(want * np.float32(learner.beta1))
            assert learner.beta_powers.cpu().numpy()[0] == want

    flags = dict(ppo_epochs=K, ppo_minibatches=M, optimizer=optimizer, gae_lambda=0.95)
    if optimizer == "adam":
        flags.update(e=1e-5, initial_lr=1e-4)
    graph = run_device_loop(N, T, "philox", cycles, use_graph=True, check=check, **flags)
    eager = run_device_loop(N, T, "philox", cycles, use_graph=False, **flags)
    assert all(np.array_equal(a, b) for a, b in zip(graph["state"], eager["state"]))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(graph["y"], eager["y"]))
    assert all(np.isfinite(a).all() for a in graph["state"])
    assert graph["global_step"] == eager["global_step"] == cycles * N * T and graph["lr"] == eager["lr"]
    assert len(seen) == 3 and len({s[0].tobytes() for s in seen}) == 3
    for _, stats, losses in seen:
        assert stats.shape == (K * M, 2) and np.isfinite(stats).all() and np.isfinite(losses).all()
        assert stats[0, 0] == 0 and abs(stats[0, 1]) < FIRST_STEP_KL, stats[0]
        assert (stats[:, 0] >= 0).all() and (stats[:, 0] <= 1).all() and (losses[:, 3] > 0).all()


# (6) parity with the float64 oracle, restarted at every optimizer step from the weights and slots the device holds.  A clip
# decision is discontinuous: a row whose float64 ratio lies within 1e-3 (relative) of 1 +- EPS could legitimately flip in float32.
# The seed below was chosen by running oracle_steps on the CPU: no row comes that close at any of the four steps; the CPU test
# asserts that and excludes nothing.
ORACLE_CASE = dict(arch="NIPS", A=4, N=8, T=5, K=2, M=2, clip=0.2, lr=0.0224, seed=3, perm_seed=42, step=5)


def oracle_case():
    from test_hip_network import make_case
    c = ORACLE_CASE
    B = c["N"] * c["T"]
    params, states, idx, y, adv = make_case(c["arch"], c["A"], B, seed=c["seed"], weight_scale=3.5)
    return params, states, idx, y, adv, perms_restated(B, c["K"], c["perm_seed"], c["step"])


def restated_step(params, states, idx, y, adv, p_old, rows, relu_masks=None):
    """The surrogate's restatement on one minibatch -> (R, L, gradients)."""
    from oracle import network as onet
    from test_ppo import ppo_restated
    c = ORACLE_CASE
    pi = onet.forward(params, states[rows], c["arch"], dtype=np.float64)["pi"]
    R = ppo_restated(pi, idx[rows], adv[rows], p_old[rows], c["clip"], 0.02)
    L, g = onet.loss_and_grads(params, states[rows], np.eye(c["A"])[idx[rows]], y[rows], R["adv_eff"], 0.02, c["arch"],
                               dtype=np.float64, relu_masks=relu_masks)
    return R, L, g


def margin_of(R):
    clip = ORACLE_CASE["clip"]
    return np.minimum(np.abs(R["ratio"] / (1 + clip) - 1), np.abs(R["ratio"] / (1 - clip) - 1)).min()


def oracle_steps():
    """The four steps wholly on the CPU (float64 oracle, clipped RMSProp) -> [(margin, clip_fraction)] per step."""
    from oracle import network as onet
    c = ORACLE_CASE
    params, states, idx, y, adv, perms = oracle_case()
    b = c["N"] * c["T"] // c["M"]
    pi0 = onet.forward(params, states, c["arch"], dtype=np.float64)["pi"]
    p_old = pi0[np.arange(len(idx)), idx]
    ms, mom = onet.rmsprop_init(params)
    out = []
    for e in range(c["K"]):
        for j in range(c["M"]):
            rows = perms[e, j * b:(j + 1) * b]
            R, _, g = restated_step(params, states, idx, y, adv, p_old, rows)
            out.append((margin_of(R), R["clip_fraction"]))
            g, _ = onet.clip_by_global_norm(g, 3.0)
            p1, ms, mom = onet.rmsprop_step({k: v.astype(np.float64) for k, v in params.items()}, g, ms, mom, c["lr"])
            params = {k: v.astype(np.float32) for k, v in p1.items()}
    return out


def test_oracle_seed_keeps_every_row_away_from_the_clip_bounds():
    steps = oracle_steps()
    assert len(steps) == 4
    assert all(m > 1e-3 for m, _ in steps), steps
    assert steps[0][1] == 0.0 and any(0 < f < 1 for _, f in steps), steps


@pytest.mark.gpu
def test_parity_with_the_float64_oracle_at_every_step():
    import torch
    from oracle import network as onet
    from paac_amd import _lib, hip_ops
    from test_ppo import unflatten, upload
    c = ORACLE_CASE
    A, K, M, B = c["A"], c["K"], c["M"], c["N"] * c["T"]
    b = B // M
    params, states, idx, y, adv, want_perms = oracle_case()
    ctx = hip_ops.Context(ARCH_ID[c["arch"]], A, max_batch=B)
    p, s, acts, yd, ad = upload(ctx, params), dev(states), dev(idx), dev(y), dev(adv)
    n = ctx.layout["total"]
    p_old = torch.zeros(B, device="cuda")
    ctx.train_forward_trunk(p, s)
    ctx.record_policy(p, acts, B, p_old, None)
    tick = torch.tensor([c["step"]], dtype=torch.int64, device="cuda")
    perms = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    hip_ops.minibatch_perms(B, c["perm_seed"], tick, 0, perms)
    assert np.array_equal(perms.cpu().numpy(), want_perms)
    pi0 = onet.forward(params, states, c["arch"], dtype=np.float64)["pi"]
    assert np.abs(p_old.cpu().numpy() - pi0[np.arange(B), idx]).max() < 1e-5
    p_old_h = p_old.cpu().numpy()
    sp, ap, yp, dp, pp = torch.zeros_like(s), torch.zeros_like(acts), torch.zeros_like(yd), torch.zeros_like(yd), torch.zeros_like(yd)
    grad, loss, stats = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
    ms, mom, lr = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), torch.tensor([c["lr"]], device="cuda")
    nconv = len(onet.ARCHS[c["arch"]][0])
    fractions = []
    for e in range(K):
        hip_ops.gather_minibatch(perms[e], s, sp, acts, ap, yd, yp, ad, dp, p_old, pp)
        for j in range(M):
            r = slice(j * b, (j + 1) * b)
            rows = want_perms[e, r]
            held = unflatten(ctx, p)                                  # the oracle restarts from the device's weights
            held = {k: v.copy() for k, v in held.items()}
            ctx.train_forward_trunk(p, sp[r])
            ctx.loss_backward_ppo(p, sp[r], ap[r], yp[r], dp[r], pp[r], c["clip"], 0.02, grad, loss, stats, forward_done=True)
            torch.cuda.synchronize()
            masks = {"a%d" % (i + 1): ctx.debug_activation(i + 1, b).cpu().numpy() > 0 for i in range(nconv)}
            masks["h"] = ctx.debug_activation(4, b).cpu().numpy() > 0
            R, L, g_ref = restated_step(held, states, idx, y, adv, p_old_h, rows, relu_masks=masks)
            assert margin_of(R) > 1e-3, (e, j, margin_of(R))
            lo, st = loss.cpu().numpy(), stats.cpu().numpy()
            want_loss = 5.0 * (R["actor"] + L["critic"])
            print("step %d.%d: loss %g / %g actor %g / %g critic %g / %g clip_fraction %g / %g approx_kl %g / %g" %
                  (e + 1, j + 1, lo[0], want_loss, lo[1], R["actor"], lo[2], L["critic"], st[0], R["clip_fraction"], st[1],
                   R["approx_kl"]))
            assert abs(lo[0] - want_loss) < 1e-4 * max(1.0, abs(want_loss))
            assert abs(lo[1] - R["actor"]) < 1e-4 * max(1.0, abs(R["actor"]))
            assert abs(lo[2] - L["critic"]) < 1e-4 * max(1.0, abs(L["critic"])) and abs(lo[3] - L["entropy"].mean()) < 1e-4
            assert st[0] == np.float32(np.float32(np.sum(~R["active"])) / np.float32(b))
            assert abs(st[1] - R["approx_kl"]) < 1e-4 * max(1.0, abs(R["approx_kl"]))
            fractions.append(float(st[0]))
            got, gn = unflatten(ctx, grad), onet.global_norm(g_ref)
            for name, want in g_ref.items():
                err, scale = np.abs(got[name] - want).max(), max(np.abs(want).max(), 1e-3 * gn)
                print("  %s: err / scale %.3g" % (name, err / scale))
                assert err / scale < 1e-4, "step %d.%d %s: max abs err %g (scale %g)" % (e + 1, j + 1, name, err, scale)
            ctx.clip_rmsprop(p, grad, ms, mom, lr, 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)
    assert fractions[0] == 0.0 and any(0 < f < 1 for f in fractions), fractions
    ctx.close()


def _device_run(cycles, drop_field=False, **flags):
    from test_learner_gpu import build_learner
    from test_gae import learner_state, loop_args
    from paac_amd.paac import DeviceRollout
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=8, emulator_workers=0, max_local_steps=5,
                     max_global_steps=1 << 40, synthetic_terminal_p=0.1, sampler="numpy", test_seed=11, **flags)
    if drop_field:
        del args.ppo_minibatches                 # a Namespace from before the flag
    learner, _, env_creator = build_learner(args)
    np.random.seed(args.test_seed)
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, env_creator.device_env_spec, sampler="numpy", use_graph=True)
    for _ in range(cycles):
        ro.run_cycle()
    ro.synchronize()
    out = learner_state(learner) + [learner.ppo_stats.cpu().numpy(), learner.ppo_loss.cpu().numpy()]
    ro.close()
    return out


def _host_run(cycles, drop_field=False, **flags):
    from test_learner_gpu import build_learner
    from test_gae import learner_state, loop_args
    N, T = 8, 5
    args = loop_args(game="pong", arch="NIPS", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=cycles * N * T, host_environments=True, synthetic_terminal_p=0.1, test_seed=42, **flags)
    if drop_field:
        del args.ppo_minibatches
    learner, _, _ = build_learner(args)
    np.random.seed(args.test_seed)
    learner.train()
    return learner_state(learner) + [learner.ppo_stats.cpu().numpy(), learner.ppo_loss.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("run", [_device_run, _host_run])
def test_one_minibatch_is_the_run_without_the_field(run):
    """(7) two cycles at K = 3: --ppo_minibatches 1 and args without the field, bit for bit; M = 3 reaches the update."""
    a = run(2, ppo_epochs=3, ppo_minibatches=1)
    b = run(2, drop_field=True, ppo_epochs=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if run is _host_run:                         # (40 rows; the device run's 40 rows as well, once is enough)
        c = run(2, ppo_epochs=3, ppo_minibatches=2)
        assert not np.array_equal(a[0], c[0]) and all(np.isfinite(x).all() for x in c) and c[-1].shape == (6, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 4])
def test_metrics_carry_one_record_per_optimizer_step(tmp_path, M):
    """(9) K * M ppo_epoch records with minibatch in 1..M; at M = 1 exactly the records from before the flag (no new field)."""
    from test_learner_gpu import build_learner
    from test_gae import loop_args
    N, T, K = 32, 5, 2
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=N, emulator_workers=0, max_local_steps=T,
                     max_global_steps=64 * N * T, synthetic_terminal_p=0.1, sampler="philox", ppo_epochs=K, ppo_minibatches=M,
                     debugging_folder=str(tmp_path))
    L, _, _ = build_learner(args)
    L.train()
    recs = [json.loads(l) for l in open(tmp_path / "metrics.jsonl")]
    steps = [r for r in recs if r.get("kind") == "ppo_epoch"]
    base = {"epoch", "loss", "actor_loss", "critic_loss", "entropy", "clip_fraction", "approx_kl"}
    assert all(base <= set(r) for r in steps)
    if M == 1:
        assert len(steps) == K and [r["epoch"] for r in steps] == [1, 2] and not any("minibatch" in r for r in steps)
        return
    assert len(steps) == K * M
    assert [(r["epoch"], r["minibatch"]) for r in steps] == [(e + 1, j + 1) for e in range(K) for j in range(M)]
    assert steps[0]["clip_fraction"] == 0.0 and abs(steps[0]["approx_kl"]) < FIRST_STEP_KL
    assert all(0.0 <= r["clip_fraction"] <= 1.0 and np.isfinite(r["approx_kl"]) and np.isfinite(r["loss"]) for r in steps)
    progress = [r for r in recs if r.get("kind") == "progress"]
    assert progress and progress[-1]["loss"] == steps[-1]["loss"]
