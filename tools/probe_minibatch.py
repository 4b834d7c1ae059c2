"""--ppo_minibatches: event-timed durations of the permutation, gather and record launches at B = 160 and B = 2560, and the
cycle time at the headline shape (Nature, 32 environments, t_max 5) for K = 4, M = 4 against K = 4, M = 1 (two alternated runs of
ten 64-cycle windows each).  Run from the repository root on the GPU; prints one JSON object."""
import json, os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
from paac_amd import hip_ops
out = {}
def timed(fn, reps=50, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return dict(median_us=ts[len(ts) // 2], min_us=ts[0], p90_us=ts[int(len(ts) * 0.9)])
for B in (160, 2560):
    K, A = 4, 4
    perms = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    tick = torch.tensor([5], dtype=torch.int64, device="cuda")
    out["perms_B%d_K%d" % (B, K)] = timed(lambda: hip_ops.minibatch_perms(B, 42, tick, 0, perms))
    states = torch.randint(0, 256, (B, 84, 84, 4), dtype=torch.uint8, device="cuda")
    so = torch.zeros_like(states)
    f = [torch.randn(B, device="cuda") for _ in range(8)]
    a, ao = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    out["gather_B%d" % B] = timed(lambda: hip_ops.gather_minibatch(perms[0], states, so, a, ao, f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]))
    ctx = hip_ops.Context(1, A, max_batch=B + 32)
    p = torch.randn(ctx.layout["total"], device="cuda") * 0.01
    ctx.set_managed_weights(True); ctx.pack_weights(p)
    po, vo = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
    ctx.train_forward_trunk(p, states)
    def rec():
        ctx.record_policy(p, a, B, po, vo, B)          # heads already finished: the pick launch alone
    out["record_pick_B%d" % B] = timed(rec)
    def rec_full():
        ctx.train_forward_trunk(p, states); ctx.record_policy(p, a, B, po, vo, B)
    def fwd_only():
        ctx.train_forward_trunk(p, states)
    out["trunk_plus_record_B%d" % B] = timed(rec_full, reps=20, warm=3)
    out["trunk_only_B%d" % B] = timed(fwd_only, reps=20, warm=3)
    ctx.close()
# cycle time at the headline shape: Nature, 32 envs, t_max 5, K = 4, M = 4 against M = 1
from test_learner_gpu import build_learner
from test_gae import loop_args
from paac_amd.paac import DeviceRollout
for M in (1, 4, 1, 4):
    args = loop_args(game="breakout", arch="NATURE", emulator_counts=32, emulator_workers=0, max_local_steps=5, max_global_steps=1 << 40,
                     synthetic_terminal_p=0.1, sampler="numpy", test_seed=11, ppo_epochs=4, ppo_minibatches=M)
    L, _, ec = build_learner(args)
    L.global_step = L.init_network()
    ro = DeviceRollout(L, ec.device_env_spec, sampler="numpy", use_graph=True)
    ro.run_cycles(32); ro.synchronize()
    wins = []
    for w in range(10):
        t0 = time.perf_counter(); ro.run_cycles(64); ro.synchronize(); wins.append((time.perf_counter() - t0) / 64 * 1e6)
    wins.sort()
    out.setdefault("cycle_us_K4_M%d" % M, []).append(dict(median=wins[5], min=wins[0], max=wins[-1]))
    ro.close()
print(json.dumps(out, indent=1))
