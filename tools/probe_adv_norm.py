"""What --adv_norm and --ppo_vclip cost, at the headline shape (T 5, N 32, 4 actions) and at the Seaquest shard (T 20, N 128,
18 actions): the replayed device cycle with --adv_norm true against off (the flag un-fuses the returns from the backward's
first launch and adds the bootstrap rows' heads finish: about two launches), the returns + normalisation launch on its own,
and one value-clipped epoch (paac_loss_backward_ppo_vclip) beside one plain surrogate epoch (paac_loss_backward_ppo), issued
eagerly between two events like tools/probe_ppo.py's.  The two settings of a pair alternate window by window; median and
minimum over the windows.  Prints one JSON line.

  python tools/probe_adv_norm.py [--windows 9] [--cycles 200] [--repeats 200]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops, train  # noqa: E402
from paac_amd.paac import DeviceRollout, PAACLearner  # noqa: E402


def stats(us):
    us = np.asarray(us, dtype=np.float64)
    return dict(median=float(np.median(us)), min=float(us.min()))


def timed(fn, count):
    """us per call of fn(count) between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(count)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


def rollout(T, N, game, adv_norm):
    args = train.get_arg_parser().parse_args(["--adv_norm", "true" if adv_norm else "false", "--gae_lambda", "0.95"])
    args.game, args.arch = game, "NATURE"
    args.emulator_counts, args.max_local_steps, args.emulator_workers = N, T, 0
    args.max_global_steps = 1 << 40
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_probe_")
    nc, ec = train.get_network_and_environment_creator(args)
    L = PAACLearner(nc, ec, args)
    L.global_step = L.init_network()
    return L, DeviceRollout(L, ec.device_env_spec, sampler="numpy", use_graph=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--cycles", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=200)
    a = ap.parse_args()
    out = dict(windows=a.windows, cycles=a.cycles, repeats=a.repeats, us={})
    rs = np.random.RandomState(0)
    for T, N, A, game in ((5, 32, 4, "breakout"), (20, 128, 18, "seaquest")):
        res, B = {}, T * N
        # -- the replayed cycle, flag off / on, alternating windows
        pair = {on: rollout(T, N, game, on) for on in (False, True)}
        assert pair[True][0].num_actions == A
        cyc = {False: [], True: []}
        for w in range(a.windows + 1):
            for on in (False, True):
                ro = pair[on][1]
                with torch.cuda.stream(ro.stream):
                    us = timed(lambda c: (ro.run_cycles(c), ro.synchronize()), a.cycles)
                if w:                                     # (window 0: capture and warm-up)
                    cyc[on].append(us)
        res["cycle_off"], res["cycle_adv_norm"] = stats(cyc[False]), stats(cyc[True])
        for on in (False, True):
            pair[on][1].close()
        del pair
        # -- the returns + normalisation launch on its own
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.float32)).cuda()
        values, v_boot = dev(3.0 * rs.randn(T, N)), dev(3.0 * rs.randn(N))
        rewards, masks = dev(rs.choice([-1.0, 0.0, 1.0], size=(T, N))), dev(rs.rand(T, N) > 0.1)
        y, adv, adv_n = [torch.zeros(B, device="cuda") for _ in range(3)]
        for lam, name in ((None, "returns_norm_nstep"), (0.95, "returns_norm_gae")):
            one = lambda c: [hip_ops.returns_norm_tick(v_boot, rewards, masks, values, 0.99, y, adv, adv_n, gae_lambda=lam)
                             for _ in range(c)]
            one(20)
            # back-to-back launches: the per-launch figure includes the launch gap, so it bounds the kernel from above
            res[name + "_back_to_back"] = stats([timed(one, a.repeats) for _ in range(a.windows)])
        # -- one value-clipped epoch beside one plain surrogate epoch
        ctx = hip_ops.Context(_lib.ARCH_NATURE, A, max_batch=B + N)
        n = ctx.layout["total"]
        p = torch.from_numpy((rs.randn(n) * 0.02).astype(np.float32)).cuda()
        ctx.set_managed_weights(True)
        ctx.pack_weights(p)
        s = torch.from_numpy(rs.randint(0, 256, (B, 84, 84, 4)).astype(np.uint8)).cuda()
        acts = torch.from_numpy(rs.randint(0, A, B).astype(np.int32)).cuda()
        p_old, v_old = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        grad, loss, st = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda")
        ms, mom, lr = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"), torch.tensor([1e-6], device="cuda")
        hip_ops.returns_norm_tick(v_boot, rewards, masks, values, 0.99, y, adv, adv_n, gae_lambda=0.95)
        ctx.loss_backward_record(p, s, acts, y, adv_n, p_old, 0.02, grad, loss)
        ctx.train_values_into(v_old, B)

        def epoch(vclip):
            ctx.train_forward_trunk(p, s)
            if vclip:
                ctx.loss_backward_ppo_vclip(p, s, acts, y, adv_n, p_old, v_old, 0.2, 0.2, 0.02, grad, loss, st, forward_done=True,
                                            phase=3)
            else:
                ctx.loss_backward_ppo(p, s, acts, y, adv_n, p_old, 0.2, 0.02, grad, loss, st, forward_done=True, phase=3)
            ctx.clip_rmsprop(p, grad, ms, mom, lr, 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)

        ep = {False: [], True: []}
        for w in range(a.windows + 1):
            for vclip in (False, True):
                us = timed(lambda c: [epoch(vclip) for _ in range(c)], a.repeats)
                if w:
                    ep[vclip].append(us)
        res["epoch_ppo"], res["epoch_ppo_vclip"] = stats(ep[False]), stats(ep[True])
        assert np.isfinite(grad.cpu().numpy()).all() and np.isfinite(st.cpu().numpy()).all()
        ctx.close()
        out["us"]["T%d_N%d_A%d" % (T, N, A)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
