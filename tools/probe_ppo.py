"""Time one extra --ppo_epochs epoch beside the epoch-1 update it follows, at the headline shape (T 5, N 32, 4 actions) and
at the Seaquest shard (T 20, N 128, 18 actions): the training forward's trunk over the T*N rollout rows, the heads launch
(heads_train_kernel's clipped-surrogate instantiation against the recording GAE one of epoch 1) and the whole epoch (forward
+ backward + optimizer step) between two events on the stream.  Kernel durations come from the library's timing hooks
(paac_prof_read), whole epochs from hipEvents around eagerly issued calls (launch gaps included, so they are upper bounds
of what a replayed graph pays); median and minimum over the repeats.  Prints one JSON line.

  python tools/probe_ppo.py [--repeats 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops  # noqa: E402

TRUNK = ("conv1_fwd", "conv2_fwd", "conv3_fwd", "conv_tower", "fc_fwd")


def stats(ms):
    us = np.asarray(ms, dtype=np.float64) * 1e3
    return dict(median=float(np.median(us)), min=float(us.min()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    out = dict(repeats=a.repeats, warmup=a.warmup, us={})
    rs = np.random.RandomState(0)
    for T, N, A in ((5, 32, 4), (20, 128, 18)):
        B = T * N
        ctx = hip_ops.Context(_lib.ARCH_NATURE, A, max_batch=B + N)
        n = ctx.layout["total"]
        p = torch.from_numpy((rs.randn(n) * 0.02).astype(np.float32)).cuda()
        ctx.set_managed_weights(True)
        ctx.pack_weights(p)
        s = torch.from_numpy(rs.randint(0, 256, (B + N, 84, 84, 4)).astype(np.uint8)).cuda()
        acts = torch.from_numpy(rs.randint(0, A, B).astype(np.int32)).cuda()
        dev = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()
        values = dev(3.0 * rs.randn(T, N))
        rewards, masks = dev(rs.choice([-1.0, 0.0, 1.0], size=(T, N))), dev(rs.rand(T, N) > 0.1)
        y, adv, p_old = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        grad, loss, st = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda")
        ms, mom = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
        lr = torch.tensor([1e-6], device="cuda")          # the weights barely move over the repeats

        def epoch1():
            ctx.train_forward_trunk(p, s)
            ctx.loss_backward_returns(p, s[:B], acts, None, rewards, masks, values, 0.99, y, adv, 0.02, grad, loss,
                                      forward_done=True, phase=3, gae_lambda=0.95, p_old_out=p_old)
            ctx.clip_rmsprop(p, grad, ms, mom, lr, 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)

        def epoch2():
            ctx.train_forward_trunk(p, s[:B])
            ctx.loss_backward_ppo(p, s[:B], acts, y, adv, p_old, 0.2, 0.02, grad, loss, st, forward_done=True, phase=3)
            ctx.clip_rmsprop(p, grad, ms, mom, lr, 0.99, 0.0, 0.1, 3.0, _lib.CLIP_GLOBAL)

        res = {}
        for name, fn in (("epoch1_update", epoch1), ("extra_epoch", epoch2)):
            epoch1()                                      # y / adv / p_old of the current weights
            # kernel durations
            ctx.prof_enable(True)
            trunk, heads = [], []
            for it in range(a.warmup + a.repeats):
                fn()
                torch.cuda.synchronize()
                recs = ctx.prof_read()
                if it >= a.warmup:
                    trunk.append(sum(ms_ for fam, _, ms_ in recs if fam in TRUNK))
                    heads += [ms_ for fam, _, ms_ in recs if fam == "heads_bwd"]
            ctx.prof_enable(False)
            # the whole epoch between two events
            whole = []
            for it in range(a.warmup + a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    whole.append(e0.elapsed_time(e1))
            assert len(heads) == a.repeats
            res[name] = dict(forward_trunk=stats(trunk), heads_launch=stats(heads), whole=stats(whole))
        out["us"]["T%d_N%d_A%d" % (T, N, A)] = res
        assert np.isfinite(grad.cpu().numpy()).all() and np.isfinite(st.cpu().numpy()).all()
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
