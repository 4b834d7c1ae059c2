"""Time the two advantage estimators where they run: the update's first launch (heads_train_kernel, which finishes the heads
forward, runs the row's returns scan and the heads gradient) and the standalone returns kernel, n-step against GAE(0.95),
at the headline shape (T 5, N 32) and at the Seaquest shard (T 20, N 128, 18 actions).  Kernel durations come from the
library's own timing hooks (the dispatch's begin / end timestamps: paac_prof_read), median and minimum over the repeats.
Prints one JSON line.

  python tools/probe_gae.py [--repeats 200] [--warmup 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops  # noqa: E402


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
        v_boot, values = dev(3.0 * rs.randn(N)), dev(3.0 * rs.randn(T, N))
        rewards, masks = dev(rs.choice([-1.0, 0.0, 1.0], size=(T, N))), dev(rs.rand(T, N) > 0.1)
        y, adv = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")
        grad, loss = torch.zeros(n, device="cuda"), torch.zeros(4, device="cuda")
        ctx.prof_enable(True)
        for name, lam in (("nstep", None), ("gae", 0.95)):
            first, alone = [], []
            for it in range(a.warmup + a.repeats):
                ctx.train_forward_trunk(p, s)
                ctx.loss_backward_returns(p, s[:B], acts, None, rewards, masks, values, 0.99, y, adv, 0.02, grad, loss,
                                          forward_done=True, phase=3, gae_lambda=lam)
                hip_ops.returns(v_boot, rewards, masks, values, 0.99, y, adv, lam)
                torch.cuda.synchronize()
                recs = ctx.prof_read()
                if it >= a.warmup:
                    first += [ms for fam, batch, ms in recs if fam == "heads_bwd"]
                    alone += [ms for fam, batch, ms in recs if fam == "nstep_returns"]
            assert len(first) == len(alone) == a.repeats
            key = "T%d_N%d_A%d" % (T, N, A)
            out["us"].setdefault(key, {})[name] = dict(update_first_launch=stats(first), returns_kernel=stats(alone))
        ctx.prof_enable(False)
        assert np.isfinite(grad.cpu().numpy()).all()
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
