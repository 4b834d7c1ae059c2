"""Time the optimizer step's two rules on the Nature layout: clip_rmsprop against clip_adam, device events around a
steady-state window of back-to-back steps replayed from one hipGraph (after a warm-up replay), per clip mode.  Prints one
JSON line.

  python tools/probe_adam.py [--steps 200] [--warmup 400] [--repeats 5] [--actions 4]

Under `rocprofv3 --kernel-trace --stats` the per-kernel times of norm_kernel / rmsprop_kernel and adam_norm_kernel /
adam_kernel come out of the same run."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from paac_amd import _lib, hip_ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--actions", type=int, default=4)
    a = ap.parse_args()
    ctx = hip_ops.Context(_lib.ARCH_NATURE, a.actions, max_batch=8)
    ctx.set_managed_weights(True)           # the learner's setting: the step also rewrites the packed copies
    n = ctx.layout["total"]
    rs = np.random.RandomState(0)
    params = torch.from_numpy(rs.randn(n).astype(np.float32) * 0.01).cuda()
    grad = torch.from_numpy(rs.randn(n).astype(np.float32) * 1e-3).cuda()
    s1, s2 = torch.ones(n, device="cuda"), torch.zeros(n, device="cuda")
    powers = torch.tensor([0.9, 0.999], dtype=torch.float32, device="cuda")
    lr, gn = torch.tensor([1e-6], device="cuda"), torch.zeros(1, device="cuda")
    rules = {
        "rmsprop": lambda mode: ctx.clip_rmsprop(params, grad, s1, s2, lr, 0.99, 0.0, 0.1, 3.0, mode, 1.0, gn),
        "adam": lambda mode: ctx.clip_adam(params, grad, s1, s2, powers, lr, 0.9, 0.999, 0.1, 3.0, mode, 1.0, gn),
    }
    stream = torch.cuda.Stream()
    out = dict(layout_floats=n, steps=a.steps, warmup=a.warmup, repeats=a.repeats, us_per_update={})
    with torch.cuda.stream(stream):
        for mode_name, mode in (("global", _lib.CLIP_GLOBAL), ("local", _lib.CLIP_LOCAL)):
            for rule, step in rules.items():
                s1.fill_(1.0 if rule == "rmsprop" else 0.0)     # RMSProp's ms starts at 1, Adam's m and v at 0
                s2.zero_()
                # `steps` steps captured into one hipGraph: the window times the GPU, not the host's launch rate
                graph = hip_ops.Graph()
                graph.begin()
                for _ in range(a.steps):
                    step(mode)
                graph.end()
                for _ in range(max(1, a.warmup // a.steps)):
                    graph.launch()
                best = []
                for _ in range(a.repeats):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    graph.launch()
                    t1.record(stream)
                    t1.synchronize()
                    best.append(t0.elapsed_time(t1) * 1e3 / a.steps)
                graph.close()
                out["us_per_update"]["%s_%s" % (rule, mode_name)] = dict(median=float(np.median(best)), min=float(min(best)))
    stream.synchronize()
    assert np.isfinite(params.cpu().numpy()).all()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
