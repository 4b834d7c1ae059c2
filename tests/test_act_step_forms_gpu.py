"""The forms of paac_act_step_mt that name no step outputs.

Context.act_mt -- no environment step at all: policy forward + numpy-parity sampler -- against Context.forward +
hip_ops.sample_mt from the same MT19937 state, bit for bit; and the step form with the optional outputs (`finished`,
`stack_out2`) left out against the same call with both given."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def context(arch, A, N):
    from oracle import network as onet
    from paac_amd import hip_ops
    ctx = hip_ops.Context({"NIPS": 0, "NATURE": 1}[arch], A, max_batch=N)
    host = onet.init_params(arch, A, np.random.RandomState(1), dtype=np.float32)
    flat = np.zeros(ctx.layout["total"], dtype=np.float32)
    for t in ctx.layout["tensors"]:
        flat[t["offset"]:t["offset"] + t["size"]] = host[t["name"]].reshape(-1)
    return ctx, torch.from_numpy(flat).cuda()


def outputs(N, A, mt):
    return dict(act=torch.full((N,), -1, dtype=torch.int32, device="cuda"), probs=torch.zeros((N, A), device="cuda"),
                val=torch.zeros(N, device="cuda"), mt=mt.clone())


# the two sides of the 32-row / 7-action in-register heads path (misc.hip: FusedHeadsHook), and the last shape under the
# 1024-draw bound of the no-step form
@pytest.mark.parametrize("N,A", [(3, 2), (32, 7), (33, 6), (60, 18)])
@pytest.mark.parametrize("arch", ["NIPS", "NATURE"])
def test_act_mt_equals_forward_and_sample_mt(arch, N, A):
    from paac_amd import hip_ops
    ctx, p = context(arch, A, N)
    rs = np.random.RandomState(1000 * N + A)
    states = torch.from_numpy(rs.randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)).cuda()
    mt = hip_ops.mt_state_from_numpy(rs.get_state(), "cuda")
    a, b = outputs(N, A, mt), outputs(N, A, mt)
    scratch = hip_ops.sample_mt_scratch(N, A, "cuda")
    for step in range(2):                  # the second step starts from the stream position the first one left
        ctx.act_mt(p, states, a["mt"], a["act"], a["probs"], a["val"])
        ctx.forward(p, states, probs=b["probs"], values=b["val"])
        hip_ops.sample_mt(b["probs"], b["mt"], scratch, b["act"])
        torch.cuda.synchronize()
        for k in ("act", "probs", "val", "mt"):
            assert torch.equal(a[k], b[k]), "step %d: %s differs" % (step, k)
        assert not torch.equal(a["mt"], mt)
        assert int(a["act"].min()) >= 0 and int(a["act"].max()) < A
    ctx.close()


def test_step_form_without_finished_and_stack_out2_equals_the_call_with_both():
    from paac_amd import hip_ops
    from paac_amd.synthetic import terminal_threshold
    N, A = 32, 4
    ctx, p = context("NATURE", A, N)
    env_seed, off, thr = 5, 3, terminal_threshold(0.15)
    mt = hip_ops.mt_state_from_numpy(np.random.RandomState(77).get_state(), "cuda")

    def fresh():
        d = outputs(N, A, mt)
        d.update(s0=torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda"),
                 s1=torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda"), rew=torch.zeros(N, device="cuda"),
                 msk=torch.zeros(N, device="cuda"), ep_r=torch.zeros(N, device="cuda"),
                 ep_l=torch.zeros(N, dtype=torch.int32, device="cuda"), tick=torch.zeros(1, dtype=torch.int64, device="cuda"))
        hip_ops.synth_reset(env_seed, off, d["s0"], None)
        return d

    a, b = fresh(), fresh()
    fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device="cuda")
    s2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    for step in range(8):                  # terminal probability 0.15: some of the 256 environment steps end an episode
        ctx.act_step_mt(p, a["s0"], a["mt"], a["act"], a["probs"], a["val"], env_seed, off, thr, a["tick"], 0, a["s1"], a["rew"],
                        a["msk"], a["ep_r"], a["ep_l"])
        ctx.act_step_mt(p, b["s0"], b["mt"], b["act"], b["probs"], b["val"], env_seed, off, thr, b["tick"], 0, b["s1"], b["rew"],
                        b["msk"], b["ep_r"], b["ep_l"], fin, stack_out2=s2)
        torch.cuda.synchronize()
        for k in ("act", "probs", "val", "mt", "rew", "msk", "ep_r", "ep_l", "s1"):
            assert torch.equal(a[k], b[k]), "step %d: %s differs" % (step, k)
        assert torch.equal(s2, b["s1"])
        for d in (a, b):
            hip_ops.counter_add(d["tick"], 1)
            d["s0"], d["s1"] = d["s1"], d["s0"]
    assert int(fin[0]) > 0                 # the ring did record episodes in the call that lent one
    ctx.close()
