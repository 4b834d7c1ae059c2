"""Which entry each route of the update reaches (no device: the ctx / the library is a recorder).  The optimizer step by
(optimizer, gated or not), the clipped-surrogate backward by --ppo_vclip from both of its callers, the plain backward by
p_old_out."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Recorder(object):
    """Records (name, args, kwargs) of every method called on it; calls return 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return call


def learner(optimizer, **fields):
    import torch
    from paac_amd.actor_learner import ActorLearner
    L = ActorLearner.__new__(ActorLearner)
    L.ctx, L.optimizer = Recorder(), optimizer
    L.network = type("Net", (), {"params": "params"})()
    L.grad_store = torch.arange(9, dtype=torch.float32)
    L.grad = L.grad_store[:8]
    L.ppo_stats = torch.arange(12, dtype=torch.float32).view(4, 3)
    L.ppo_loss = torch.zeros(4, 4)
    L.ppo_applied, L.ppo_kl_checked = torch.zeros(4, dtype=torch.int32), torch.zeros(4)
    for k in ("adam_m", "adam_v", "beta_powers", "lr_dev", "beta1", "beta2", "rms", "mom", "alpha", "momentum", "e", "clip_norm",
              "clip_mode", "gnorm_dev", "kl_stop", "p_old", "v_old", "ppo_clip", "ppo_vclip", "entropy_beta"):
        setattr(L, k, k)
    L.kl_thr, L.target_kl_on, L.first_gated_step, L.ppo_steps, L.kl_in_store, L.vclip_on = 0.03, True, 1, 4, False, False
    for k, v in fields.items():
        setattr(L, k, v)
    return L


RULE = {"adam": ("adam_m", "adam_v", "beta_powers", "lr_dev", "beta1", "beta2"), "rmsprop": ("rms", "mom", "lr_dev", "alpha", "momentum")}


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
@pytest.mark.parametrize("kl_in_store", [False, True])
def test_apply_gradients_reaches_the_entry_of_its_optimizer_and_gate(optimizer, kl_in_store):
    import torch
    L = learner(optimizer, kl_in_store=kl_in_store)
    for step in (None, 0, 1, 3, 4):
        L.apply_gradients(step)
    calls = L.ctx.calls
    stem = "clip_" + optimizer
    assert [c[0] for c in calls] == [stem, stem, stem + "_gated", stem + "_gated", stem]
    scale = L._grad_scale()
    for (name, a, k), step in zip(calls, (None, 0, 1, 3, 4)):
        assert a[0] == "params" and a[1] is L.grad
        assert a[2:] == RULE[optimizer] + ("e", "clip_norm", "clip_mode", scale, "gnorm_dev")
        if not name.endswith("_gated"):
            assert k == {}
            continue
        assert sorted(k) == ["applied", "checked", "first", "kl", "kl_scale", "stop", "thr"]
        want_kl = L.grad_store[8:] if kl_in_store else L.ppo_stats[step, 1:2]
        assert torch.equal(k["kl"], want_kl) and k["kl"].data_ptr() == want_kl.data_ptr()
        assert k["kl_scale"] == (scale if kl_in_store else 1.0) and k["thr"] == 0.03 and k["stop"] == "kl_stop"
        assert k["first"] is (step == 1)
        assert k["applied"].data_ptr() == L.ppo_applied[step:step + 1].data_ptr() and k["applied"].numel() == 1
        assert k["checked"].data_ptr() == L.ppo_kl_checked[step:step + 1].data_ptr() and k["checked"].numel() == 1


@pytest.mark.parametrize("vclip_on", [False, True])
def test_surrogate_backward_reaches_the_vclip_entry_exactly_under_the_flag(vclip_on):
    import torch
    L = learner("rmsprop", vclip_on=vclip_on, target_kl_on=False, ppo_minibatches=2)
    rows = 8
    L.mb = dict(perms=torch.zeros((2, rows), dtype=torch.int32), states=torch.zeros((rows, 1), dtype=torch.uint8),
                actions=torch.zeros(rows, dtype=torch.int32), y=torch.zeros(rows), adv=torch.zeros(rows), p_old=torch.zeros(rows),
                v_old=torch.zeros(rows) if vclip_on else None)
    L.ppo_epoch_backward(2, "states", "actions", "y", "adv", 3)
    L.minibatch_step_backward(1, "states", "actions", "y", "adv", 0)
    entry = "loss_backward_ppo_vclip" if vclip_on else "loss_backward_ppo"
    assert [c[0] for c in L.ctx.calls] == ["train_forward_trunk", entry, "train_forward_trunk", entry]
    _, a, k = L.ctx.calls[1]
    head, clips = ("params", "states", "actions", "y", "adv", "p_old"), ("ppo_clip",)
    if vclip_on:
        head, clips = head + ("v_old",), ("ppo_clip", "ppo_vclip")
    assert a[:len(head) + len(clips) + 1] == head + clips + ("entropy_beta",) and a[len(head) + len(clips) + 1] is L.grad
    assert a[-2].data_ptr() == L.ppo_loss[2].data_ptr() and a[-1].data_ptr() == L.ppo_stats[2].data_ptr()
    assert k == dict(forward_done=True, phase=3)
    _, a, k = L.ctx.calls[3]                     # step 1 = epoch 0, minibatch 1: rows [4, 8) of the staging block
    staged = [L.mb[n][4:8] for n in ("states", "actions", "y", "adv", "p_old") + (("v_old",) if vclip_on else ())]
    assert a[0] == "params" and all(x.data_ptr() == w.data_ptr() and x.shape == w.shape for x, w in zip(a[1:], staged))
    assert a[1 + len(staged):1 + len(staged) + len(clips)] == clips
    assert a[-2].data_ptr() == L.ppo_loss[1].data_ptr() and a[-1].data_ptr() == L.ppo_stats[1].data_ptr()
    assert k == dict(forward_done=True, phase=0)


def test_loss_backward_with_p_old_out_reaches_the_record_entry(monkeypatch):
    import torch
    from paac_amd import hip_ops
    monkeypatch.setattr(hip_ops, "_ptr", lambda t, dtype, numel, name, optional=False: (name, t))
    monkeypatch.setattr(hip_ops, "_stream", lambda: "stream")
    ctx = hip_ops.Context.__new__(hip_ops.Context)
    ctx.lib, ctx.handle, ctx.max_batch, ctx.layout = Recorder(), "handle", 8, {"total": 10}
    states = torch.zeros((8, 84, 84, 4), dtype=torch.uint8)
    ctx.loss_backward("p", states, "a", "y", "adv", 0.02, "g", "l", forward_done=True, phase=3)
    ctx.loss_backward("p", states, "a", "y", "adv", 0.02, "g", "l", forward_done=True, phase=3, p_old_out="po")
    ctx.loss_backward_record("p", states, "a", "y", "adv", "po", 0.02, "g")
    plain, rec, alias = ctx.lib.calls
    head = ("handle", ("params", "p"), ("states", states), ("actions", "a"), ("y", "y"), ("adv", "adv"))
    assert plain == ("paac_loss_backward", head + (8, 0.02, ("grad", "g"), ("loss_out", "l"), 1, 3, "stream"), {})
    assert rec == ("paac_loss_backward_record",
                   head + (("p_old_out", "po"), 8, 0.02, ("grad", "g"), ("loss_out", "l"), 1, 3, "stream"), {})
    assert alias == ("paac_loss_backward_record",
                     head + (("p_old_out", "po"), 8, 0.02, ("grad", "g"), ("loss_out", None), 0, 0, "stream"), {})
    with pytest.raises(ValueError, match="outside"):          # _check_states
        ctx.loss_backward("p", torch.zeros((9, 84, 84, 4), dtype=torch.uint8), "a", "y", "adv", 0.02, "g")
