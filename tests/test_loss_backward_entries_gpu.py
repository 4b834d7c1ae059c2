"""The six paac_loss_backward* entries as one table: what each refuses, and which heads instantiation each (loss, estimator)
cell reaches on both heads routes.  Every comparison is bit for bit: the cells share their arithmetic by construction
(csrc/heads.h), so any difference is a dispatch error -- a wrong argument block, a wrong instantiation, a dropped array."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ARCH_ID = {"NIPS": 0, "NATURE": 1}
ENTRIES = ("paac_loss_backward", "paac_loss_backward_returns", "paac_loss_backward_returns_record", "paac_loss_backward_record",
           "paac_loss_backward_ppo", "paac_loss_backward_ppo_vclip")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rollout_records(T, N, seed):
    rs = np.random.RandomState(seed)
    return (dev(rs.randn(N).astype(np.float32)), dev(rs.choice([-1.0, 0.0, 1.0], size=(T, N)).astype(np.float32)),
            dev((rs.rand(T, N) > 0.2).astype(np.float32)), dev(rs.randn(T, N).astype(np.float32)))


# ---- refusals -------------------------------------------------------------------------------------------------------
class Refusals:
    """One valid call per entry through raw ctypes (NIPS, A = 4, max_batch = 8) and the means to spoil one argument of it."""

    def __init__(self):
        import torch
        from paac_amd import hip_ops
        self.ctx = hip_ops.Context(ARCH_ID["NIPS"], 4, max_batch=8)
        n = self.ctx.layout["total"]
        self.p, self.g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        self.s = torch.zeros((9, 84, 84, 4), dtype=torch.uint8, device="cuda")
        self.a, self.z = torch.zeros(9, dtype=torch.int32, device="cuda"), torch.zeros(9, device="cuda")

    def returns(self, batch, **spoil):
        from paac_amd import hip_ops
        N = batch if 0 < batch <= 9 else 8       # T * N = batch wherever a batch can have records: one defect at a time
        z = self.z[:N].view(1, N)
        ret = hip_ops._returns_struct(self.z[:N], z, z, z, 0.99, self.z[:N], self.z[:N], None, 0, 0.0, 1, None, None, 0, None)
        for k, v in spoil.items():
            setattr(ret, k, v)
        return ret

    def call(self, entry, params=True, batch=8, phase=0, **spoil):
        """-> (rc, message) of `entry` with valid arguments except the ones named."""
        lib, z = self.ctx.lib, self.z.data_ptr()
        head = (self.ctx.handle, self.p.data_ptr() if params else None, self.s.data_ptr(), self.a.data_ptr())
        tail = (batch, 0.02, self.g.data_ptr(), None)
        end = (0, phase, None)
        ret = self.returns(batch, **spoil)
        if entry == "paac_loss_backward":
            rc = lib.paac_loss_backward(*head, z, z, *tail, *end)
        elif entry == "paac_loss_backward_returns":
            rc = lib.paac_loss_backward_returns(*head, ctypes.byref(ret), *tail, *end)
        elif entry == "paac_loss_backward_returns_record":
            rc = lib.paac_loss_backward_returns_record(*head, ctypes.byref(ret), z, *tail, *end)
        elif entry == "paac_loss_backward_record":
            rc = lib.paac_loss_backward_record(*head, z, z, z, *tail, *end)
        elif entry == "paac_loss_backward_ppo":
            rc = lib.paac_loss_backward_ppo(*head, z, z, z, 0.2, *tail, None, *end)
        elif entry == "paac_loss_backward_ppo_vclip":
            rc = lib.paac_loss_backward_ppo_vclip(*head, z, z, z, z, 0.2, 0.2, *tail, None, *end)
        else:       # paac_returns_norm_tick: the other caller of the returns checks
            rc = lib.paac_returns_norm_tick(self.ctx.handle, self.p.data_ptr(), ctypes.byref(ret), z, None, None)
        return rc, lib.paac_last_error().decode()


@pytest.fixture(scope="module")
def refusals():
    r = Refusals()
    yield r
    r.ctx.close()


SHARED_DEFECTS = [(dict(params=False), "null argument"), (dict(batch=0), "batch 0 outside (0, max_batch=8]"),
                  (dict(batch=9), "batch 9 outside (0, max_batch=8]"), (dict(phase=-1), "phase -1"), (dict(phase=4), "phase 4")]
# paac_loss_backward_returns_record reported its refusals under paac_loss_backward_returns' name before the entries shared
# one body: the one case of this file that differs from the parent of that change
NAME_FIXED = {"paac_loss_backward_returns_record"}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("defect,wording", SHARED_DEFECTS, ids=[w.split(" outside")[0] for _, w in SHARED_DEFECTS])
def test_each_entry_refuses_each_shared_defect_under_its_own_name(refusals, entry, defect, wording):
    rc, msg = refusals.call(entry, **defect)
    print(entry, defect, "->", rc, msg)
    assert rc < 0 and wording in msg
    assert msg.startswith(entry + ":"), "the one known difference from the parent" if entry in NAME_FIXED else msg


RETURNS_DEFECTS = [(dict(estimator=2), "estimator 2"), (dict(gae_lambda=1.5), "gae_lambda 1.5 outside [0, 1]"),
                   (dict(rewards=None), "null rollout record")]


@pytest.mark.parametrize("entry", ["paac_loss_backward_returns", "paac_loss_backward_returns_record", "paac_returns_norm_tick"])
@pytest.mark.parametrize("defect,wording", RETURNS_DEFECTS, ids=[w.split(" ")[0] for _, w in RETURNS_DEFECTS])
def test_both_callers_of_the_returns_checks_refuse_each_defect(refusals, entry, defect, wording):
    rc, msg = refusals.call(entry, **defect)
    print(entry, defect, "->", rc, msg)
    assert rc < 0 and wording in msg
    assert msg.startswith(entry + ":"), "the one known difference from the parent" if entry in NAME_FIXED else msg


def test_the_valid_call_of_the_table_is_accepted(refusals):
    """The table's calls are wrong in the one way named: unspoiled, every entry runs."""
    import torch
    for entry in ENTRIES + ("paac_returns_norm_tick",):
        rc, msg = refusals.call(entry)
        assert rc == 0, (entry, msg)
    torch.cuda.synchronize()


# ---- dispatch ---------------------------------------------------------------------------------------------------------
T, N = 2, 4
B = T * N          # one workgroup per row, every reduction workgroup present: nothing in the dispatch depends on more rows
CLIP, EPSV, BETA, GAMMA, LAM = 0.2, 0.1, 0.02, 0.99, 0.95


def run_cells(ctx, p, s, acts, recs, route, phase):
    """Every (loss, estimator) cell once on `route` ("trunk": heads_train_kernel inside the backward's first launch; "whole":
    the separate heads_bwd_kernel) -> {cell: dict(grad, loss, y, adv, p_old, stats)}."""
    import torch
    v_boot, rewards, masks, values = recs
    n = ctx.layout["total"]
    out = {}

    def cell(name, backward, nstats=0):
        r = dict(grad=torch.zeros(n, device="cuda"), loss=torch.zeros(4, device="cuda"), y=torch.zeros(B, device="cuda"),
                 adv=torch.zeros(B, device="cuda"), p_old=torch.zeros(B, device="cuda"),
                 stats=torch.full((max(nstats, 1),), 7.0, device="cuda"))
        (ctx.train_forward_trunk if route == "trunk" else ctx.train_forward)(p, s)
        backward(r)
        out[name] = r

    def returns(lam, record):
        return lambda r: ctx.loss_backward_returns(p, s, acts, v_boot, rewards, masks, values, GAMMA, r["y"], r["adv"], BETA,
                                                   r["grad"], r["loss"], forward_done=True, phase=phase, gae_lambda=lam,
                                                   p_old_out=r["p_old"] if record else None)
    cell("a3c/nstep", returns(None, False))
    cell("a3c/gae", returns(LAM, False))
    cell("record/nstep", returns(None, True))
    cell("record/gae", returns(LAM, True))
    y, adv, p_old = out["a3c/nstep"]["y"], out["a3c/nstep"]["adv"], out["record/nstep"]["p_old"]
    cell("a3c/arrays", lambda r: ctx.loss_backward(p, s, acts, y, adv, BETA, r["grad"], r["loss"], forward_done=True, phase=phase))
    cell("record/arrays", lambda r: ctx.loss_backward_record(p, s, acts, y, adv, r["p_old"], BETA, r["grad"], r["loss"],
                                                             forward_done=True, phase=phase))
    cell("ppo", lambda r: ctx.loss_backward_ppo(p, s, acts, y, adv, p_old, CLIP, BETA, r["grad"], r["loss"], r["stats"],
                                                forward_done=True, phase=phase), nstats=2)
    v_own = torch.zeros(B, device="cuda")
    ctx.train_values_into(v_own, B)
    cell("vclip", lambda r: ctx.loss_backward_ppo_vclip(p, s, acts, y, adv, p_old, v_own, CLIP, EPSV, BETA, r["grad"], r["loss"],
                                                        r["stats"], forward_done=True, phase=phase), nstats=3)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("A", [4, 6, 18])
def test_every_cell_reaches_its_instantiation_on_both_heads_routes(A):
    import torch
    from paac_amd import hip_ops
    from test_hip_network import make_case
    from test_ppo import upload
    params, states, idx, _, _ = make_case("NATURE", A, B, seed=A)
    ctx = hip_ops.Context(ARCH_ID["NATURE"], A, max_batch=B)
    p, s, acts = upload(ctx, params), dev(states), dev(idx)
    recs = rollout_records(T, N, seed=100 + A)
    eq = torch.equal
    for phase in (0, 3):
        runs = {route: run_cells(ctx, p, s, acts, recs, route, phase) for route in ("trunk", "whole")}
        for route, c in runs.items():
            where = (A, phase, route)
            assert float(c["a3c/nstep"]["grad"].abs().max()) > 0 and not eq(c["a3c/nstep"]["adv"], c["a3c/gae"]["adv"]), where
            # the plain gradient and loss against the recording one, per estimator; the arrays entries against the in-launch returns
            for est in ("nstep", "gae", "arrays"):
                plain, rec = c["a3c/" + est], c["record/" + est]
                assert eq(plain["grad"], rec["grad"]) and eq(plain["loss"], rec["loss"]), where + (est,)
                assert eq(plain["y"], rec["y"]) and eq(plain["adv"], rec["adv"]), where + (est,)
                assert eq(rec["p_old"], c["record/nstep"]["p_old"]) and float(rec["p_old"].min()) > 0, where + (est,)
            assert eq(c["a3c/arrays"]["grad"], c["a3c/nstep"]["grad"]) and eq(c["a3c/arrays"]["loss"], c["a3c/nstep"]["loss"]), where
            # the surrogate fed the recorded p_old: the plain gradient, nothing clipped, no divergence
            assert eq(c["ppo"]["grad"], c["a3c/nstep"]["grad"]) and c["ppo"]["stats"].tolist() == [0.0, 0.0], where
            # the value clip around the training values themselves: the surrogate, nothing clipped
            assert eq(c["vclip"]["grad"], c["ppo"]["grad"]) and eq(c["vclip"]["loss"], c["ppo"]["loss"]), where
            assert c["vclip"]["stats"].tolist() == [0.0, 0.0, 0.0], where
        for name, tr in runs["trunk"].items():
            wh = runs["whole"][name]
            for key in ("grad", "loss", "y", "adv", "p_old", "stats"):
                assert eq(tr[key], wh[key]), (A, phase, name, key)
    ctx.close()
