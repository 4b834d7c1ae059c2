"""The environment step's entries, without a device.

1. What each entry refuses and in which words (raw ctypes; every case is refused before any launch, so no GPU is touched): one
   spoiled argument per case, the message recorded from the build before the step's arguments became one block (SynthStep /
   EnvRecords, csrc/synth_dev.h) and asserted in full.
2. Which entry each of DeviceRollout's seven acting routes reaches, and with which of the rollout's tensors (the ctx and the
   hip_ops step functions are recorders, in the manner of tests/test_update_routing.py)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMES = ("catch", "bricks", "rally")

# ---- 1. refusals ------------------------------------------------------------------------------------------------------------
# An entry's arguments in C order (include/paac_hip.h): (name, valid value).  Pointers are arbitrary distinct non-null integers
# -- nothing dereferences them, every case below is refused first; nullable pointers are valid as 0.
_P = iter(range(0x10000, 0x1000000, 0x10000))


def _args(*names_values):
    return [(n, next(_P) if v is Ellipsis else v) for n, v in names_values]


_RECORDS = [("rewards_out", ...), ("masks_out", ...), ("ep_reward", ...), ("ep_len", ...), ("finished", 0)]
ENTRIES = {
    "paac_synth_reset": _args(("seed", 1), ("env_offset", 0), ("N", 4), ("stack_out", ...), ("raw_scratch", 0), ("stream", 0)),
    "paac_synth_step": _args(("seed", 1), ("env_offset", 0), ("N", 4), ("actions", ...), ("terminal_threshold", 9),
                             ("step_base_dev", 0), ("step_offset", 0), ("stack_in", ...), ("stack_out", ...), ("stack_out2", 0),
                             *_RECORDS, ("raw_scratch", 0), ("stream", 0)),
    "paac_sample_mt_synth_step": _args(("probs", ...), ("A", 4), ("mt_state", ...), ("actions", ...), ("seed", 1), ("env_offset", 0),
                                       ("N", 4), ("terminal_threshold", 9), ("step_base_dev", 0), ("step_offset", 0),
                                       ("stack_in", ...), ("stack_out", ...), ("stack_out2", 0), *_RECORDS, ("walk_scratch", 0),
                                       ("walk_scratch_bytes", 0), ("raw_scratch", 0), ("stream", 0)),
}
for _g in GAMES:
    ENTRIES["paac_%s_reset" % _g] = _args(("seed", 1), ("env_offset", 0), ("N", 4), ("state_out", ...), ("stack_out", ...),
                                          ("stream", 0))
    ENTRIES["paac_%s_step" % _g] = _args(("seed", 1), ("env_offset", 0), ("N", 4), ("actions", ...), ("state_in", ...),
                                         ("state_out", ...), ("state_out2", 0), ("stack_in", ...), ("stack_out", ...),
                                         ("stack_out2", 0), *_RECORDS, *([("single_life", 0)] if _g == "bricks" else []),
                                         ("stream", 0))

# (entry, what is spoiled, {argument: value}) -> the message.  A null in turn for every pointer the entry requires; in-place
# buffers where the entry forbids them (`=`: the first argument is given the second one's value).
_BAD = "%s: bad arguments"
_IN_PLACE = "%s: the step cannot run in place (every band workgroup of an environment reads state_in)"
_NULL = "paac_sample_mt_synth_step: null argument"
EXPECTED = {}
for _e in ("paac_synth_reset", "paac_synth_step") + tuple("paac_%s_%s" % (g, k) for g in GAMES for k in ("reset", "step")):
    EXPECTED[(_e, "N=0")] = _BAD % _e
    for _n, _v in ENTRIES[_e]:
        if _v and _n not in ("seed", "N", "terminal_threshold"):
            EXPECTED[(_e, _n + "=0")] = _BAD % _e
for _g in GAMES:
    for _pair in ("state_out=state_in", "state_out2=state_in", "stack_out=stack_in", "stack_out2=stack_in"):
        EXPECTED[("paac_%s_step" % _g, _pair)] = _IN_PLACE % ("paac_%s_step" % _g)
EXPECTED.update({
    ("paac_sample_mt_synth_step", "N=0"): "paac_sample_mt_synth_step: N=0 A=4",
    ("paac_sample_mt_synth_step", "A=1"): "paac_sample_mt_synth_step: N=4 A=1",
    ("paac_sample_mt_synth_step", "A=33"): "paac_sample_mt_synth_step: N=4 A=33",
    ("paac_sample_mt_synth_step", "N=2305,A=2"): "paac_sample_mt_synth_step: N*(A-1)=2305 exceeds the fused kernel's limit 2304 "
                                                 "(use paac_sample_mt + paac_synth_step)",
})
for _n in ("probs", "mt_state", "actions", "stack_in", "stack_out", "rewards_out", "masks_out", "ep_reward", "ep_len"):
    EXPECTED[("paac_sample_mt_synth_step", _n + "=0")] = _NULL


def refusal(entry, spoil):
    """-> (rc, message) of `entry` called with its valid arguments, `spoil` ('name=value[,name=value]') applied."""
    from paac_amd import _lib
    lib = _lib.load()
    values = dict(ENTRIES[entry])
    for item in spoil.split(","):
        name, value = item.split("=")
        assert name in values, (entry, name)
        values[name] = values[value] if value in values else int(value)
    rc = getattr(lib, entry)(*[values[n] for n, _ in ENTRIES[entry]])
    return rc, (lib.paac_last_error() or b"").decode()


def test_the_cases_cover_every_required_pointer():
    assert len(EXPECTED) == 2 + 8 + 13 + 3 * (3 + 10 + 4)
    for entry, args in ENTRIES.items():
        from paac_amd import _lib
        assert len(args) == len(_lib._SIGNATURES[entry][1]), entry
        assert len({v for _, v in args if v > 0x1000}) == len([v for _, v in args if v > 0x1000])      # distinct pointers


@pytest.mark.parametrize("entry,spoil", sorted(EXPECTED), ids=lambda v: v)
def test_entry_refuses_with_its_message(entry, spoil):
    rc, message = refusal(entry, spoil)
    assert rc < 0
    assert message == EXPECTED[(entry, spoil)]


# ---- 2. the acting step's routes ----------------------------------------------------------------------------------------------
class Recorder(object):
    """Records (name, args, kwargs) of every method called on it, into a list it may share; calls return 0."""

    def __init__(self, calls=None):
        self.calls = [] if calls is None else calls

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
            return 0
        return call


T, N = 2, 4
# route -> (fields the decision reads, the entries one step reaches in order, the entry that steps the environments)
ROUTES = {
    "stateful philox": (dict(stateful=True, sampler="philox"), ["forward_sample", "game_step"], "stateful"),
    "stateful numpy": (dict(stateful=True, sampler="numpy"), ["forward", "sample_mt", "game_step"], "stateful"),
    "act-step small": (dict(sampler="numpy", A=4), ["act_step_mt"], "act_step"),
    "act-step large": (dict(sampler="numpy", A=4, N_decide=128, act_step_large=True), ["act_step_mt"], "act_step"),
    "fused": (dict(sampler="numpy", A=4, N_decide=128), ["forward", "sample_mt_synth_step"], "fused"),
    "numpy separate": (dict(sampler="numpy", A=4, N_decide=1024), ["forward", "sample_mt", "synth_step"], "separate"),
    "philox heads step": (dict(sampler="philox"), ["forward_sample_synth_step"], "heads_step"),
    "philox raw": (dict(sampler="philox", raw=True), ["forward_sample", "synth_step"], "separate"),
}


def rollout(monkeypatch, stateful=False, sampler="numpy", A=4, N_decide=N, act_step_large=False, raw=False):
    import torch
    from paac_amd import hip_ops
    from paac_amd.paac import DeviceRollout
    R = DeviceRollout.__new__(DeviceRollout)
    calls = []
    R.L = type("Learner", (), {})()
    R.L.ctx, R.L.network = Recorder(calls), type("Net", (), {"params": "params"})()
    rec = Recorder(calls)
    for name in ("sample_mt", "synth_step", "sample_mt_synth_step"):
        monkeypatch.setattr(hip_ops, name, getattr(rec, name))
    R.T, R.N, R.A, R.sampler, R.act_step_large, R.reuse_acting = T, N_decide, A, sampler, act_step_large, True
    R.stateful = dict(step=rec.game_step) if stateful else None
    R.raw = "raw" if raw else None
    R.route = R._route()
    R.N = N                                     # (the decision above may have been asked about a larger shard)
    R.states = torch.zeros((2 * T + 1, N, 2), dtype=torch.uint8)
    R.env_state = torch.zeros((2 * T + 1, N, 3), dtype=torch.int32)
    R.actions, R.values = torch.zeros((T, N), dtype=torch.int32), torch.zeros((T, N))
    R.rewards, R.masks = torch.zeros((T, N)), torch.zeros((T, N))
    R.records = [(R.rewards[t], R.masks[t], "ep_reward", "ep_len", "finished") for t in range(T)]
    R.probs, R.tick, R.mt_state, R.mt_scratch, R.walk_scratch = "probs", "tick", "mt_state", "mt_scratch", "walk"
    R.env_spec, R.env_offset, R.sampler_seed, R.env_step_kwargs = dict(seed=7, terminal_threshold=9), 5, 42, dict(single_life=1)
    return R, calls


def same(x, tensor):
    return x.data_ptr() == tensor.data_ptr() and x.shape == tensor.shape


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_acting_route_reaches_its_entries_with_the_rollouts_own_tensors(monkeypatch, route):
    fields, entries, name = ROUTES[route]
    R, calls = rollout(monkeypatch, **fields)
    assert R.route == name
    heads_step = name == "heads_step"
    for t in range(T):
        del calls[:]
        R._act_step(1, t)
        slot, last = T + t, t == T - 1
        assert calls[0] == ("keep_next_forward", (t * N,), {})
        assert [c[0] for c in calls[1:]] == entries
        _, a, k = calls[-1]                                    # the call that steps the environments
        # the step's records: the rollout's own objects, slot t of the per-step ones
        records = [x for x in a if any(x is r for r in R.records[t])]
        assert len(records) == 5 and all(x is r for x, r in zip(records, R.records[t]))
        assert same(records[0], R.rewards[t]) and same(records[1], R.masks[t])
        # observation slot t in, slot t + 1 out; the actions and values of step t
        stacks = [x for x in a if hasattr(x, "data_ptr") and x.dtype == R.states.dtype]
        assert len(stacks) == 2 and same(stacks[0], R.states[slot]) and same(stacks[1], R.states[slot + 1])
        assert sum(same(x, R.actions[t]) for x in a if hasattr(x, "data_ptr")) == 1
        policy = calls[1]                                      # the call that runs the policy: values of step t, by keyword or not
        assert sum(same(x, R.values[t]) for x in policy[1] + tuple(policy[2].values()) if hasattr(x, "data_ptr")) == 1
        # the ring's wrap-around output: on the last step of parity 1 only, slot 0 -- of the observations and, for a game,
        # of the state records; the heads launch has no second output, its route copies (a tensor op, not a recorded call)
        if heads_step:
            assert "stack_out2" not in k
        else:
            assert (k["stack_out2"] is not None) == last and (not last or same(k["stack_out2"], R.states[0]))
        if name == "stateful":
            assert (k["state_out2"] is not None) == last and (not last or same(k["state_out2"], R.env_state[0]))
            states = [x for x in a if hasattr(x, "data_ptr") and x.dtype == R.env_state.dtype and x.dim() == 2]
            assert len(states) == 2 and same(states[0], R.env_state[slot]) and same(states[1], R.env_state[slot + 1])
            assert k["single_life"] == 1
        if name in ("act_step", "fused", "separate"):
            assert k["raw_scratch"] == R.raw
        if name in ("act_step", "fused"):
            assert k["walk_scratch"] == "walk"


def test_heads_step_route_copies_the_wrap_and_parity_0_never_wraps(monkeypatch):
    import torch
    R, calls = rollout(monkeypatch, sampler="philox")
    R.states[2 * T] = 3                                       # what the last step of parity 1 "writes"
    R._act_step(1, 0)
    assert not R.states[0].any()
    R._act_step(1, T - 1)
    assert torch.equal(R.states[0], R.states[2 * T])
    for fields, _, name in ROUTES.values():
        if name == "heads_step":
            continue
        R, calls = rollout(monkeypatch, **fields)
        for t in range(T):
            R._act_step(0, t)
        assert all(c[2].get("stack_out2") is None and c[2].get("state_out2") is None for c in calls)
