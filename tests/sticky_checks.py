"""What tests/test_sticky_gpu.py's cases share: the sticky step entries against wrapped host twins, bit for bit, and what the
entries refuse.  The user game's case loads the example game's library, and a process holds one kernel library, so it runs in a
child process of its own, as the checks of tests/user_game_checks.py do:
    python tests/sticky_checks.py patrol
prints CHECK_OK as its last line.  Nothing here runs on import."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 3
P = 0.25


def hashed_actions(steps, N, num_actions, salt=0):
    """Actions that depend on nothing but (step, environment): int32 [steps, N]."""
    t, e = np.meshgrid(np.arange(steps, dtype=np.uint64), np.arange(N, dtype=np.uint64), indexing="ij")
    h = (t * np.uint64(2654435761) + e * np.uint64(40503) + np.uint64(salt) * np.uint64(97)) >> np.uint64(7)
    return (h % np.uint64(num_actions)).astype(np.int32)


class StepBuffers(object):
    """What one sticky step launch of N rows reads and writes; states, stacks and the prev plane ping-pong between 0 and 1."""

    def __init__(self, N, words, dev="cuda"):
        import torch
        from paac_amd import hip_ops
        self.N = N
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, words), dtype=torch.int32, device=dev) for _ in range(2)]
        self.prev = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2, self.state2 = torch.zeros_like(self.stacks[0]), torch.zeros_like(self.states[0])
        self.prev2 = torch.full((N,), -7, dtype=torch.int32, device=dev)
        self.actions = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r = (torch.zeros(N, device=dev) for _ in range(3))
        self.truncs = torch.full((N,), 7.0, device=dev)
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)
        self.tick = torch.zeros(1, dtype=torch.int64, device=dev)

    def records(self):
        return (self.rew, self.msk, self.ep_r, self.ep_l, self.fin)

    def flip(self):
        for pair in (self.stacks, self.states, self.prev):
            pair.reverse()

    def outputs(self):
        """Everything the last launch wrote, as host arrays."""
        return dict(states=self.states[1].cpu().numpy(), stacks=self.stacks[1].cpu().numpy(), rewards=self.rew.cpu().numpy(),
                    masks=self.msk.cpu().numpy(), truncs=self.truncs.cpu().numpy(), prev=self.prev[1].cpu().numpy(),
                    ep_reward=self.ep_r.cpu().numpy(), ep_len=self.ep_l.cpu().numpy(), finished=self.fin.cpu().numpy())


def set_step(b, t, actions):
    """Step t of a run: the tick's base in device memory and the rest as the offset (both halves of the sum are exercised)."""
    import torch
    b.tick.fill_(t - t % 7)
    b.actions.copy_(torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32)))
    return t % 7


def game_against_wrapped_twins(kind, make_twin, num_actions, N, env_offset, steps, reset, words, p=P, seed=SEED, **option):
    """paac_game_step_sticky of `kind` against N wrapped twins, bit for bit at every step: state records, stacks, rewards, masks,
    the truncation plane and the prev plane (and its second copy on some steps) -> (steps that stuck, terminal steps)."""
    from paac_amd import hip_ops
    from paac_amd.sticky import StickyEnvironment
    b = StepBuffers(N, words)
    twins = [StickyEnvironment(make_twin(env_offset + e), p, seed, env_offset + e) for e in range(N)]
    want_obs = np.stack([env.get_initial_state() for env in twins])
    reset(seed, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.stacks[0].cpu().numpy(), want_obs)
    chosen = hashed_actions(steps, N, num_actions)
    one_hot = np.eye(num_actions)
    stuck = terminals = 0
    for t in range(steps):
        second = t % 5 == 4
        offset = set_step(b, t, chosen[t])
        hip_ops.game_step_sticky(kind, p, b.tick, offset, b.prev[0], b.prev[1], seed, env_offset, b.actions, b.states[0],
                                 b.states[1], b.stacks[0], b.stacks[1], *b.records(), stack_out2=b.stack2 if second else None,
                                 state_out2=b.state2 if second else None, truncs_out=b.truncs,
                                 prev_out2=b.prev2 if second else None, **option)
        obs, rewards, overs, truncs = [], [], [], []
        for e, env in enumerate(twins):
            o, r, over = env.next(one_hot[chosen[t, e]])
            stuck += env.last_executed != chosen[t, e]
            truncs.append(bool(over) and bool(getattr(env, "last_step_truncated", False)))
            if over:
                o = env.get_initial_state()
            obs.append(o)
            rewards.append(r)
            overs.append(over)
        terminals += sum(overs)
        got = b.outputs()
        assert np.array_equal(got["states"], np.stack([env.state_words() for env in twins])), "step %d: states" % t
        assert np.array_equal(got["stacks"], np.stack(obs)), "step %d: stacks" % t
        assert np.array_equal(got["rewards"], np.asarray(rewards, dtype=np.float32)), "step %d: rewards" % t
        assert np.array_equal(got["masks"], 1.0 - np.asarray(overs, dtype=np.float32)), "step %d: masks" % t
        assert np.array_equal(got["truncs"], np.asarray(truncs, dtype=np.float32)), "step %d: truncation plane" % t
        assert np.array_equal(got["prev"], np.asarray([env.prev for env in twins], dtype=np.int32)), "step %d: prev" % t
        if second:
            import torch
            assert torch.equal(b.prev2, b.prev[1]) and torch.equal(b.state2, b.states[1]) and torch.equal(b.stack2, b.stacks[1])
        b.flip()
    return int(stuck), int(terminals)


# ---- refusals: raw ctypes on arbitrary non-null pointers -- every case is refused before any launch, nothing is dereferenced ----
def _pointers():
    return iter(range(0x10000, 0x4000000, 0x10000))


def refusal_cases():
    """-> [(entry, what is spoiled, the arguments in C order, words the message must hold)] for the three sticky entries."""
    from paac_amd import _lib
    cases = []

    def block(ptr, **kw):
        fields = dict(p=0.25, step_base_dev=0, step_offset=0, prev_in=next(ptr), prev_out=next(ptr), prev_out2=0)
        fields.update({k: (fields[v] if isinstance(v, str) else v) for k, v in kw.items()})
        return _lib.Sticky(fields["p"], fields["step_base_dev"], fields["step_offset"], fields["prev_in"], fields["prev_out"],
                           fields["prev_out2"])

    def step_args(entry, sticky, **kw):
        ptr = _pointers()
        v = dict(game=_lib.EVAL_BRICKS, seed=1, env_offset=0, N=4, actions=next(ptr), state_in=next(ptr), state_out=next(ptr),
                 state_out2=0, stack_in=next(ptr), stack_out=next(ptr), stack_out2=0)
        rec = _lib.EnvRecords(next(ptr), next(ptr), next(ptr), next(ptr), 0, 0)
        v.update({k: (v[x] if isinstance(x, str) else x) for k, x in kw.items()})
        records = kw.get("rec", ctypes.byref(rec))
        head = [v["seed"], v["env_offset"], v["N"], v["actions"], v["state_in"], v["state_out"], v["state_out2"], v["stack_in"],
                v["stack_out"], v["stack_out2"], records]
        keep = (rec, sticky)                                   # (alive until the call)
        st = None if sticky is None else ctypes.byref(sticky)
        if entry == "paac_game_step_sticky":
            return [v["game"]] + head + [0, st, 0], keep
        return head + [st, 0], keep

    sticky_spoils = [
        ("p=-0.1", dict(p=-0.1), "outside [0, 1)"), ("p=1", dict(p=1.0), "outside [0, 1)"), ("p=1.5", dict(p=1.5), "outside [0, 1)"),
        ("p=nan", dict(p=float("nan")), "outside [0, 1)"), ("prev_in=0", dict(prev_in=0), "null prev_in / prev_out"),
        ("prev_out=0", dict(prev_out=0), "null prev_in / prev_out"), ("prev_out=prev_in", dict(prev_out="prev_in"), "in place"),
        ("prev_out2=prev_in", dict(prev_out2="prev_in"), "in place"),
    ]
    for entry in ("paac_game_step_sticky", "paac_duel_step_sticky"):
        for name, spoil, words in sticky_spoils:
            cases.append((entry, name, step_args(entry, block(_pointers(), **spoil)), words))
        cases.append((entry, "sticky=NULL", step_args(entry, None), "null sticky block"))
        cases.append((entry, "rec=NULL", step_args(entry, block(_pointers()), rec=None), "null records"))
        cases.append((entry, "actions=0", step_args(entry, block(_pointers()), actions=0), "bad arguments"))
        cases.append((entry, "state_out=state_in", step_args(entry, block(_pointers()), state_out="state_in"), "in place"))
        cases.append((entry, "stack_out2=stack_in", step_args(entry, block(_pointers()), stack_out2="stack_in"), "in place"))
    cases.append(("paac_game_step_sticky", "N=0", step_args("paac_game_step_sticky", block(_pointers()), N=0), "bad arguments"))
    cases.append(("paac_game_step_sticky", "game=7", step_args("paac_game_step_sticky", block(_pointers()), game=7), "game 7 is none of"))
    cases.append(("paac_duel_step_sticky", "N=3", step_args("paac_duel_step_sticky", block(_pointers()), N=3), "not an even number"))

    def eval_args(**kw):
        ptr = _pointers()
        v = dict(game=_lib.EVAL_RALLY, probs=next(ptr), N=4, A=6, greedy=0, eval_seed=5, noops=3, step_base_dev=0, step_offset=0,
                 env_seed=1, env_offset=0, state_in=next(ptr), state_out=next(ptr), stack_in=next(ptr), stack_out=next(ptr),
                 actions_out=next(ptr), score=next(ptr), length=next(ptr), done=next(ptr), alive=next(ptr), p=0.25,
                 prev_in=next(ptr), prev_out=next(ptr), stream=0)
        order = list(v)
        v.update({k: (v[x] if isinstance(x, str) else x) for k, x in kw.items()})
        return [v[k] for k in order], ()

    for name, spoil, words in sticky_spoils[:7]:
        cases.append(("paac_eval_step_sticky", name, eval_args(**spoil), words))
    for name, spoil, words in (("N=0", dict(N=0), "N=0"), ("A=1", dict(A=1), "outside [2, 32]"), ("A=33", dict(A=33), "outside [2, 32]"),
                               ("noops=-1", dict(noops=-1), "negative"), ("probs=0", dict(probs=0), "bad arguments"),
                               ("alive=0", dict(alive=0), "bad arguments"), ("state_out=state_in", dict(state_out="state_in"), "in place"),
                               ("stack_out=stack_in", dict(stack_out="stack_in"), "in place"), ("game=9", dict(game=9), "game 9 is none of")):
        cases.append(("paac_eval_step_sticky", name, eval_args(**spoil), words))
    return cases


def check_refusals(user_library=False):
    """Every case comes back below zero with the entry's name and the reason in the message.  The stock library also refuses
    the user game's id by name; a library with a user game serves it."""
    from paac_amd import _lib
    lib = _lib.load()
    cases = refusal_cases()
    for entry, name, (args, keep), words in cases:
        rc = getattr(lib, entry)(*args)
        message = (lib.paac_last_error() or b"").decode()
        assert rc == -1 and message.startswith(entry + ":") and words in message, (entry, name, rc, message)
    if not user_library:
        for entry, slot in (("paac_game_step_sticky", 0), ("paac_eval_step_sticky", 0)):
            args = [c for c in cases if c[0] == entry][0][2][0]
            good = list(args)
            good[slot] = _lib.EVAL_USER
            if entry == "paac_game_step_sticky":
                sticky = _lib.Sticky(0.25, 0, 0, 0x5550000, 0x5560000, 0)
                good[-2] = ctypes.byref(sticky)
            else:
                good[-4] = 0.25
            rc = getattr(lib, entry)(*good)
            message = (lib.paac_last_error() or b"").decode()
            assert rc == -1 and message.startswith(entry + ": game %d is none of" % _lib.EVAL_USER), (entry, rc, message)
    return len(cases)


# ---- the user game: in a process of its own ------------------------------------------------------------------------------------
def check_patrol():
    """examples/patrol through --device_game: N = 3, env_offset 5, 60 steps of the sticky step against the wrapped twin, and
    what a library with a user game refuses."""
    import user_game_checks as checks
    module, hip_ops = checks.load_game()
    words = hip_ops.USER_GAMES["user"]["words"]
    stuck, terminals = game_against_wrapped_twins("user", lambda g: module.Environment(g, seed=SEED), module.NUM_ACTIONS, 3, 5, 60,
                                                  hip_ops.user_game_reset, words)
    print("patrol: %d of 180 steps executed the previous action, %d terminal steps" % (stuck, terminals))
    assert stuck >= 20
    check_refusals(user_library=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    {"patrol": check_patrol}[sys.argv[1]](*sys.argv[2:])
    print("CHECK_OK")
