"""What tests/test_user_game.py and tests/test_user_game_gpu.py share, and the GPU checks of the latter: a process holds one
kernel library, so every check that loads the example game's library (examples/patrol) runs in a child process of its own,
    python tests/user_game_checks.py <check> [arguments]
and prints CHECK_OK as its last line.  Nothing here runs on import."""
import functools
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATROL = os.path.join(ROOT, "examples", "patrol", "patrol.py")
SEED = 3
ACTION_SEED = 1                                            # of the RandomState the kernel-against-twin runs draw actions from
SHAPES = [(1, 1000, 300), (5, 7, 300), (64, 0, 60)]        # (N, env_offset, steps) of the kernel-against-twin runs
TRACE_KINDS = ("kill", "hit", "escape", "entry", "shot_off", "death")


@functools.lru_cache(maxsize=None)
def patrol():
    """The example's specification module, loaded by path (the twin needs no library)."""
    spec = importlib.util.spec_from_file_location("patrol_spec_for_tests", PATROL)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@functools.lru_cache(maxsize=None)
def random_run(N, env_offset, steps, seed=SEED, action_seed=ACTION_SEED):
    """The uniform random actions of a kernel-against-twin run and what they lead the twins through ->
    (int32 [steps, N], {kind: count}).  States only: no rendering."""
    p = patrol()
    actions = np.random.RandomState(action_seed).randint(0, p.NUM_ACTIONS, (steps, N)).astype(np.int32)
    states = [p.start_state(seed, env_offset + e, 0) for e in range(N)]
    seen = dict.fromkeys(TRACE_KINDS, 0)
    for t in range(steps):
        for e in range(N):
            lives = states[e][3]
            states[e], _, term, trunc, events = p.step_events(seed, env_offset + e, states[e], int(actions[t, e]))
            seen["kill"] += bool(events & {"kill_flight", "kill_move"})
            seen["hit"] += bool(events & {"hit_walk", "hit_move"})
            for kind in ("escape", "entry", "shot_off"):
                seen[kind] += kind in events
            seen["death"] += bool(term and not trunc and lives == 1)
    return actions, seen


def S(px, py, face=1, lives=3, shot=(0, 0, 0), steps=10, x=(-9, -9, -9, -9), d=(1, 1, 1, 1), k=0):
    return (px, py, face, lives) + tuple(shot) + (steps,) + tuple(x) + tuple(d) + (k,)


def reentry_steps(env, i, k=0):
    """The first steps value from 10 on at which drone i of (environment env, episode k), parked on that step, waits 1."""
    from paac_amd.synthetic import synth_key
    p = patrol()
    h = synth_key(SEED, env, k)
    return next(t for t in range(10, 990) if p.park(h, 0x9A7E1000 + 16 * t + i)[0] == -1)


# Hand-made records, one per event kind: (name, state, action, single_life) -> what the step must show is in EXPECT below.
# Record e is stepped as environment e (the parking hashes hang on it); only "reentry" depends on them.
def crafted():
    cases = [
        ("kill_flight", S(3, 5, x=(-9, 5, -9, -9), d=(1, -1, 1, 1)), 1, False),
        ("kill_move", S(3, 5, x=(-9, 6, -9, -9), d=(1, -1, 1, 1)), 1, False),
        ("hit_walk", S(3, 5, x=(-9, 4, -9, -9)), 3, False),
        ("hit_move", S(3, 5, x=(-9, 4, -9, -9), d=(1, -1, 1, 1)), 0, False),
        ("escape", S(0, 0, x=(13, -9, 0, -9), d=(1, 1, -1, 1)), 0, False),
        ("entry", S(0, 0, x=(-1, -1, -9, -9), d=(1, -1, 1, 1)), 0, False),
        ("reentry", None, 1, False),
        ("shot_off", S(12, 0), 1, False),
        ("fire_ignored", S(8, 7, shot=(2, 0, 1)), 1, False),
        ("kill_and_hit", S(3, 5, shot=(4, 2, 1), x=(6, 4, -9, -9), d=(-1, -1, 1, 1)), 0, False),
        ("death", S(3, 5, lives=1, x=(-9, 4, -9, -9), d=(1, -1, 1, 1), k=2), 0, False),
        ("single_life", S(3, 5, x=(-9, 4, -9, -9), d=(1, -1, 1, 1)), 0, True),
        ("hit_with_lives", S(3, 5, x=(-9, 4, -9, -9), d=(1, -1, 1, 1)), 0, False),
        ("cap", S(3, 4, steps=999, k=1), 0, False),
        ("cap_and_death", S(3, 5, lives=1, steps=999, x=(-9, 4, -9, -9), d=(1, -1, 1, 1)), 0, False),
        ("cap_and_hit", S(3, 5, lives=3, steps=999, x=(-9, 4, -9, -9), d=(1, -1, 1, 1)), 0, False),
        ("one_short_of_cap", S(3, 4, steps=998), 0, False),
        ("diagonal_fire", S(5, 5, face=-1), 14, False),
    ]
    e = [name for name, _, _, _ in cases].index("reentry")
    cases[e] = ("reentry", S(3, 5, steps=reentry_steps(e, 1), x=(-9, 5, -9, -9), d=(1, -1, 1, 1)), 1, False)
    return cases


# name -> (reward, terminal, truncated, events that must be among the step's)
EXPECT = {
    "kill_flight": (1.0, False, False, {"kill_flight"}), "kill_move": (1.0, False, False, {"kill_move"}),
    "hit_walk": (-1.0, False, False, {"hit_walk"}), "hit_move": (-1.0, False, False, {"hit_move"}),
    "escape": (0.0, False, False, {"escape"}), "entry": (0.0, False, False, {"entry"}),
    "reentry": (1.0, False, False, {"kill_flight", "entry"}), "shot_off": (0.0, False, False, {"shot_off"}),
    "fire_ignored": (0.0, False, False, set()), "kill_and_hit": (0.0, False, False, {"kill_flight", "hit_move"}),
    "death": (-1.0, True, False, {"hit_move"}), "single_life": (-1.0, True, False, {"hit_move"}),
    "hit_with_lives": (-1.0, False, False, {"hit_move"}), "cap": (0.0, True, True, set()),
    "cap_and_death": (-1.0, True, False, {"hit_move"}), "cap_and_hit": (-1.0, True, True, {"hit_move"}),
    "one_short_of_cap": (0.0, False, False, set()), "diagonal_fire": (0.0, False, False, set()),
}


def drained(fin):
    """The device ring of finished episodes -> (count, sorted [(reward, length)])."""
    host = fin.cpu().numpy()
    count = int(host[0])
    assert count <= 4096
    return count, sorted(zip(host[2:2 + 4096].view(np.float32)[:count].tolist(), host[2 + 4096:2 + 4096 + count].tolist()))


def step_twins(twins, actions):
    """runners.step_emulators for a list of twins -> (observations, rewards, masks, truncations)."""
    one_hot = np.eye(twins[0].num_actions)
    obs, rewards, overs, truncs = [], [], [], []
    for env, a in zip(twins, actions):
        o, r, t = env.next(one_hot[int(a)])
        truncs.append(env.last_step_truncated)
        if t:
            o = env.get_initial_state()
        obs.append(o)
        rewards.append(r)
        overs.append(t)
    return (np.stack(obs), np.asarray(rewards, dtype=np.float32), 1.0 - np.asarray(overs, dtype=np.float32),
            np.asarray(truncs, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the checks: each runs in a process of its own

def load_game():
    """--emulator user --device_game examples/patrol/patrol.py, as the creator does it -> (the module, hip_ops)."""
    from paac_amd import hip_ops, user_game
    return user_game.load(PATROL), hip_ops


class Buffers(object):
    """What one paac_user_game_step launch of N environments reads and writes."""

    def __init__(self, N, words, dev="cuda"):
        import torch
        from paac_amd import hip_ops
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, words), dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.state2 = torch.zeros((N, words), dtype=torch.int32, device=dev)
        self.actions = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r, self.trunc = (torch.zeros(N, device=dev) for _ in range(4))
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)

    def step(self, seed, env_offset, a, second=False, **option):
        import torch
        from paac_amd import hip_ops
        self.actions.copy_(torch.from_numpy(np.asarray(a, dtype=np.int32)))
        self.trunc.fill_(7.0)
        hip_ops.user_game_step_records(seed, env_offset, self.actions, self.states[0], self.states[1], self.stacks[0],
                                       self.stacks[1], self.rew, self.msk, self.ep_r, self.ep_l, self.fin,
                                       stack_out2=self.stack2 if second else None, state_out2=self.state2 if second else None,
                                       truncs_out=self.trunc, **option)


def check_kernel(N, env_offset, steps):
    """Kernel against twin, bit for bit: records, stacks, rewards, masks, the truncation plane, episode totals, the ring."""
    import torch
    module, hip_ops = load_game()
    N, env_offset, steps = int(N), int(env_offset), int(steps)
    assert hip_ops.USER_GAMES["user"] == dict(words=20, eval_id=3, step_option="single_life")
    b = Buffers(N, module.STATE_WORDS)
    twins = [module.Environment(env_offset + e, seed=SEED) for e in range(N)]
    want_obs = np.stack([env.get_initial_state() for env in twins])
    hip_ops.user_game_reset(SEED, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.stacks[0].cpu().numpy(), want_obs)
    assert np.array_equal(b.states[0].cpu().numpy(), np.stack([env.state_words() for env in twins]))
    want_ep_r, want_ep_l, want_fin = np.zeros(N, np.float32), np.zeros(N, np.int32), []
    script, seen = random_run(N, env_offset, steps)
    for step in range(steps):
        second = step == 7
        b.step(SEED, env_offset, script[step], second=second)
        want_obs, want_rew, want_msk, want_trunc = step_twins(twins, script[step])
        want_ep_r += want_rew
        want_ep_l += 1
        for e in np.nonzero(want_msk == 0.0)[0]:
            want_fin.append((float(want_ep_r[e]), int(want_ep_l[e])))
            want_ep_r[e], want_ep_l[e] = 0.0, 0
        assert np.array_equal(b.states[1].cpu().numpy(), np.stack([env.state_words() for env in twins])), "step %d: states" % step
        assert np.array_equal(b.stacks[1].cpu().numpy(), want_obs), "step %d: stacks" % step
        assert np.array_equal(b.rew.cpu().numpy(), want_rew) and np.array_equal(b.msk.cpu().numpy(), want_msk), "step %d" % step
        assert np.array_equal(b.trunc.cpu().numpy(), want_trunc), "step %d: truncs" % step
        assert np.array_equal(b.ep_r.cpu().numpy(), want_ep_r) and np.array_equal(b.ep_l.cpu().numpy(), want_ep_l), "step %d" % step
        assert drained(b.fin) == (len(want_fin), sorted(want_fin)), "step %d: finished ring" % step
        if second:
            assert torch.equal(b.stack2, b.stacks[1]) and torch.equal(b.state2, b.states[1])
        b.stacks.reverse()
        b.states.reverse()
    print("N = %d, %d steps: %s; episodes %s" % (N, steps, seen, want_fin))


def check_crafted():
    """One launch over the hand-made records per option value: the rarer branches, against the twin."""
    import torch
    module, hip_ops = load_game()
    cases = crafted()
    N = len(cases)
    b = Buffers(N, module.STATE_WORDS)
    records = np.stack([module.state_words(s) for _, s, _, _ in cases])
    history = np.random.RandomState(4).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    for single_life in (False, True):
        b.states[0].copy_(torch.from_numpy(records))
        b.stacks[0].copy_(torch.from_numpy(history))
        b.ep_r.fill_(2.0)
        b.ep_l.fill_(40)
        b.fin.zero_()
        b.step(SEED, 0, [a for _, _, a, _ in cases], single_life=single_life)
        got_states, got_stacks = b.states[1].cpu().numpy(), b.stacks[1].cpu().numpy()
        got = (b.rew.cpu().numpy(), b.msk.cpu().numpy(), b.trunc.cpu().numpy())
        want_fin = []
        for e, (name, s, a, _) in enumerate(cases):
            state, r, t, tr = module.step_state_truncated(SEED, e, s, a, single_life)
            assert np.array_equal(got_states[e], module.state_words(state)), (name, single_life)
            assert (got[0][e], got[1][e], got[2][e]) == (r, 0.0 if t else 1.0, 1.0 if tr else 0.0), (name, single_life)
            want = np.zeros((84, 84, 4), dtype=np.uint8)
            if not t:
                want[..., :3] = history[e][..., 1:]
            want[..., 3] = module.plane(state)
            assert np.array_equal(got_stacks[e], want), (name, single_life)
            if t:
                want_fin.append((2.0 + r, 41))
        assert drained(b.fin) == (len(want_fin), sorted(want_fin))
    print("crafted: %d records" % N)


def check_refusals():
    import ctypes
    import torch
    from paac_amd import _lib
    module, hip_ops = load_game()
    N, W = 2, module.STATE_WORDS
    stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    stack_b = torch.zeros_like(stack)
    state = torch.zeros((N, W), dtype=torch.int32, device="cuda")
    state_b = torch.zeros_like(state)
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    f, i = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    hip_ops.user_game_reset(1, 0, state, stack)

    def refused(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except _lib.PaacHipError as exc:
            return str(exc)
        raise AssertionError("not refused")

    step = hip_ops.user_game_step
    assert "in place" in refused(step, 1, 0, actions, state, state, stack, stack_b, f, f.clone(), f.clone(), i)
    assert "in place" in refused(step, 1, 0, actions, state, state_b, stack, stack, f, f.clone(), f.clone(), i)
    assert "in place" in refused(step, 1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, state_out2=state)
    assert "in place" in refused(step, 1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, stack_out2=stack)
    for bad in ("state_b[:, :8].contiguous()", "state_b[:1]"):
        try:
            step(1, 0, actions, state, eval(bad), stack, stack_b, f, f.clone(), f.clone(), i)
            raise AssertionError("not refused")
        except ValueError:
            pass
    # null arguments and N = 0: past the wrapper, at the library
    lib = _lib.load()
    rec = _lib.EnvRecords(f.data_ptr(), f.data_ptr(), f.data_ptr(), i.data_ptr(), None, None)
    ptrs = [actions.data_ptr(), state.data_ptr(), state_b.data_ptr(), None, stack.data_ptr(), stack_b.data_ptr(), None]
    assert lib.paac_user_game_step(1, 0, N, *ptrs, None, 0, None) < 0 and b"null records" in lib.paac_last_error()
    assert lib.paac_user_game_step(1, 0, 0, *ptrs, ctypes.byref(rec), 0, None) < 0 and b"bad arguments" in lib.paac_last_error()
    for hole in (0, 1, 2, 4, 5):
        holed = list(ptrs)
        holed[hole] = None
        assert lib.paac_user_game_step(1, 0, N, *holed, ctypes.byref(rec), 0, None) < 0 and b"bad arguments" in lib.paac_last_error()
    assert lib.paac_user_game_reset(1, 0, 0, state.data_ptr(), stack.data_ptr(), None) < 0
    assert lib.paac_user_game_reset(1, 0, N, None, stack.data_ptr(), None) < 0
    # an id no game has: the user-game library's list names the user game
    assert lib.paac_game_step(4, 1, 0, N, *ptrs, ctypes.byref(rec), 0, None) < 0
    assert b"rally (2), the user game (3)" in lib.paac_last_error()
    torch.cuda.synchronize()
    assert not state_b.any() and not stack_b.any()          # nothing was launched
    print("refusals ok")


def check_stock_refusals():
    """The stock library: no user game in it."""
    import ctypes
    import torch
    from paac_amd import _lib, hip_ops
    assert _lib.user_game() is None and os.path.basename(_lib.LIB_PATH) == "libpaac_hip.so"
    N, W = 2, 20
    stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    stack_b = torch.zeros_like(stack)
    state = torch.zeros((N, W), dtype=torch.int32, device="cuda")
    state_b = torch.zeros_like(state)
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    f, i = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    rec = _lib.EnvRecords(f.data_ptr(), f.data_ptr(), f.data_ptr(), i.data_ptr(), None, None)
    ptrs = [actions.data_ptr(), state.data_ptr(), state_b.data_ptr(), None, stack.data_ptr(), stack_b.data_ptr(), None]
    for rc in (lib.paac_user_game_step(1, 0, N, *ptrs, ctypes.byref(rec), 0, None),
               lib.paac_user_game_reset(1, 0, N, state_b.data_ptr(), stack_b.data_ptr(), None)):
        message = lib.paac_last_error().decode()
        assert rc < 0 and "built without a user game" in message and "--device_game" in message, message
    assert lib.paac_game_step(_lib.EVAL_USER, 1, 0, N, *ptrs, ctypes.byref(rec), 0, None) < 0
    assert lib.paac_last_error() == b"paac_game_step: game 3 is none of catch (0), bricks (1), rally (2)"
    try:
        hip_ops.user_game_reset(1, 0, state_b, stack_b)
        raise AssertionError("not refused")
    except ValueError as exc:
        assert "no user game is registered" in str(exc)
    torch.cuda.synchronize()
    assert not state_b.any() and not stack_b.any()
    print("stock refusals ok")


def make_args(**kw):
    import tempfile
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "user", "--device_game", PATROL])
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_test_")
    args.emulator_workers = 0
    args.max_global_steps = 1 << 40
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def build_learner(args, params_seed=0):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(params_seed))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


def check_device_loop(sampler):
    """N = 8, T = 5, NIPS: eager, captured and batched-replay runs agree bit for bit and replay through 8 twins."""
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 8, 5, 6
    outs, records = [], []
    for mode in ("eager", "captured", "batched"):
        learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler=sampler, arch="NIPS"))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        spec = learner.environment_creator.device_env_spec
        assert spec == dict(kind="user", seed=3, single_life=False) and learner.num_actions == 18
        ro = DeviceRollout(learner, spec, sampler=sampler, use_graph=mode != "eager")
        assert ro.stateful and tuple(ro.env_state.shape) == (2 * T + 1, N, 20) and ro.A == 18
        if mode == "batched":
            ro.run_cycles(cycles)
        else:
            for _ in range(cycles):
                ro.run_cycle()
                if mode == "eager":
                    ro.synchronize()
                    records.append((ro.actions.cpu().numpy().copy(), ro.rewards.cpu().numpy().copy(),
                                    ro.masks.cpu().numpy().copy(), ro.rollout_states().cpu().numpy().copy()))
        ro.synchronize()
        outs.append(dict(params=learner.network.get_parameters(), stacks=ro.states.cpu().numpy().copy(),
                         states=ro.env_state.cpu().numpy().copy(), actions=ro.actions.cpu().numpy().copy(),
                         rewards=ro.rewards.cpu().numpy().copy(), masks=ro.masks.cpu().numpy().copy(),
                         step=int(ro.global_step_dev.item()), finished=ro.finished_episodes()))
        ro.close()
    for other in outs[1:]:
        assert other["step"] == outs[0]["step"] == cycles * N * T
        for k in ("stacks", "states", "actions", "rewards", "masks"):
            assert np.array_equal(outs[0][k], other[k]), k
        for k, v in outs[0]["params"].items():
            assert np.array_equal(v, other["params"][k]), k
        assert outs[0]["finished"][0] == other["finished"][0] and sorted(outs[0]["finished"][1]) == sorted(other["finished"][1])
    module = patrol()
    twins = [module.Environment(e, seed=3) for e in range(N)]
    obs = np.stack([env.get_initial_state() for env in twins])
    played = set()
    for c, (actions, rewards, masks, trained_on) in enumerate(records):
        assert actions.min() >= 0 and actions.max() <= 17
        played.update(actions.reshape(-1).tolist())
        for t in range(T):
            assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "cycle %d step %d" % (c, t)
            obs, want_rew, want_msk, _ = step_twins(twins, actions[t])
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], want_msk), "cycle %d step %d" % (c, t)
    assert len(played) >= 12, played                       # 240 draws from a fresh policy over 18 actions
    last = (cycles & 1) * T
    assert np.array_equal(outs[0]["stacks"][last], obs)
    assert np.array_equal(outs[0]["states"][last], np.stack([env.state_words() for env in twins]))
    print("%s: actions %s" % (sampler, sorted(played)))


def check_host_loop():
    """The host loop stepping the twin as a plugin == the device loop on the same np.random sampler stream."""
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 8, 5, 4
    feeds = []
    host = build_learner(make_args(emulator_counts=N, max_local_steps=T, max_global_steps=cycles * N * T, sampler="numpy",
                                   host_environments=True, record_feeds=True, feed_callback=feeds.append, arch="NIPS"))
    np.random.seed(7)
    host.train()
    assert len(feeds) == cycles
    devl = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler="numpy", arch="NIPS"))
    np.random.seed(7)
    devl.global_step = devl.init_network()
    ro = DeviceRollout(devl, devl.environment_creator.device_env_spec, sampler="numpy", use_graph=True)
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        assert np.array_equal(ro.rollout_states().cpu().numpy(), feeds[c]["states"]), "cycle %d" % c
        assert np.array_equal(ro.actions.view(-1).cpu().numpy(), feeds[c]["actions"]), "cycle %d" % c
        assert np.array_equal(ro.rewards.cpu().numpy(), feeds[c]["rewards"]), "cycle %d" % c
        assert np.array_equal(ro.masks.cpu().numpy(), feeds[c]["masks"]), "cycle %d" % c
        assert np.allclose(ro.y.cpu().numpy(), feeds[c]["y"], atol=1e-5)
    gh, gd = host.network.get_parameters(), devl.network.get_parameters()
    for k in gh:
        assert np.abs(gh[k] - gd[k]).max() < 1e-5, k
    ro.close()
    print("host loop ok")


def check_eval_step():
    """paac_eval_step with PAAC_EVAL_USER behind the acting forward of a seeded network against the replay on the twins."""
    import torch
    from paac_amd import evaluation, hip_ops, train
    EVAL_SEED, N, A, steps, env_offset, dev = (0x5EED << 32) + 11, 6, 18, 40, 0, "cuda"
    network_creator, env_creator = train.get_network_and_environment_creator(make_args(arch="NIPS"))
    network = network_creator()
    network.initialize(np.random.RandomState(0))
    ctx = hip_ops.Context(network.arch_id, A, max_batch=8)
    for greedy, noops in ((True, 0), (True, 3), (False, 0), (False, 3)):
        stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        states = [torch.zeros((N, 20), dtype=torch.int32, device=dev) for _ in range(2)]
        probs = torch.zeros((N, A), dtype=torch.float32, device=dev)
        actions = torch.zeros((steps, N), dtype=torch.int32, device=dev)
        score = torch.zeros(N, dtype=torch.float32, device=dev)
        length, done = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
        alive = torch.full((1,), N, dtype=torch.int32, device=dev)
        hip_ops.user_game_reset(SEED, env_offset, states[0], stacks[0])
        for t in range(steps):
            a, b = t & 1, (t & 1) ^ 1
            ctx.forward(network.params, stacks[a], probs=probs)
            hip_ops.eval_step("user", probs, greedy, EVAL_SEED, noops, None, t, SEED, env_offset, states[a], states[b], stacks[a],
                              stacks[b], actions[t], score, length, done, alive)
        trace = actions.cpu().numpy()
        noops_e = evaluation.eval_noops(EVAL_SEED, env_offset + np.arange(N), noops)
        assert trace.min() >= 0 and trace.max() <= 17
        for e in range(N):
            assert not trace[:noops_e[e], e].any()
        twins = [env_creator.create_environment(env_offset + e) for e in range(N)]
        for env in twins:
            env.get_initial_state()
        rewards, terminals = np.zeros((steps, N), dtype=np.float32), np.zeros((steps, N), dtype=bool)
        for t in range(steps):
            rewards[t], terminals[t] = evaluation.step_twins(twins, trace[t])
        final = steps & 1
        assert np.array_equal(states[final].cpu().numpy(), np.stack([env.state_words() for env in twins]))
        assert np.array_equal(stacks[final].cpu().numpy(), np.stack([env.stack for env in twins]))
        want_score, want_length, want_done = evaluation.account(rewards, terminals, noops_e)
        got = (score.cpu().numpy(), length.cpu().numpy(), done.cpu().numpy())
        print("greedy %s, noops %s: scores %s lengths %s done %s" % (greedy, noops_e, got[0], got[1], got[2]))
        assert np.array_equal(got[0], want_score) and np.array_equal(got[1], want_length) and np.array_equal(got[2], want_done)
        assert int(alive.item()) == N - int(want_done.sum())
        replayed = evaluation.replay_on_twins(env_creator, trace, noops_e, env_offset=env_offset)
        assert np.array_equal(got[0], replayed[0]) and np.array_equal(got[1], replayed[1])
        if not greedy:
            assert len(set(trace[noops:].reshape(-1).tolist())) >= 8
    ctx.close()


def check_learns(steps, bar):
    """--emulator user --device_game examples/patrol/patrol.py through train.main: the final greedy --eval_every evaluation on
    64 held-out instances."""
    import json
    import tempfile
    from paac_amd import train
    folder = tempfile.mkdtemp(prefix="paac_patrol_")
    steps = int(steps)
    args = train.get_arg_parser().parse_args(["--emulator", "user", "--device_game", PATROL, "-df", folder, "-ew", "0",
                                              "--max_global_steps", str(steps), "--eval_every", str(steps), "--arch", "NIPS"]
                                             + sys.argv[4:])
    train.main(args)
    evals = [json.loads(line) for line in open(os.path.join(folder, "metrics.jsonl"))]
    evals = [r for r in evals if r["kind"] == "eval"]
    for r in evals:
        print("evaluation at %d steps: mean %+.3f (min %+.1f, max %+.1f, std %.2f), mean length %.1f"
              % (r["global_step"], r["mean"], r["min"], r["max"], r["std"], r["mean_length"]))
    assert evals and evals[-1]["count"] == 64 and evals[-1]["greedy"]
    assert evals[-1]["mean"] >= float(bar), evals[-1]


if __name__ == "__main__":
    {"kernel": check_kernel, "crafted": check_crafted, "refusals": check_refusals, "stock_refusals": check_stock_refusals,
     "device_loop": check_device_loop, "host_loop": check_host_loop, "eval_step": check_eval_step,
     "learns": check_learns}[sys.argv[1]](*(sys.argv[2:4] if sys.argv[1] == "learns" else sys.argv[2:]))
    print("CHECK_OK")
