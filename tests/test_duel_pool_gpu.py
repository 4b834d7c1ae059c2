"""-m gpu: duel against a pool of past selves on the device (paac_duel_ghost_reset / paac_duel_ghost_step, DeviceRollout with
a pooled duel spec, the training loop's pool events) against the specification paac_amd/duel_pool.py and its numpy twin."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from paac_amd import duel, duel_pool, rally                        # noqa: E402
from test_truncation import returns_restated                       # noqa: E402  (the host estimators of --bootstrap_truncated)

SEED, SAMPLER_SEED, A = 3, 42, 6


def drained(fin):
    """The device ring of finished episodes -> (count, sorted [(reward, length)])."""
    host = fin.cpu().numpy()
    count = int(host[0])
    assert count <= 4096
    return count, sorted(zip(host[2:2 + 4096].view(np.float32)[:count].tolist(), host[2 + 4096:2 + 4096 + count].tolist()))


class Buffers(object):
    """What paac_duel_ghost_step launches of N boards read and write; records and both stacks ping-pong between 0 and 1."""

    def __init__(self, N, env_offset=0, steps=1, tick=0, dev="cuda"):
        from paac_amd import hip_ops
        W = hip_ops.DUEL_STATE_WORDS
        self.N, self.env_offset = N, env_offset
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.ghosts = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, W), dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2, self.ghost2 = (torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2))
        self.state2 = torch.zeros((N, W), dtype=torch.int32, device=dev)
        self.actions = torch.zeros((steps, N), dtype=torch.int32, device=dev)
        self.probs = torch.zeros((steps, N, A), dtype=torch.float32, device=dev)
        self.ghost_actions = torch.full((steps, N), -1, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r = (torch.zeros(N, device=dev) for _ in range(3))
        self.truncs = torch.full((N,), 7.0, device=dev)
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)
        self.tick = torch.full((1,), int(tick), dtype=torch.int64, device=dev)

    def reset(self):
        from paac_amd import hip_ops
        hip_ops.duel_ghost_reset(SEED, self.env_offset, self.states[0], self.stacks[0], self.ghosts[0])

    def step(self, slot=0, parity=0, step_offset=0, second=False, truncs=True, tick=True):
        from paac_amd import hip_ops
        a, b = parity, parity ^ 1
        hip_ops.duel_ghost_step(SEED, self.env_offset, self.actions[slot], self.probs[slot], SAMPLER_SEED,
                                self.tick if tick else None, step_offset, self.states[a], self.states[b], self.stacks[a],
                                self.stacks[b], self.ghosts[a], self.ghosts[b], self.ghost_actions[slot], self.rew, self.msk,
                                self.ep_r, self.ep_l, self.fin, stack_out2=self.stack2 if second else None,
                                state_out2=self.state2 if second else None, ghost_stack_out2=self.ghost2 if second else None,
                                truncs_out=self.truncs if truncs else None)

    def upload(self, actions, probs, slot=0):
        self.actions[slot].copy_(torch.from_numpy(np.asarray(actions, dtype=np.int32)))
        self.probs[slot].copy_(torch.from_numpy(np.asarray(probs, dtype=np.float32)))


class Accounts(object):
    """ep_reward / ep_len / the finished episodes as the step's bookkeeping keeps them, on the host."""

    def __init__(self, N):
        self.ep_r, self.ep_l, self.finished = np.zeros(N, np.float32), np.zeros(N, np.int32), []

    def step(self, rewards, terminals):
        self.ep_r += rewards
        self.ep_l += 1
        for e in np.nonzero(terminals)[0]:
            self.finished.append((float(self.ep_r[e]), int(self.ep_l[e])))
            self.ep_r[e], self.ep_l[e] = 0.0, 0


def check_step(b, out, want, ghost_actions, accounts, where):
    """Everything one launch wrote into ping-pong side `out` against the twin's step `want`."""
    records, stacks, ghosts, rewards, terminals, truncated = want
    accounts.step(rewards, terminals)
    assert np.array_equal(b.states[out].cpu().numpy(), records), "%s: records" % (where,)
    assert np.array_equal(b.stacks[out].cpu().numpy(), stacks), "%s: the learner's observations" % (where,)
    assert np.array_equal(b.ghosts[out].cpu().numpy(), ghosts), "%s: the ghosts' observations" % (where,)
    got = b.rew.cpu().numpy()
    assert np.array_equal(got, rewards) and not np.signbit(got[got == 0.0]).any(), "%s: rewards" % (where,)
    assert np.array_equal(b.msk.cpu().numpy(), 1.0 - terminals.astype(np.float32)), "%s: masks" % (where,)
    assert np.array_equal(b.ep_r.cpu().numpy(), accounts.ep_r) and np.array_equal(b.ep_l.cpu().numpy(), accounts.ep_l), where
    assert np.array_equal(b.truncs.cpu().numpy(), truncated.astype(np.float32)), "%s: truncation plane" % (where,)
    assert np.array_equal(b.ghost_actions[0].cpu().numpy(), ghost_actions), "%s: ghost actions" % (where,)


@pytest.mark.parametrize("N,env_offset", [(1, 0), (3, 4)])
def test_step_entry_matches_the_twin_bit_for_bit(N, env_offset):
    """300 ping-pong steps under uploaded random learner actions and random normalised ghost rows, the tick crossing 2^32:
    after every step the records, both stacks (all four channels), rewards, masks, episode totals, the truncation plane and the
    ghosts' actions are the twin's; the finished ring at the end.  N = 1: the two columns of one board."""
    steps, base = 300, (1 << 32) - 150
    b, twin, accounts = Buffers(N, env_offset, tick=base), duel_pool.PooledBoards(N, SEED, env_offset), Accounts(N)
    records, stacks, ghosts = twin.reset()
    b.reset()
    assert np.array_equal(b.states[0].cpu().numpy(), records) and np.array_equal(b.stacks[0].cpu().numpy(), stacks)
    assert np.array_equal(b.ghosts[0].cpu().numpy(), ghosts)
    rs = np.random.RandomState(20 + N)
    ids = env_offset + np.arange(N)
    played, points = set(), 0
    for step in range(steps):
        a = rs.randint(A, size=N).astype(np.int32)
        p = rs.dirichlet(np.ones(A) * 0.5, size=N).astype(np.float32)
        b.upload(a, p)
        b.step(parity=step & 1, step_offset=step)
        g = duel_pool.ghost_actions(p, SAMPLER_SEED, base + step, ids)
        want = twin.step(a, g)
        check_step(b, (step & 1) ^ 1, want, g, accounts, "step %d" % step)
        played.update(g.tolist())
        points += int((want[3] != 0).sum())
    assert drained(b.fin) == (len(accounts.finished), sorted(accounts.finished))
    assert played == set(range(A)) and points >= 5


def test_the_step_cap_truncates_and_drops_both_histories():
    """A crafted record ten steps short of the cap, the learner always NOOP, the ghost playing rally's script through one-hot
    rows (a certain action whatever the random word): the capping step is terminal AND truncated, the next episode starts, and
    the history of both stacks is dropped -- only the newest channel is set."""
    N = 2
    b, twin, accounts = Buffers(N), duel_pool.PooledBoards(N, SEED), Accounts(N)
    twin.reset()
    board = (5, 8, 1, 1, 9, 3, 1, 2, 990, 4)
    twin.boards.rows = [board, board, duel.mirror(board), duel.mirror(board)]
    history = np.random.RandomState(4).randint(0, 256, (2 * N, 84, 84, 4)).astype(np.uint8)
    twin.boards.stacks = history.copy()
    b.states[0].copy_(torch.from_numpy(twin.boards.records()[:N]))
    b.stacks[0].copy_(torch.from_numpy(history[:N]))
    b.ghosts[0].copy_(torch.from_numpy(history[N:]))
    seen = []
    for step in range(24):
        g = np.array([duel.scripted_top_action(SEED, e, twin.boards.rows[e]) for e in range(N)], dtype=np.int32)
        b.upload([rally.NOOP] * N, np.eye(A, dtype=np.float32)[g])
        b.step(parity=step & 1, step_offset=step)
        want = twin.step([rally.NOOP] * N, g)
        check_step(b, (step & 1) ^ 1, want, g, accounts, "step %d" % step)
        seen.append((want[4].tolist(), want[5].tolist()))
        if step == 9:
            for stack in (b.stacks[0], b.ghosts[0]):          # (step 9 wrote side 0)
                host = stack.cpu().numpy()
                assert not host[..., :3].any() and host[..., 3].any()
    assert seen[9] == ([True] * N, [True] * N)                           # steps 990 -> 1000
    assert all(t == [False] * N for _, t in seen[:9] + seen[10:])
    assert [l for _, l in accounts.finished] == [10] * N


def test_second_outputs_a_missing_plane_and_a_null_tick():
    N, env_offset, steps = 3, 4, 40
    rs = np.random.RandomState(5)
    script = rs.randint(A, size=(steps, N)).astype(np.int32)
    probs = rs.dirichlet(np.ones(A), size=(steps, N)).astype(np.float32)
    runs = []
    for second, truncs, tick in ((False, True, True), (True, True, True), (True, False, True), (False, True, False)):
        b = Buffers(N, env_offset, tick=0)
        b.reset()
        trace = []
        for step in range(steps):
            b.upload(script[step], probs[step])
            b.step(parity=step & 1, step_offset=step, second=second, truncs=truncs, tick=tick)
            out = (step & 1) ^ 1
            if second:
                assert torch.equal(b.stack2, b.stacks[out]) and torch.equal(b.state2, b.states[out]), step
                assert torch.equal(b.ghost2, b.ghosts[out]), step
            trace.append(b.ghost_actions[0].cpu().numpy().copy())
        last = steps & 1
        runs.append([t.cpu().numpy().copy() for t in (b.states[last], b.stacks[last], b.ghosts[last], b.rew, b.msk, b.ep_r, b.ep_l)]
                    + [np.stack(trace), drained(b.fin), b.truncs.cpu().numpy().copy(), (b.stack2.any().item(), b.ghost2.any().item())])
    for other in runs[1:]:
        for x, y in zip(runs[0][:8], other[:8]):
            assert np.array_equal(x, y)
        assert runs[0][8] == other[8]
    ids = env_offset + np.arange(N)
    for step in range(steps):          # a null tick is tick 0: the step's offset alone
        assert np.array_equal(runs[3][7][step], duel_pool.ghost_actions(probs[step], SAMPLER_SEED, step, ids))
    assert np.array_equal(runs[0][9], runs[1][9]) and set(runs[0][9].tolist()) <= {0.0, 1.0}
    assert (runs[2][9] == 7.0).all()                                      # truncs_out=None: the plane was not written
    assert runs[0][10] == (False, False) and runs[1][10] == (True, True)  # no second output asked for: none written


def test_refusals_name_the_argument_and_launch_nothing():
    from paac_amd import _lib, hip_ops
    N = 2
    b = Buffers(N)
    b.reset()
    b.upload([1, 2], np.full((N, A), 1.0 / A))
    torch.cuda.synchronize()
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f, m, r = (torch.zeros(N, device="cuda") for _ in range(3))
    i = torch.zeros(N, dtype=torch.int32, device="cuda")
    rec = _lib.EnvRecords(f.data_ptr(), m.data_ptr(), r.data_ptr(), i.data_ptr(), None, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731

    def arguments(**change):
        args = dict(N=N, actions=p(b.actions[0]), ghost_probs=p(b.probs[0]), A=A, state_in=p(b.states[0]), state_out=p(b.states[1]),
                    state_out2=None, stack_in=p(b.stacks[0]), stack_out=p(b.stacks[1]), stack_out2=None,
                    ghost_stack_in=p(b.ghosts[0]), ghost_stack_out=p(b.ghosts[1]), ghost_stack_out2=None, rec=ctypes.byref(rec),
                    ghost_actions_out=p(b.ghost_actions[0]))
        args.update(change)
        return (SEED, 0, args["N"], args["actions"], args["ghost_probs"], args["A"], SAMPLER_SEED, None, 0, args["state_in"],
                args["state_out"], args["state_out2"], args["stack_in"], args["stack_out"], args["stack_out2"],
                args["ghost_stack_in"], args["ghost_stack_out"], args["ghost_stack_out2"], args["rec"], args["ghost_actions_out"],
                stream)

    no_rewards = _lib.EnvRecords(None, m.data_ptr(), r.data_ptr(), i.data_ptr(), None, None)
    for change, named in ((dict(N=0), "N=0"), (dict(N=-2), "N=-2"), (dict(A=4), "A=4"), (dict(actions=None), "actions"),
                          (dict(ghost_probs=None), "ghost_probs"), (dict(state_in=None), "state_in"),
                          (dict(state_out=None), "state_out"), (dict(stack_in=None), "stack_in"),
                          (dict(stack_out=None), "stack_out"), (dict(ghost_stack_in=None), "ghost_stack_in"),
                          (dict(ghost_stack_out=None), "ghost_stack_out"), (dict(rec=None), "records"),
                          (dict(rec=ctypes.byref(no_rewards)), "rewards"), (dict(ghost_actions_out=None), "ghost_actions_out"),
                          (dict(state_out=p(b.states[0])), "state_in is state_out"),
                          (dict(state_out2=p(b.states[0])), "state_in is state_out"),
                          (dict(stack_out=p(b.stacks[0])), "stack_in is stack_out"),
                          (dict(stack_out2=p(b.stacks[0])), "stack_in is stack_out"),
                          (dict(ghost_stack_out=p(b.ghosts[0])), "ghost_stack_in is ghost_stack_out"),
                          (dict(ghost_stack_out2=p(b.ghosts[0])), "ghost_stack_in is ghost_stack_out"),
                          (dict(ghost_stack_out=p(b.stacks[1])), "overlap")):
        rc = lib.paac_duel_ghost_step(*arguments(**change))
        message = lib.paac_last_error().decode()
        assert rc < 0 and "paac_duel_ghost_step: " in message and named in message, (change, message)
    for args, named in (((SEED, 0, 0, p(b.states[1]), p(b.stacks[1]), p(b.ghosts[1]), stream), "N=0"),
                        ((SEED, 0, N, None, p(b.stacks[1]), p(b.ghosts[1]), stream), "state_out"),
                        ((SEED, 0, N, p(b.states[1]), None, p(b.ghosts[1]), stream), "stack_out"),
                        ((SEED, 0, N, p(b.states[1]), p(b.stacks[1]), None, stream), "ghost_stack_out"),
                        ((SEED, 0, N, p(b.states[1]), p(b.stacks[1]), p(b.stacks[1]), stream), "same buffer")):
        rc = lib.paac_duel_ghost_reset(*args)
        message = lib.paac_last_error().decode()
        assert rc < 0 and "paac_duel_ghost_reset: " in message and named in message, message
    # the wrappers' own shape checks
    with pytest.raises(ValueError):
        hip_ops.duel_ghost_reset(SEED, 0, torch.zeros((N, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"),
                                 b.stacks[1], b.ghosts[1])
    with pytest.raises(ValueError):
        hip_ops.duel_ghost_reset(SEED, 0, b.states[1], b.stacks[1], b.ghosts[1][:1])
    with pytest.raises(ValueError, match="ghost_probs"):
        hip_ops.duel_ghost_step(SEED, 0, b.actions[0], b.probs[0][:1], SAMPLER_SEED, None, 0, b.states[0], b.states[1],
                                b.stacks[0], b.stacks[1], b.ghosts[0], b.ghosts[1], b.ghost_actions[0], f, m, r, i)
    with pytest.raises(ValueError, match="ghost_stack_out"):
        hip_ops.duel_ghost_step(SEED, 0, b.actions[0], b.probs[0], SAMPLER_SEED, None, 0, b.states[0], b.states[1],
                                b.stacks[0], b.stacks[1], b.ghosts[0], b.ghosts[1][:1], b.ghost_actions[0], f, m, r, i)
    with pytest.raises(_lib.PaacHipError, match=r"paac_duel_ghost_step: A=4"):
        hip_ops.duel_ghost_step(SEED, 0, b.actions[0], torch.zeros((N, 4), device="cuda"), SAMPLER_SEED, None, 0, b.states[0],
                                b.states[1], b.stacks[0], b.stacks[1], b.ghosts[0], b.ghosts[1], b.ghost_actions[0], f, m, r, i)
    torch.cuda.synchronize()
    assert not b.states[1].any() and not b.stacks[1].any() and not b.ghosts[1].any()          # nothing was launched
    assert (b.ghost_actions == -1).all() and not f.any()
    b.step()                                                                                   # ... and the plain call is fine
    torch.cuda.synchronize()
    assert b.states[1].any() and b.ghosts[1].any() and (b.ghost_actions[0] >= 0).all()


def test_captured_block_replays_like_the_eager_steps():
    """16 steps in one hipGraph, replayed four times at N = 3: the device tick moves the ghosts' stream on by itself."""
    from paac_amd import hip_ops
    N, K, blocks, env_offset = 3, 16, 4, 1
    rs = np.random.RandomState(8)
    p = rs.dirichlet(np.ones(A), size=(K, N)).astype(np.float32)
    a = rs.randint(A, size=(K, N)).astype(np.int32)
    outs = []
    for captured in (False, True):
        b = Buffers(N, env_offset, steps=K)
        b.probs.copy_(torch.from_numpy(p))
        b.actions.copy_(torch.from_numpy(a))
        b.reset()
        torch.cuda.synchronize()

        def block():
            for j in range(K):
                b.step(slot=j, parity=j & 1, step_offset=j)
            hip_ops.counter_add(b.tick, K)

        stream = torch.cuda.Stream()
        trace = []
        with torch.cuda.stream(stream):
            graph = None
            if captured:
                graph = hip_ops.Graph()
                graph.begin()
                block()
                graph.end()
            for _ in range(blocks):
                graph.launch() if captured else block()
                trace.append(b.ghost_actions.cpu().numpy().copy())
            stream.synchronize()
            if graph is not None:
                graph.close()
        outs.append(dict(trace=np.concatenate(trace), states=b.states[0].cpu().numpy(), stacks=b.stacks[0].cpu().numpy(),
                         ghosts=b.ghosts[0].cpu().numpy(), ep=(b.ep_r.cpu().numpy(), b.ep_l.cpu().numpy()), fin=drained(b.fin),
                         tick=int(b.tick.item())))
    eager, replayed = outs
    assert eager["tick"] == replayed["tick"] == K * blocks
    for k in ("trace", "states", "stacks", "ghosts"):
        assert np.array_equal(eager[k], replayed[k]), k
    assert eager["fin"] == replayed["fin"] and all(np.array_equal(x, y) for x, y in zip(eager["ep"], replayed["ep"]))
    # ... and both are the specification
    twin = duel_pool.PooledBoards(N, SEED, env_offset)
    twin.reset()
    ids = env_offset + np.arange(N)
    for t in range(K * blocks):
        g = duel_pool.ghost_actions(p[t % K], SAMPLER_SEED, t, ids)
        assert np.array_equal(eager["trace"][t], g), t
        records, stacks, ghosts = twin.step(a[t % K], g)[:3]
    assert np.array_equal(eager["states"], records) and np.array_equal(eager["stacks"], stacks)
    assert np.array_equal(eager["ghosts"], ghosts)


# -- through the device loop -----------------------------------------------------------------------------------------------------
def make_args(*flags, **kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "duel", "--arch", "NIPS"] + list(flags))
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_pooltest_")
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


def pooled_rollout(flags=(), N=4, T=5, sampler="philox", use_graph=False, **kw):
    from paac_amd.paac import DeviceRollout
    learner = build_learner(make_args("-ec", str(N), "--max_local_steps", str(T), "--sampler", sampler, "--duel_pool", "3", *flags,
                                      **kw))
    np.random.seed(9)
    learner.global_step = learner.init_network()
    spec = learner.environment_creator.device_env_spec
    assert spec == dict(kind="duel", seed=3, pool=3) and learner.num_actions == A
    ro = DeviceRollout(learner, spec, sampler=sampler, use_graph=use_graph)
    learner.rollout = ro
    assert ro.pool is not None and ro.route == "stateful" and tuple(ro.env_state.shape) == (2 * T + 1, N, 12)
    assert tuple(ro.ghost_states.shape) == tuple(ro.states.shape) and tuple(ro.ghost_actions.shape) == (T, N)
    assert tuple(ro.pool.pool.shape) == (3, learner.network.params.numel()) and torch.equal(ro.pool.opponent, learner.network.params)
    assert ro.pool.opponent.data_ptr() != learner.network.params.data_ptr()
    return learner, ro


@pytest.mark.parametrize("sampler,cycles", [("philox", 6), ("numpy", 6)])
def test_device_loop_replays_like_the_eager_run_and_through_the_twin(sampler, cycles):
    N, T = 4, 5
    outs, records = [], []
    for mode in ("eager", "captured"):
        learner, ro = pooled_rollout(N=N, T=T, sampler=sampler, use_graph=mode != "eager")
        opponent = ro.pool.opponent.clone()
        for _ in range(cycles):
            ro.run_cycle()
            ro.synchronize()
            records.append((mode, ro.actions.cpu().numpy().copy(), ro.ghost_actions.cpu().numpy().copy(),
                            ro.rewards.cpu().numpy().copy(), ro.masks.cpu().numpy().copy(),
                            ro.rollout_states().cpu().numpy().copy(), ro.ghost_states.cpu().numpy().copy(),
                            ro.ghost_probs.cpu().numpy().copy()))
        assert torch.equal(ro.pool.opponent, opponent) and not torch.equal(opponent, learner.network.params)     # frozen
        outs.append(dict(params=learner.network.get_parameters(), stacks=ro.states.cpu().numpy().copy(),
                         ghosts=ro.ghost_states.cpu().numpy().copy(), states=ro.env_state.cpu().numpy().copy(),
                         step=int(ro.global_step_dev.item()), finished=ro.finished_episodes()))
        ro.close()
        ro.pool.close()
    eager, captured = outs
    assert eager["step"] == captured["step"] == cycles * N * T
    for k in ("stacks", "ghosts", "states"):
        assert np.array_equal(eager[k], captured[k]), k
    for k, v in eager["params"].items():
        assert np.array_equal(v, captured["params"][k]) and np.isfinite(v).all(), k
    assert eager["finished"][0] == captured["finished"][0] and sorted(eager["finished"][1]) == sorted(captured["finished"][1])
    # both runs through the twin, from `actions` and `ghost_actions`: every observation trained on, the ghosts' ring, every
    # reward and mask -- and the ghosts' actions are the rule on the probabilities the last step left
    for mode in ("eager", "captured"):
        twin = duel_pool.PooledBoards(N, seed=3)
        _, obs, ghost_obs = twin.reset()
        played = set()
        for c, (_, actions, ghost_actions, rewards, masks, trained_on, ghost_ring, ghost_probs) in enumerate(
                [r for r in records if r[0] == mode]):
            played.update(ghost_actions.reshape(-1).tolist())
            parity = c & 1
            for t in range(T):
                assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "%s cycle %d step %d" % (mode, c, t)
                assert np.array_equal(ghost_ring[parity * T + t], ghost_obs), "%s cycle %d step %d: ghosts" % (mode, c, t)
                _, obs, ghost_obs, want_rew, want_term, _ = twin.step(actions[t], ghost_actions[t])
                assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], 1.0 - want_term.astype(np.float32)), (c, t)
            assert np.array_equal(ghost_ring[parity * T + T], ghost_obs)
            if parity == 1:
                assert np.array_equal(ghost_ring[0], ghost_obs)          # the wrap output
            tick = c * T + T - 1
            assert np.array_equal(ghost_actions[T - 1], duel_pool.ghost_actions(ghost_probs, 42, tick, np.arange(N)))
            assert np.allclose(ghost_probs.sum(axis=1), 1.0, atol=1e-5)
        assert played <= set(range(A)) and len(played) >= 3, played
    last = (cycles & 1) * T
    assert np.array_equal(eager["stacks"][last], obs) and np.array_equal(eager["ghosts"][last], ghost_obs)


def test_the_ghost_is_frozen_and_reaches_the_update_through_the_records_only():
    """One cycle from the same start under three opponents: the run's own start weights, the same with the actor bias moved by
    1e-5 (other probabilities bit for bit, the same sampled actions), and another network.  The ghosts' probabilities follow the
    opponent tensor; where the records agree, the gradient and the updated weights agree bit for bit."""
    from paac_amd import train
    outs = []
    for variant in ("own", "nudged", "other"):
        learner, ro = pooled_rollout()
        if variant != "own":
            other = train.get_network_and_environment_creator(make_args())[0]()
            other.initialize(np.random.RandomState(0 if variant == "nudged" else 5))
            weights = other.params.clone()
            if variant == "nudged":
                assert torch.equal(weights, ro.pool.opponent)
                bias = [t for t in learner.network.layout["tensors"] if t["name"] == "actor_output_biases"][0]
                assert bias["size"] == A
                weights[bias["offset"]:bias["offset"] + A] += torch.linspace(-1e-5, 1e-5, A, device=weights.device)
            ro.pool.set_opponent(weights)
        live = learner.network.params.clone()
        ro.run_cycle()
        ro.synchronize()
        outs.append(dict(probs=ro.ghost_probs.cpu().numpy().copy(), ghost_actions=ro.ghost_actions.cpu().numpy().copy(),
                         actions=ro.actions.cpu().numpy().copy(), rewards=ro.rewards.cpu().numpy().copy(),
                         states=ro.rollout_states().cpu().numpy().copy(), grad=learner.grad.cpu().numpy().copy(),
                         params=learner.network.params.cpu().numpy().copy()))
        assert not torch.equal(live, learner.network.params)
        ro.close()
        ro.pool.close()
    own, nudged, other = outs
    assert not np.array_equal(own["probs"], nudged["probs"]) and np.abs(own["probs"] - nudged["probs"]).max() < 1e-4
    assert np.abs(own["probs"] - other["probs"]).max() > 1e-4
    for k in ("ghost_actions", "actions", "rewards", "states"):          # the same records ...
        assert np.array_equal(own[k], nudged[k]), k
    assert np.array_equal(own["grad"], nudged["grad"]) and np.array_equal(own["params"], nudged["params"])      # ... the same update
    assert np.isfinite(own["grad"]).all() and own["grad"].any()


def test_ppo_gae_and_truncation_on_a_pooled_rollout():
    """--ppo_epochs 2 --gae_lambda 0.95 --adv_norm true --bootstrap_truncated true with the pool on, the boards moved to three
    steps before the cap: the plane has its ones at row 2, and the frozen y / adv are the host estimator's on the recorded
    rollout (the option set of test_truncation_gpu's PPO case)."""
    N, T, cap_at = 4, 5, 2
    learner, ro = pooled_rollout(("--ppo_epochs", "2", "--gae_lambda", "0.95", "--adv_norm", "true", "--bootstrap_truncated",
                                  "true"), N=N, T=T)
    assert ro.truncs is not None and tuple(ro.truncs.shape) == (T, N)
    ro.env_state[0][:, 8] = rally.MAX_STEPS - cap_at - 1          # the steps word: the planes do not depend on it
    ro.run_cycle()
    ro.synchronize()
    Bn = N * T
    v_boot = learner.ctx.debug_activation(25, Bn + N)[Bn:].cpu().numpy()
    host = (v_boot, ro.rewards.cpu().numpy(), ro.masks.cpu().numpy(), ro.values.cpu().numpy(), ro.truncs.cpu().numpy())
    want = np.zeros((T, N), np.float32)
    want[cap_at] = 1.0
    assert np.array_equal(host[4], want) and not host[2][cap_at].any() and learner.truncated_steps() == N
    ye, ae = returns_restated(*host, learner.gamma, 0.95)
    assert np.array_equal(ro.y.cpu().numpy(), ye.reshape(-1)) and np.array_equal(ro.adv.cpu().numpy(), ae.reshape(-1))
    y0, _ = returns_restated(*host[:4], np.zeros_like(host[4]), learner.gamma, 0.95)
    assert not np.array_equal(y0, ye)
    # a terminal step drops the ghosts' history too
    ghosts = ro.ghost_states[cap_at + 1].cpu().numpy()
    assert not ghosts[..., :3].any() and ghosts[..., 3].any()
    for v in learner.network.get_parameters().values():
        assert np.isfinite(v).all()
    ro.close()
    ro.pool.close()


def real_run(*flags, strip=False, max_global_steps=2600):
    from paac_amd import logger_utils
    args = make_args("-ec", "4", "--max_local_steps", "5", *flags, max_global_steps=max_global_steps)
    if strip:          # a Namespace from before the flags
        for name in ("duel_pool", "duel_pool_every", "duel_pool_latest_p"):
            delattr(args, name)
    logger_utils.save_args(args, args.debugging_folder)
    learner = build_learner(args)
    learner.train()
    path = os.path.join(args.debugging_folder, "metrics.jsonl")
    records = [json.loads(line) for line in open(path)] if os.path.exists(path) else []
    return args, learner.network.get_parameters(), records


def test_a_real_run_follows_the_schedule_and_its_folder_is_a_duel_folder(capsys):
    from paac_amd import test as harness
    flags = ("--duel_pool", "3", "--duel_pool_every", "640", "--eval_every", "1280", "--eval_match", "4", "--eval_count", "4")
    runs = [real_run(*flags) for _ in range(2)]
    args, params, records = runs[0]
    fields = ("global_step", "event", "slot", "size", "opponent_slot", "opponent_global_step", "latest")
    pool = [{k: r[k] for k in fields} for r in records if r["kind"] == "duel_pool"]
    want = duel_pool.schedule(0, 4 * 5, 2600, 3, 640, 0.5, int(args.random_seed))
    assert pool == want and [r["global_step"] for r in pool] == [640, 1280, 1920, 2560]
    pushed = {0} | {r["global_step"] for r in pool}
    assert all(r["opponent_global_step"] in pushed for r in pool)
    again = [{k: r[k] for k in fields} for r in runs[1][2] if r["kind"] == "duel_pool"]
    assert again == pool
    for k, v in params.items():          # ... and the same weights: the pool's draws are the run's own
        assert np.array_equal(v, runs[1][1][k]) and np.isfinite(v).all(), k
    assert [r["global_step"] for r in records if r["kind"] == "eval"] == [1280, 2560]
    assert [r["global_step"] for r in records if r["kind"] == "match"] == [1280, 2560]
    assert all(r["opponent"] == "scripted" for r in records if r["kind"] == "eval")
    capsys.readouterr()
    scores = harness.main(["-f", args.debugging_folder, "--device_environments", "true", "-tc", "4", "-np", "4"])
    assert scores.shape == (4,) and "Performed 4 tests" in capsys.readouterr().out


def test_pool_off_is_the_run_without_the_flag():
    """--duel_pool 0 (the other two flags set to anything) against a Namespace from before the flags: bit-equal weights, no
    `duel_pool` record, no pool."""
    off = real_run("--duel_pool", "0", "--duel_pool_every", "40", "--duel_pool_latest_p", "0.9", max_global_steps=200)
    before = real_run(strip=True, max_global_steps=200)
    assert not hasattr(before[0], "duel_pool") and off[0].duel_pool == 0
    for k, v in off[1].items():
        assert np.array_equal(v, before[1][k]), k
    assert not [r for r in off[2] + before[2] if r["kind"] == "duel_pool"]
    on = real_run("--duel_pool", "2", "--duel_pool_every", "40", max_global_steps=200)
    assert any(not np.array_equal(v, on[1][k]) for k, v in off[1].items())          # the flag does change the run
    assert [r["global_step"] for r in on[2] if r["kind"] == "duel_pool"] == [40, 80, 120, 160, 200]
