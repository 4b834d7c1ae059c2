"""-m gpu: the duel game on the device (paac_duel_reset / paac_duel_step, DeviceRollout with a kind == "duel" spec, the
evaluation of a duel run) against its specification paac_amd/duel.py and the numpy twin DuelBoards."""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import duel, rally
from paac_amd.duel import DuelBoards

SEED = 3


def drained(fin):
    """The device ring of finished episodes -> (count, sorted [(reward, length)])."""
    host = fin.cpu().numpy()
    count = int(host[0])
    assert count <= 4096
    return count, sorted(zip(host[2:2 + 4096].view(np.float32)[:count].tolist(), host[2 + 4096:2 + 4096 + count].tolist()))


class Buffers(object):
    """What one paac_duel_step launch of N rows reads and writes."""

    def __init__(self, N, dev="cuda"):
        from paac_amd import hip_ops
        W = hip_ops.DUEL_STATE_WORDS
        self.N = N
        self.stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.states = [torch.zeros((N, W), dtype=torch.int32, device=dev) for _ in range(2)]
        self.stack2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
        self.state2 = torch.zeros((N, W), dtype=torch.int32, device=dev)
        self.actions = torch.zeros(N, dtype=torch.int32, device=dev)
        self.rew, self.msk, self.ep_r = (torch.zeros(N, device=dev) for _ in range(3))
        self.truncs = torch.full((N,), 7.0, device=dev)
        self.ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
        self.fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)

    def step(self, seed, env_offset, a, second=False, truncs=True):
        from paac_amd import hip_ops
        self.actions.copy_(torch.from_numpy(np.asarray(a, dtype=np.int32)))
        hip_ops.duel_step(seed, env_offset, self.actions, self.states[0], self.states[1], self.stacks[0], self.stacks[1],
                          self.rew, self.msk, self.ep_r, self.ep_l, self.fin, stack_out2=self.stack2 if second else None,
                          state_out2=self.state2 if second else None, truncs_out=self.truncs if truncs else None)

    def flip(self):
        self.stacks.reverse()
        self.states.reverse()


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


def check_step(b, want, accounts, where):
    """Everything one launch wrote against the twin's step `want` = (records, stacks, rewards, terminals, truncated)."""
    records, stacks, rewards, terminals, truncated = want
    accounts.step(rewards, terminals)
    assert np.array_equal(b.states[1].cpu().numpy(), records), "%s: state records" % (where,)
    assert np.array_equal(b.stacks[1].cpu().numpy(), stacks), "%s: observations" % (where,)
    got = b.rew.cpu().numpy()
    assert np.array_equal(got, rewards) and not np.signbit(got[got == 0.0]).any(), "%s: rewards" % (where,)
    assert np.array_equal(b.msk.cpu().numpy(), 1.0 - terminals.astype(np.float32)), "%s: masks" % (where,)
    assert np.array_equal(b.ep_r.cpu().numpy(), accounts.ep_r) and np.array_equal(b.ep_l.cpu().numpy(), accounts.ep_l), where
    assert np.array_equal(b.truncs.cpu().numpy(), truncated.astype(np.float32)), "%s: truncation plane" % (where,)


@pytest.mark.parametrize("N,env_offset", [(2, 0), (6, 4)])
def test_step_entry_matches_the_twin_bit_for_bit(N, env_offset):
    """1200 ping-pong steps (more than one step cap) under uploaded random actions: after every step the records, the
    observations (all four channels), rewards, masks, ep_reward, ep_len and the truncation plane are DuelBoards'; the finished
    ring at the end.  N = 2: one board, the partner index arithmetic at its smallest."""
    from paac_amd import hip_ops
    steps = 1200
    b, twin, accounts = Buffers(N), DuelBoards(N, seed=SEED, env_offset=env_offset), Accounts(N)
    records, stacks = twin.reset()
    hip_ops.duel_reset(SEED, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.states[0].cpu().numpy(), records) and np.array_equal(b.stacks[0].cpu().numpy(), stacks)
    script = np.random.RandomState(10 + N).randint(6, size=(steps, N)).astype(np.int32)
    points = 0
    for step in range(steps):
        b.step(SEED, env_offset, script[step])
        want = twin.step(script[step])
        check_step(b, want, accounts, "step %d" % step)
        points += int((want[2] > 0).sum())
        b.flip()
    assert drained(b.fin) == (len(accounts.finished), sorted(accounts.finished))
    # both players' episodes are in the ring: the returns of a board's two rows cancel
    assert len(accounts.finished) >= 2 * (N // 2) and len(accounts.finished) % 2 == 0 and points >= 5
    assert sum(r for r, _ in accounts.finished) == 0.0
    assert {k for _, _, _, _, _, _, _, _, _, k in twin.rows} != {0}          # odd episodes (served towards the top) were played


def test_the_step_cap_is_reached_and_marks_both_rows():
    """Row 0 always NOOP, its partner playing rally's script, from a crafted record ten steps short of the cap: the capping
    step is terminal and truncated on both rows, the plane's ones are written, and the next episode is served to the top."""
    from paac_amd import hip_ops
    N = 2
    b, twin, accounts = Buffers(N), DuelBoards(N, seed=SEED), Accounts(N)
    twin.reset()
    board = (5, 8, 1, 1, 9, 3, 1, 2, 990, 4)
    twin.rows = [board, duel.mirror(board)]
    history = np.random.RandomState(4).randint(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    twin.stacks = history.copy()
    b.states[0].copy_(torch.from_numpy(twin.records()))
    b.stacks[0].copy_(torch.from_numpy(history))
    seen = []
    for step in range(24):
        a = [rally.NOOP, duel.scripted_top_action(SEED, 0, twin.rows[0])]
        b.step(SEED, 0, a)
        want = twin.step(a)
        check_step(b, want, accounts, "step %d" % step)
        seen.append((want[3].tolist(), want[4].tolist()))
        b.flip()
    assert seen[9] == ([True, True], [True, True])                       # steps 990 -> 1000
    assert all(t == [False, False] for _, t in seen[:9] + seen[10:])
    assert [l for _, l in accounts.finished] == [10, 10] and sum(r for r, _ in accounts.finished) == 0.0
    assert twin.rows[0][9] == 5 and tuple(b.states[0].cpu().numpy()[0][:10]) == twin.rows[0]


def test_second_outputs_and_a_missing_plane_change_nothing_else():
    from paac_amd import hip_ops
    N, env_offset = 6, 4
    script = np.random.RandomState(5).randint(6, size=(40, N)).astype(np.int32)
    runs = []
    for second, truncs in ((False, True), (True, True), (True, False)):
        b = Buffers(N)
        hip_ops.duel_reset(SEED, env_offset, b.states[0], b.stacks[0])
        for step in range(len(script)):
            b.step(SEED, env_offset, script[step], second=second, truncs=truncs)
            if second:
                assert torch.equal(b.stack2, b.stacks[1]) and torch.equal(b.state2, b.states[1]), step
            b.flip()
        runs.append([t.cpu().numpy().copy() for t in (b.states[0], b.stacks[0], b.rew, b.msk, b.ep_r, b.ep_l, b.truncs)]
                    + [drained(b.fin)])
    for other in runs[1:]:
        for x, y in zip(runs[0][:6], other[:6]):
            assert np.array_equal(x, y)
        assert runs[0][7] == other[7]
    assert np.array_equal(runs[0][6], runs[1][6]) and set(runs[0][6].tolist()) <= {0.0, 1.0}
    assert (runs[2][6] == 7.0).all()                                      # truncs_out=None: the plane was not written


def test_refusals_name_the_entry_and_launch_nothing():
    from paac_amd import _lib, hip_ops

    def buffers(N):
        stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
        state = torch.zeros((N, hip_ops.DUEL_STATE_WORDS), dtype=torch.int32, device="cuda")
        return (stack, torch.zeros_like(stack), state, torch.zeros_like(state), torch.zeros(N, dtype=torch.int32, device="cuda"),
                torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"))

    for N in (3, 1):
        stack, stack_b, state, state_b, actions, f, i = buffers(N)
        with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_reset: "):
            hip_ops.duel_reset(1, 0, state_b, stack_b)
        with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
            hip_ops.duel_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i)
        torch.cuda.synchronize()
        assert not state_b.any() and not stack_b.any()
    stack, stack_b, state, state_b, actions, f, i = buffers(2)
    hip_ops.duel_reset(1, 0, state, stack)
    with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
        hip_ops.duel_step(1, 0, actions, state, state, stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
        hip_ops.duel_step(1, 0, actions, state, state_b, stack, stack, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
        hip_ops.duel_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, state_out2=state)
    with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
        hip_ops.duel_step(1, 0, actions, state, state_b, stack, stack_b, f, f.clone(), f.clone(), i, stack_out2=stack)
    # null pointers: past the Python wrapper, straight into the library
    lib, stream = _lib.load(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g, m, r = f.clone(), f.clone(), f.clone()
    rec = _lib.EnvRecords(g.data_ptr(), m.data_ptr(), r.data_ptr(), i.data_ptr(), None, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in ((None, p(state), p(state_b), None, p(stack), p(stack_b), None, ctypes.byref(rec)),           # actions
                 (p(actions), p(state), p(state_b), None, p(stack), p(stack_b), None, None),                  # records
                 (p(actions), p(state), None, None, p(stack), p(stack_b), None, ctypes.byref(rec))):          # state_out
        with pytest.raises(_lib.PaacHipError, match=r"\): paac_duel_step: "):
            _lib.check(lib.paac_duel_step(1, 0, 2, *args, stream), "paac_duel_step")
    with pytest.raises(ValueError):          # a catch record is no duel record
        hip_ops.duel_reset(1, 0, torch.zeros((2, hip_ops.CATCH_STATE_WORDS), dtype=torch.int32, device="cuda"), stack)
    torch.cuda.synchronize()
    assert not state_b.any() and not stack_b.any()          # nothing was launched


def make_args(*flags, **kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "duel"] + list(flags))
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


def pairs_hold(env_state):
    """record[b + HALF] == mirror(record[b]) in every slot of an env_state ring [slots, N, 12]."""
    half = env_state.shape[1] // 2
    for slot in env_state:
        for b_ in range(half):
            if tuple(slot[b_ + half][:10]) != duel.mirror(tuple(slot[b_][:10])):
                return False
    return True


def run_device_loop(flags, N, T, cycles, sampler, modes):
    from paac_amd.paac import DeviceRollout
    outs, records = [], []
    for mode in modes:
        learner = build_learner(make_args("-ec", str(N), "--max_local_steps", str(T), "--sampler", sampler, "--arch", "NIPS", *flags))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        assert learner._truncation_applies() == ("--bootstrap_truncated" in flags)          # duel has a step cap
        spec = learner.environment_creator.device_env_spec
        assert spec == dict(kind="duel", seed=3) and learner.num_actions == 6
        ro = DeviceRollout(learner, spec, sampler=sampler, use_graph=mode != "eager")
        assert ro.stateful and ro.route == "stateful" and tuple(ro.env_state.shape) == (2 * T + 1, N, 12) and ro.A == 6
        for _ in range(cycles):
            ro.run_cycle()
            if mode == "eager":
                ro.synchronize()
                records.append((ro.actions.cpu().numpy().copy(), ro.rewards.cpu().numpy().copy(), ro.masks.cpu().numpy().copy(),
                                ro.rollout_states().cpu().numpy().copy()))
        ro.synchronize()
        outs.append(dict(params=learner.network.get_parameters(), stacks=ro.states.cpu().numpy().copy(),
                         states=ro.env_state.cpu().numpy().copy(), actions=ro.actions.cpu().numpy().copy(),
                         rewards=ro.rewards.cpu().numpy().copy(), masks=ro.masks.cpu().numpy().copy(),
                         step=int(ro.global_step_dev.item()), finished=ro.finished_episodes(),
                         truncs=None if ro.truncs is None else ro.truncs.cpu().numpy().copy()))
        ro.close()
    return outs, records


@pytest.mark.parametrize("sampler,cycles", [("philox", 6), ("numpy", 2)])
def test_device_loop_replays_like_the_eager_run_and_through_the_twin(sampler, cycles):
    N, T = 4, 5
    outs, records = run_device_loop((), N, T, cycles, sampler, ("eager", "captured"))
    eager, captured = outs
    assert eager["step"] == captured["step"] == cycles * N * T and eager["truncs"] is None
    for k in ("stacks", "states", "actions", "rewards", "masks"):
        assert np.array_equal(eager[k], captured[k]), k
    for k, v in eager["params"].items():
        assert np.array_equal(v, captured["params"][k]) and np.isfinite(v).all(), k
    assert eager["finished"][0] == captured["finished"][0] and sorted(eager["finished"][1]) == sorted(captured["finished"][1])
    # the whole run through the twin on the recorded actions: every observation trained on, every reward and mask
    twin = DuelBoards(N, seed=3)
    _, obs = twin.reset()
    played = set()
    for c, (actions, rewards, masks, trained_on) in enumerate(records):
        played.update(actions.reshape(-1).tolist())
        for t in range(T):
            assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "cycle %d step %d" % (c, t)
            _, obs, want_rew, want_term, _ = twin.step(actions[t])
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], 1.0 - want_term.astype(np.float32)), (c, t)
    assert played <= set(range(6)) and len(played) >= 3, played
    last = (cycles & 1) * T          # the slot the next cycle starts from holds the twin's present
    assert np.array_equal(eager["stacks"][last], obs) and np.array_equal(eager["states"][last], twin.records())
    written = eager["states"] if cycles >= 2 else eager["states"][:T + 1]
    assert pairs_hold(written)


def test_device_loop_runs_under_the_update_options():
    """--ppo_epochs 2 --gae_lambda 0.95 --bootstrap_truncated true, two cycles: it runs, the plane exists, every value is finite
    and the pair invariant holds in every slot of the state ring."""
    N, T = 4, 5
    (out,), _ = run_device_loop(("--ppo_epochs", "2", "--gae_lambda", "0.95", "--bootstrap_truncated", "true"), N, T, 2, "philox",
                                ("captured",))
    assert out["step"] == 2 * N * T
    assert out["truncs"] is not None and out["truncs"].shape == (T, N) and not out["truncs"].any()      # no cap in ten steps
    for k, v in out["params"].items():
        assert np.isfinite(v).all(), k
    assert np.isfinite(out["rewards"]).all() and set(out["masks"].reshape(-1).tolist()) <= {0.0, 1.0}
    assert pairs_hold(out["states"])
    assert np.array_equal(out["rewards"][:, N // 2:], -out["rewards"][:, :N // 2])


def test_the_device_loop_refuses_an_odd_row_count():
    from paac_amd.paac import DeviceRollout
    learner = build_learner(make_args("-ec", "4", "--arch", "NIPS"))
    learner.global_step = learner.init_network()
    learner.emulator_counts = 3
    with pytest.raises(ValueError, match="emulator_counts"):
        DeviceRollout(learner, dict(kind="duel", seed=3))


def test_a_duel_run_is_evaluated_as_rally_against_the_script():
    """A DeviceEvaluator built the way --eval_every builds it for a duel learner returns, bit for bit, the scores and lengths of
    one built from dict(kind="rally", seed=same) on the same weights (count 8, greedy) -- and the `eval` record a real duel run
    writes carries those numbers and opponent: "scripted"."""
    from paac_amd import evaluation, hip_ops, paac
    N, T, cycles = 4, 5, 8
    args = make_args("-ec", str(N), "--max_local_steps", str(T), "--arch", "NIPS", "--eval_every", str(cycles * N * T),
                     "--eval_count", "8", max_global_steps=cycles * N * T)
    learner = build_learner(args)
    learner.train()
    records = [json.loads(line) for line in open(os.path.join(args.debugging_folder, "metrics.jsonl"))]
    evals = [r for r in records if r["kind"] == "eval"]
    assert [r["global_step"] for r in evals] == [cycles * N * T]
    assert evals[0]["opponent"] == "scripted" and evals[0]["count"] == 8 and evals[0]["greedy"] is True
    seed = int(args.random_seed) + 1
    derived = paac.eval_env_spec(learner.environment_creator.device_env_spec, seed=seed, single_life=False)
    assert derived == dict(kind="rally", seed=seed)
    ctx = hip_ops.Context(learner.network.arch_id, 6, max_batch=8)
    results = []
    for spec in (derived, dict(kind="rally", seed=seed)):
        ev = evaluation.DeviceEvaluator(learner.network, ctx, spec, 8, noops=30, greedy=True, seed=seed)
        assert ev.kind == "rally"
        results.append(ev.run())
        ev.close()
    ctx.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    scores, lengths = results[0]
    assert evals[0]["mean"] == float(np.mean(scores)) and evals[0]["mean_length"] == float(np.mean(lengths))
    assert -5.0 <= scores.min() and scores.max() <= 5.0 and lengths.min() >= 35 - 30 and lengths.max() <= rally.MAX_STEPS
