"""-m gpu: --sticky_action_p on the device (paac_game_step_sticky / paac_duel_step_sticky / paac_eval_step_sticky, DeviceRollout
with a prev ring, DeviceEvaluator(sticky_p=...)) against its specification paac_amd/sticky.py: the wrapped host twins and, for
duel, DuelBoards with sticky.apply on both players.  Everything here is bit for bit.  The CPU side is tests/test_sticky.py."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import sticky_checks as checks
from paac_amd import bricks, catch, evaluation, rally, sticky
from paac_amd.duel import DuelBoards
from paac_amd.sticky import EVAL_STREAM_STICKY, STICKY_STREAM, StickyEnvironment

SEED, P = checks.SEED, checks.P
TWINS = {"catch": (catch.CatchEnvironment, 3), "bricks": (bricks.BricksEnvironment, 3), "rally": (rally.RallyEnvironment, 6)}


# ---- 1. the step entries against wrapped twins ------------------------------------------------------------------------------------
def game_case(kind, N, env_offset, steps, **option):
    from paac_amd import hip_ops
    import functools
    twin, num_actions = TWINS[kind]
    return checks.game_against_wrapped_twins(kind, lambda g: twin(g, seed=SEED, **option), num_actions, N, env_offset, steps,
                                             functools.partial(hip_ops.game_reset, kind), hip_ops.DEVICE_GAMES[kind]["words"],
                                             **option)


@pytest.mark.parametrize("kind", ["catch", "bricks", "rally"])
def test_step_entry_matches_wrapped_twins_bit_for_bit(kind):
    """N = 3, env_offset 5, 120 steps of hashed actions: 87 of the 360 draws stick (tests/test_sticky.py counts them); a step
    shows it only where the previous action differs from the chosen one."""
    stuck, terminals = game_case(kind, 3, 5, 120)
    print("%s: %d of 360 steps executed another action than the chosen one, %d terminal steps" % (kind, stuck, terminals))
    # (catch: 120 steps of episodes of at most 13 -- the plane is cleared behind at least 27 terminal steps)
    assert 20 <= stuck <= 87 and terminals >= (27 if kind == "catch" else 0)


@pytest.mark.parametrize("kind", ["catch", "bricks", "rally"])
def test_step_entry_matches_wrapped_twins_past_one_tile(kind):
    stuck, _ = game_case(kind, 33, 0, 40)
    assert stuck >= 100


def test_bricks_single_life_under_sticky_actions():
    stuck, terminals = game_case("bricks", 3, 5, 120, single_life=True)
    assert stuck >= 20 and terminals >= 3


def test_duel_step_matches_duel_boards_with_apply_on_both_players():
    from paac_amd import hip_ops
    N, env_offset, steps = 6, 5, 150
    b = checks.StepBuffers(N, hip_ops.DUEL_STATE_WORDS)
    boards = DuelBoards(N, SEED, env_offset)
    want_records, want_stacks = boards.reset()
    hip_ops.duel_reset(SEED, env_offset, b.states[0], b.stacks[0])
    assert np.array_equal(b.states[0].cpu().numpy(), want_records) and np.array_equal(b.stacks[0].cpu().numpy(), want_stacks)
    chosen = checks.hashed_actions(steps, N, 6)
    prev = np.zeros(N, dtype=np.int32)
    differs = independent = terminals = 0
    for t in range(steps):
        second = t % 5 == 4
        offset = checks.set_step(b, t, chosen[t])
        hip_ops.duel_step_sticky(P, b.tick, offset, b.prev[0], b.prev[1], SEED, env_offset, b.actions, b.states[0], b.states[1],
                                 b.stacks[0], b.stacks[1], *b.records(), truncs_out=b.truncs, state_out2=b.state2 if second else None,
                                 stack_out2=b.stack2 if second else None, prev_out2=b.prev2 if second else None)
        stuck = sticky.sticks(P, SEED, t, env_offset + np.arange(N), STICKY_STREAM)          # keyed per ROW
        independent += int((stuck[:N // 2] != stuck[N // 2:]).sum())
        executed, prev = sticky.apply(chosen[t], prev, t, env_offset + np.arange(N), P, SEED, STICKY_STREAM)
        differs += int((executed != chosen[t]).sum())
        want_records, want_stacks, rewards, terms, truncs = boards.step(executed)
        prev[terms] = 0
        terminals += int(terms.sum())
        got = b.outputs()
        assert np.array_equal(got["states"], want_records), "step %d: states" % t
        assert np.array_equal(got["stacks"], want_stacks), "step %d: stacks" % t
        assert np.array_equal(got["rewards"], rewards) and np.array_equal(got["masks"], 1.0 - terms.astype(np.float32)), "step %d" % t
        assert np.array_equal(got["truncs"], truncs.astype(np.float32)) and np.array_equal(got["prev"], prev), "step %d" % t
        if second:
            assert torch.equal(b.prev2, b.prev[1]) and torch.equal(b.state2, b.states[1]) and torch.equal(b.stack2, b.stacks[1])
        b.flip()
    print("duel: %d of %d row steps executed another action, the two players of a board drew differently %d times, %d terminal "
          "row steps" % (differs, steps * N, independent, terminals))
    assert differs >= 100 and independent >= 50


# ---- 2. p = 0 is the plain entry; the refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bricks", "duel"])
def test_p_zero_gives_the_plain_entrys_outputs_byte_for_byte(kind):
    from paac_amd import hip_ops
    N, env_offset, steps = 6, 5, 20
    words = 12
    plain, stuck = checks.StepBuffers(N, words), checks.StepBuffers(N, words)
    num_actions = 6 if kind == "duel" else 3
    chosen = checks.hashed_actions(steps, N, num_actions)
    for b in (plain, stuck):
        (hip_ops.duel_reset if kind == "duel" else hip_ops.bricks_reset)(SEED, env_offset, b.states[0], b.stacks[0])
    stuck.prev[0].fill_(2)                                     # whatever the plane holds: nothing sticks at p = 0
    for t in range(steps):
        for b in (plain, stuck):
            offset = checks.set_step(b, t, chosen[t])
        if kind == "duel":
            hip_ops.duel_step(SEED, env_offset, plain.actions, plain.states[0], plain.states[1], plain.stacks[0], plain.stacks[1],
                              *plain.records(), truncs_out=plain.truncs, stack_out2=plain.stack2, state_out2=plain.state2)
            hip_ops.duel_step_sticky(0.0, stuck.tick, offset, stuck.prev[0], stuck.prev[1], SEED, env_offset, stuck.actions,
                                     stuck.states[0], stuck.states[1], stuck.stacks[0], stuck.stacks[1], *stuck.records(),
                                     truncs_out=stuck.truncs, stack_out2=stuck.stack2, state_out2=stuck.state2, prev_out2=stuck.prev2)
        else:
            hip_ops.game_step_records(kind, SEED, env_offset, plain.actions, plain.states[0], plain.states[1], plain.stacks[0],
                                      plain.stacks[1], *plain.records(), truncs_out=plain.truncs, stack_out2=plain.stack2,
                                      state_out2=plain.state2)
            hip_ops.game_step_sticky(kind, 0.0, stuck.tick, offset, stuck.prev[0], stuck.prev[1], SEED, env_offset, stuck.actions,
                                     stuck.states[0], stuck.states[1], stuck.stacks[0], stuck.stacks[1], *stuck.records(),
                                     truncs_out=stuck.truncs, stack_out2=stuck.stack2, state_out2=stuck.state2, prev_out2=stuck.prev2)
        want, got = plain.outputs(), stuck.outputs()
        for key in want:
            if key != "prev":
                assert want[key].tobytes() == got[key].tobytes(), "step %d: %s" % (t, key)
        assert torch.equal(stuck.stack2, plain.stack2) and torch.equal(stuck.state2, plain.state2)
        # the plane holds the chosen action (0 behind a terminal step), and the second copy is the first
        assert np.array_equal(got["prev"], np.where(got["masks"] == 0.0, 0, chosen[t])) and torch.equal(stuck.prev2, stuck.prev[1])
        plain.flip()
        stuck.flip()


def test_p_zero_evaluation_step_is_the_plain_one():
    from paac_amd import hip_ops
    N, A, steps = 5, 6, 20
    rs = np.random.RandomState(2)
    probs = torch.from_numpy(rs.dirichlet(np.ones(A), size=(steps, N)).astype(np.float32)).cuda()
    outs = []
    for form in ("plain", "sticky"):
        b = checks.StepBuffers(N, 12)
        hip_ops.rally_reset(SEED, 4, b.states[0], b.stacks[0])
        score, length, done = b.rew, b.ep_l, torch.zeros(N, dtype=torch.int32, device="cuda")
        alive = torch.full((1,), N, dtype=torch.int32, device="cuda")
        trace = []
        for t in range(steps):
            args = (probs[t], False, 11, 2, b.tick, t, SEED, 4, b.states[0], b.states[1], b.stacks[0], b.stacks[1], b.actions, score,
                    length, done, alive)
            if form == "plain":
                hip_ops.eval_step("rally", *args)
            else:
                hip_ops.eval_step_sticky("rally", 0.0, b.prev[0], b.prev[1], *args)
            trace.append(b.actions.cpu().numpy().copy())
            b.flip()
        outs.append([b.states[0].cpu().numpy(), b.stacks[0].cpu().numpy(), np.array(trace), score.cpu().numpy(),
                     length.cpu().numpy(), done.cpu().numpy(), alive.cpu().numpy()])
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()


def test_every_refusal_comes_back_as_an_error_without_a_launch():
    cases = checks.check_refusals()
    assert cases >= 40
    torch.cuda.synchronize()
    # ... and through the wrappers: the library's refusal is a PaacHipError
    from paac_amd import _lib, hip_ops
    b = checks.StepBuffers(2, 12)
    hip_ops.bricks_reset(SEED, 0, b.states[0], b.stacks[0])
    for p, prev_out in ((1.0, b.prev[1]), (float("nan"), b.prev[1]), (0.25, b.prev[0])):
        with pytest.raises(_lib.PaacHipError):
            hip_ops.game_step_sticky("bricks", p, b.tick, 0, b.prev[0], prev_out, SEED, 0, b.actions, b.states[0], b.states[1],
                                     b.stacks[0], b.stacks[1], *b.records())
    with pytest.raises(ValueError):          # a plane of another shape
        hip_ops.game_step_sticky("bricks", 0.25, b.tick, 0, b.prev[0][:1], b.prev[1], SEED, 0, b.actions, b.states[0], b.states[1],
                                 b.stacks[0], b.stacks[1], *b.records())
    torch.cuda.synchronize()


# ---- 3. evaluation --------------------------------------------------------------------------------------------------------------
EVAL_SEED = (0x5EED << 32) + 11


def game_args(game, *flags, **kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", game, "--arch", "NIPS"] + list(flags))
    args.debugging_folder = tempfile.mkdtemp(prefix="paac_stickytest_")
    args.emulator_workers = 0
    args.max_global_steps = 1 << 40
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def fresh_network(args):
    from paac_amd import train
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    network = network_creator()
    network.initialize(np.random.RandomState(0))
    return network, env_creator


@pytest.mark.parametrize("game", ["catch", "rally"])
def test_evaluator_with_sticky_actions_replays_on_wrapped_twins(game):
    from paac_amd import hip_ops
    network, env_creator = fresh_network(game_args(game, "--sticky_action_p", str(P)))
    spec = env_creator.device_env_spec
    ctx = hip_ops.Context(network.arch_id, env_creator.num_actions, max_batch=8)
    env_creator.sticky_stream, env_creator.sticky_seed = EVAL_STREAM_STICKY, EVAL_SEED          # the evaluation's key
    assert isinstance(env_creator.create_environment(0), StickyEnvironment)
    plain_creator = fresh_network(game_args(game))[1]
    for greedy in (True, False):
        ev = evaluation.DeviceEvaluator(network, ctx, spec, count=5, noops=4, greedy=greedy, record=True, seed=EVAL_SEED, sticky_p=P)
        scores, lengths, trace, noops_e = ev.run()
        assert ev.summary(scores, lengths, 0.0)["sticky_action_p"] == P
        ev.close()
        want = evaluation.replay_on_twins(env_creator, trace, noops_e)
        assert np.array_equal(scores, want[0]) and np.array_equal(lengths, want[1])
        # sticky_p = 0: the numbers of the evaluator as it was, by the entry as it was
        zero = evaluation.DeviceEvaluator(network, ctx, spec, count=5, noops=4, greedy=greedy, record=True, seed=EVAL_SEED, sticky_p=0.0)
        was = evaluation.DeviceEvaluator(network, ctx, spec, count=5, noops=4, greedy=greedy, record=True, seed=EVAL_SEED)
        a, b = zero.run(), was.run()
        assert zero.prev is None and "sticky_action_p" not in zero.summary(a[0], a[1], 0.0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        want = evaluation.replay_on_twins(plain_creator, a[2], a[3])
        assert np.array_equal(a[0], want[0]) and np.array_equal(a[1], want[1])
        zero.close()
        was.close()
        print("%s, %s: sticky scores %s lengths %s; plain scores %s lengths %s" % (game, "greedy" if greedy else "sampled",
                                                                                  scores, lengths, a[0], a[1]))
    # the captured blocks give the eager run's numbers (the plane ping-pongs inside a block)
    ev = evaluation.DeviceEvaluator(network, ctx, spec, count=5, noops=4, greedy=False, seed=EVAL_SEED, sticky_p=P, steps_per_launch=4)
    first, second = ev.run(), ev.run()
    assert ev.use_graph and np.array_equal(first[0], scores) and np.array_equal(first[1], lengths)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    ev.close()
    ctx.close()


# ---- 4. the device loop ------------------------------------------------------------------------------------------------------------
def build_learner(args, params_seed=0):
    from paac_amd import train
    from paac_amd.paac import PAACLearner
    network_creator, env_creator = train.get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    learner.network.initialize(np.random.RandomState(params_seed))
    learner.network.init = lambda folder, saver, session: 0      # keep the seeded weights
    return learner


def device_run(args, sampler, use_graph, cycles, keep_records=False):
    from paac_amd.paac import DeviceRollout
    learner = build_learner(args)
    np.random.seed(9)
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, sampler=sampler, use_graph=use_graph)
    records = []
    for _ in range(cycles):
        ro.run_cycle()
        if keep_records:
            ro.synchronize()
            records.append((ro.actions.cpu().numpy().copy(), ro.rewards.cpu().numpy().copy(), ro.masks.cpu().numpy().copy()))
    ro.synchronize()
    out = dict(params=learner.network.get_parameters(), stacks=ro.states.cpu().numpy().copy(), states=ro.env_state.cpu().numpy().copy(),
               actions=ro.actions.cpu().numpy().copy(), rewards=ro.rewards.cpu().numpy().copy(), masks=ro.masks.cpu().numpy().copy(),
               prev=None if ro.prev is None else ro.prev.cpu().numpy().copy(), finished=ro.finished_episodes())
    ro.close()
    return out, records


def same_run(a, b):
    for k in ("stacks", "states", "actions", "rewards", "masks"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["prev"] is None) == (b["prev"] is None) and (a["prev"] is None or np.array_equal(a["prev"], b["prev"]))
    for k, v in a["params"].items():
        assert np.array_equal(v, b["params"][k]), k
    assert a["finished"][0] == b["finished"][0] and sorted(a["finished"][1]) == sorted(b["finished"][1])


@pytest.mark.parametrize("game,sampler", [("bricks", "numpy"), ("duel", "philox")])
def test_device_loop_eager_and_replayed_agree_and_replay_through_the_twins(game, sampler):
    N, T, cycles = 4, 5, 4          # four cycles: the ring's wrap slot is crossed twice
    flags = ["--sticky_action_p", str(P)]
    eager, records = device_run(game_args(game, *flags, emulator_counts=N, max_local_steps=T, sampler=sampler), sampler, False,
                                cycles, keep_records=True)
    replayed, _ = device_run(game_args(game, *flags, emulator_counts=N, max_local_steps=T, sampler=sampler), sampler, True, cycles)
    assert tuple(eager["prev"].shape) == (2 * T + 1, N)
    same_run(eager, replayed)
    # the recorded CHOSEN actions through the spec: wrapped twins, or DuelBoards with apply on every row
    differs = 0
    if game == "duel":
        boards = DuelBoards(N, SEED, 0)
        boards.reset()
        prev = np.zeros(N, dtype=np.int32)
    else:
        twins = [StickyEnvironment(bricks.BricksEnvironment(e, seed=SEED), P, SEED, e) for e in range(N)]
        for env in twins:
            env.get_initial_state()
    for c, (actions, rewards, masks) in enumerate(records):
        for t in range(T):
            step = c * T + t
            if game == "duel":
                executed, prev = sticky.apply(actions[t], prev, step, np.arange(N), P, SEED, STICKY_STREAM)
                _, _, want_rew, terms, _ = boards.step(executed)
                prev[terms] = 0
                want_msk = 1.0 - terms.astype(np.float32)
                differs += int((executed != actions[t]).sum())
            else:
                want_rew, want_msk = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
                for e, env in enumerate(twins):
                    _, want_rew[e], over = env.next(np.eye(3)[actions[t, e]])
                    differs += env.last_executed != actions[t, e]
                    want_msk[e] = 0.0 if over else 1.0
                    if over:
                        env.get_initial_state()
                prev = np.array([env.prev for env in twins], dtype=np.int32)
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], want_msk), "cycle %d step %d" % (c, t)
    # the slot the next cycle starts from holds the spec's present: the previous actions (and, for bricks, the records)
    last = (cycles & 1) * T
    assert np.array_equal(eager["prev"][last], prev)
    if game != "duel":
        assert np.array_equal(eager["states"][last], np.stack([env.state_words() for env in twins]))
    print("%s, %s sampler: %d of %d steps executed another action than the chosen one" % (game, sampler, differs, cycles * T * N))
    assert differs >= 5


def test_p_zero_is_weight_identical_to_a_run_without_the_flag():
    N, T, cycles = 4, 5, 4
    without, _ = device_run(game_args("bricks", emulator_counts=N, max_local_steps=T), "philox", True, cycles)
    zero, _ = device_run(game_args("bricks", "--sticky_action_p", "0.0", emulator_counts=N, max_local_steps=T), "philox", True, cycles)
    assert without["prev"] is None and zero["prev"] is None
    same_run(without, zero)
    stuck, _ = device_run(game_args("bricks", "--sticky_action_p", str(P), emulator_counts=N, max_local_steps=T), "philox", True,
                          cycles)
    assert not np.array_equal(stuck["states"], without["states"])          # ... and the flag does something


# ---- 5. the host loop against the device loop -------------------------------------------------------------------------------------
def test_host_loop_matches_device_loop_record_for_record():
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 3
    flags = ["--sticky_action_p", str(P)]
    feeds = []
    host = build_learner(game_args("catch", *flags, emulator_counts=N, max_local_steps=T, max_global_steps=cycles * N * T,
                                   sampler="numpy", host_environments=True, record_feeds=True, feed_callback=feeds.append))
    assert all(isinstance(env, StickyEnvironment) for env in host.emulators)
    np.random.seed(7)
    host.train()
    assert len(feeds) == cycles
    devl = build_learner(game_args("catch", *flags, emulator_counts=N, max_local_steps=T, sampler="numpy"))
    np.random.seed(7)
    devl.global_step = devl.init_network()
    ro = DeviceRollout(devl, devl.environment_creator.device_env_spec, sampler="numpy", use_graph=True)
    assert ro.prev is not None and ro.sticky_p == P
    for c in range(cycles):
        ro.run_cycle()
        ro.synchronize()
        assert np.array_equal(ro.rollout_states().cpu().numpy(), feeds[c]["states"]), "cycle %d" % c
        assert np.array_equal(ro.actions.view(-1).cpu().numpy(), feeds[c]["actions"]), "cycle %d" % c
        assert np.array_equal(ro.rewards.cpu().numpy(), feeds[c]["rewards"]), "cycle %d" % c
        assert np.array_equal(ro.masks.cpu().numpy(), feeds[c]["masks"]), "cycle %d" % c
    ro.close()
    # (what the run was asked: draws that stick are among its 60)
    stuck = sum(int(sticky.sticks(P, SEED, t, np.arange(N), STICKY_STREAM).sum()) for t in range(cycles * T))
    print("host loop: %d of %d draws stuck" % (stuck, cycles * T * N))
    assert stuck >= 5


# ---- 6. a user's game -----------------------------------------------------------------------------------------------------------------
def test_user_game_sticky_step_matches_the_wrapped_twin():
    """examples/patrol through --device_game, N = 3, 60 steps, in a child process: a process holds one kernel library."""
    res = subprocess.run([sys.executable, os.path.join(checks.ROOT, "tests", "sticky_checks.py"), "patrol"], cwd=checks.ROOT,
                         capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:])
    print(res.stderr[-3000:], file=sys.stderr)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("CHECK_OK"), (res.stdout[-2000:], res.stderr[-4000:])
