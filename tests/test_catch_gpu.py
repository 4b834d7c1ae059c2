"""-m gpu: the catch game on the device (paac_catch_reset / paac_catch_step, DeviceRollout with a kind == "catch" spec)
against its host twin paac_amd/catch.py -- and the one end-to-end check the parity tests cannot give: it learns."""
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from paac_amd import catch
from paac_amd.catch import CatchEnvironment

ONE_HOT = np.eye(3)
ACTION_CYCLE = (0, 1, 2, 2, 1)


def step_twins(twins, actions):
    """runners.step_emulators for a list of twins -> (observations, rewards, masks)."""
    obs, rewards, overs = [], [], []
    for env, a in zip(twins, actions):
        o, r, t = env.next(ONE_HOT[int(a)])
        if t:
            o = env.get_initial_state()
        obs.append(o)
        rewards.append(r)
        overs.append(t)
    return np.stack(obs), np.asarray(rewards, dtype=np.float32), 1.0 - np.asarray(overs, dtype=np.float32)


def drained(fin):
    """The device ring of finished episodes -> (count, sorted [(reward, length)])."""
    host = fin.cpu().numpy()
    count = int(host[0])
    assert count <= 4096
    return count, sorted(zip(host[2:2 + 4096].view(np.float32)[:count].tolist(), host[2 + 4096:2 + 4096 + count].tolist()))


@pytest.mark.parametrize("N,env_offset", [(3, 5), (33, 0), (1, 7)])
def test_kernel_matches_twin_bit_for_bit(N, env_offset):
    from paac_amd import hip_ops
    seed, steps, W = 3, 40, hip_ops.CATCH_STATE_WORDS
    dev = "cuda"
    stacks = [torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
    states = [torch.zeros((N, W), dtype=torch.int32, device=dev) for _ in range(2)]
    stack2 = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device=dev)
    state2 = torch.zeros((N, W), dtype=torch.int32, device=dev)
    actions = torch.zeros(N, dtype=torch.int32, device=dev)
    rew, msk, ep_r = (torch.zeros(N, device=dev) for _ in range(3))
    ep_l = torch.zeros(N, dtype=torch.int32, device=dev)
    fin = torch.zeros(hip_ops.FINISHED_RING_BYTES // 4, dtype=torch.int32, device=dev)
    twins = [CatchEnvironment(env_offset + e, seed=seed) for e in range(N)]
    want_obs = np.stack([env.get_initial_state() for env in twins])
    hip_ops.catch_reset(seed, env_offset, states[0], stacks[0])
    assert np.array_equal(stacks[0].cpu().numpy(), want_obs)
    assert np.array_equal(states[0].cpu().numpy(), np.stack([env.state_words() for env in twins]))
    want_ep_r, want_ep_l, want_fin = np.zeros(N, np.float32), np.zeros(N, np.int32), []
    for step in range(steps):
        a = np.array([ACTION_CYCLE[(step + e) % 5] for e in range(N)], dtype=np.int32)
        actions.copy_(torch.from_numpy(a))
        second = step == 7
        hip_ops.catch_step(seed, env_offset, actions, states[0], states[1], stacks[0], stacks[1], rew, msk, ep_r, ep_l, fin,
                           stack_out2=stack2 if second else None, state_out2=state2 if second else None)
        want_obs, want_rew, want_msk = step_twins(twins, a)
        want_ep_r += want_rew
        want_ep_l += 1
        for e in np.nonzero(want_msk == 0.0)[0]:
            want_fin.append((float(want_ep_r[e]), int(want_ep_l[e])))
            want_ep_r[e], want_ep_l[e] = 0.0, 0
        assert np.array_equal(stacks[1].cpu().numpy(), want_obs), "step %d: stacks" % step
        assert np.array_equal(states[1].cpu().numpy(), np.stack([env.state_words() for env in twins])), "step %d: states" % step
        assert np.array_equal(rew.cpu().numpy(), want_rew) and np.array_equal(msk.cpu().numpy(), want_msk), "step %d" % step
        assert np.array_equal(ep_r.cpu().numpy(), want_ep_r) and np.array_equal(ep_l.cpu().numpy(), want_ep_l), "step %d" % step
        assert drained(fin) == (len(want_fin), sorted(want_fin)), "step %d: finished ring" % step
        if second:
            assert torch.equal(stack2, stacks[1]) and torch.equal(state2, states[1])
        stacks.reverse()
        states.reverse()
    # three episodes per environment (a fourth where the first one lasted a single step), the short first one among them
    assert 3 * N <= len(want_fin) <= 4 * N and max(l for _, l in want_fin) == 13
    assert sorted(l for _, l in want_fin)[:N] == sorted(13 - catch.start_state(seed, env_offset + e, 0)[1] for e in range(N))


def test_step_in_place_and_bad_shapes_are_refused():
    from paac_amd import _lib, hip_ops
    N, W = 2, hip_ops.CATCH_STATE_WORDS
    stack = torch.zeros((N, 84, 84, 4), dtype=torch.uint8, device="cuda")
    stack_b = torch.zeros_like(stack)
    state = torch.zeros((N, W), dtype=torch.int32, device="cuda")
    state_b = torch.zeros_like(state)
    actions = torch.zeros(N, dtype=torch.int32, device="cuda")
    f, i = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    hip_ops.catch_reset(1, 0, state, stack)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.catch_step(1, 0, actions, state, state, stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(_lib.PaacHipError):
        hip_ops.catch_step(1, 0, actions, state, state_b, stack, stack, f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.catch_step(1, 0, actions, state, state_b[:, :4].contiguous(), stack, stack_b, f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.catch_step(1, 0, actions, state, state_b, stack, stack_b[:1], f, f.clone(), f.clone(), i)
    with pytest.raises(ValueError):
        hip_ops.catch_reset(1, 0, state_b[:1], stack)
    torch.cuda.synchronize()


def make_args(**kw):
    from paac_amd import train
    args = train.get_arg_parser().parse_args(["--emulator", "catch"])
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


def test_forward_with_three_actions_matches_the_oracle():
    """No other suite runs the heads at A = 3 (odd, below the smallest game's 4)."""
    from oracle import network as onet
    learner = build_learner(make_args(emulator_counts=5, max_local_steps=2))
    params = learner.network.get_parameters()
    states = np.random.RandomState(1).randint(0, 256, (5, 84, 84, 4)).astype(np.uint8)
    probs = torch.zeros((5, 3), device="cuda")
    values = torch.zeros(5, device="cuda")
    learner.ctx.forward(learner.network.params, torch.from_numpy(states).cuda(), probs=probs, values=values)
    want = onet.forward(params, states, "NIPS", dtype=np.float64)
    assert np.abs(probs.cpu().numpy() - want["pi"]).max() < 1e-5 and np.abs(values.cpu().numpy() - want["v"]).max() < 1e-4


@pytest.mark.parametrize("sampler", ["numpy", "philox"])
def test_device_loop_eager_captured_and_batched_agree_and_replay_through_the_twins(sampler):
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 7          # odd T: the ring's wrap-around slot is exercised
    outs, records = [], []
    for mode in ("eager", "captured", "batched"):
        learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler=sampler))
        np.random.seed(9)
        learner.global_step = learner.init_network()
        ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, sampler=sampler, use_graph=mode != "eager")
        assert ro.catch and tuple(ro.env_state.shape) == (2 * T + 1, N, 8)
        if mode == "batched":
            ro.run_cycles(cycles)           # 4 cycles in one graph launch, then 3 single ones
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
    # the whole run through the host twins on the recorded actions: every observation trained on, every reward and mask
    twins = [CatchEnvironment(e, seed=3) for e in range(N)]
    obs = np.stack([env.get_initial_state() for env in twins])
    episodes, totals, lengths = [], np.zeros(N), np.zeros(N, dtype=np.int64)
    for c, (actions, rewards, masks, trained_on) in enumerate(records):
        assert actions.min() >= 0 and actions.max() <= 2
        for t in range(T):
            assert np.array_equal(trained_on[t * N:(t + 1) * N], obs), "cycle %d step %d" % (c, t)
            obs, want_rew, want_msk = step_twins(twins, actions[t])
            assert np.array_equal(rewards[t], want_rew) and np.array_equal(masks[t], want_msk), "cycle %d step %d" % (c, t)
            totals += want_rew
            lengths += 1
            for e in np.nonzero(want_msk == 0.0)[0]:
                episodes.append((float(totals[e]), int(lengths[e])))
                totals[e], lengths[e] = 0.0, 0
    assert np.array_equal(outs[0]["rewards"], records[-1][1]) and np.array_equal(outs[0]["actions"], records[-1][0])
    # the slot the next cycle starts from holds the twins' present: observations and state records
    last = (cycles & 1) * T
    assert np.array_equal(outs[0]["stacks"][last], obs)
    assert np.array_equal(outs[0]["states"][last], np.stack([env.state_words() for env in twins]))
    assert len(episodes) >= N and outs[0]["finished"][0] == len(episodes)
    assert sorted(outs[0]["finished"][1]) == sorted(episodes)


LEARN_STEPS = 2 * 921600      # twice the smallest step count at which the default flags cleared the bar (DESIGN.md has the curve)


def test_it_learns():
    """The device loop with the default flags (NIPS trunk, RMSProp, lr 0.0224, 32 environments, t_max 5), weights seeded, philox
    sampler: the mean return of the last 1000 finished episodes must exceed -0.5.  The uniform random policy scores -0.86 and
    a 1000-episode mean has a standard error of about 0.016, so the bar is more than twenty standard errors above chance.
    Measured on the MI355X: first above the bar at 921,600 steps (checked every 20,480); the test trains twice as long."""
    from paac_amd.paac import DeviceRollout
    N, T = 32, 5
    learner = build_learner(make_args(emulator_counts=N, max_local_steps=T, arch="NIPS"))
    learner.global_step = learner.init_network()
    ro = DeviceRollout(learner, learner.environment_creator.device_env_spec, sampler="philox", sampler_seed=42, use_graph=True)
    ro.run_cycles(LEARN_STEPS // (N * T))
    ro.synchronize()
    count, episodes = ro.finished_episodes()
    assert int(ro.global_step_dev.item()) == LEARN_STEPS and count > 100000 and len(episodes) == 4096
    mean = float(np.mean([r for r, _ in episodes[-1000:]]))
    print("catch after %d steps: mean return of the last 1000 of %d episodes %+.3f" % (LEARN_STEPS, count, mean))
    ro.close()
    assert mean > -0.5


def test_host_plugin_loop_matches_device_loop():
    """The host loop stepping CatchEnvironment plugins == the device loop on the same np.random sampler stream."""
    from paac_amd.paac import DeviceRollout
    N, T, cycles = 4, 5, 3
    feeds = []
    host = build_learner(make_args(emulator_counts=N, max_local_steps=T, max_global_steps=cycles * N * T, sampler="numpy",
                                   host_environments=True, record_feeds=True, feed_callback=feeds.append))
    np.random.seed(7)
    host.train()
    assert len(feeds) == cycles
    devl = build_learner(make_args(emulator_counts=N, max_local_steps=T, sampler="numpy"))
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
