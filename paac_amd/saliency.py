"""Jacobian saliency of a trained agent (Wang et al., arXiv 1511.06581): which pixels move the value, or the chosen action?

  python -m paac_amd.saliency -f logs/ -o maps.npz -tc 8 --steps 64 --target value

Restores the latest checkpoint of a training folder as paac_amd.test does, plays -tc host environments with the sampled policy
(the loop of test.evaluate: every emulator works) and at every step takes the gradient of the target with respect to the
observation batch on the GPU (hip_ops.Context.input_gradient; include/paac_hip.h: paac_input_grad) -- the value V(s), or
log pi(a | s) of the action just chosen (--target action).  Environments whose episode ends start their next one.

OUT.npz holds, for S steps of N environments: observations uint8 [S, N, 84, 84, 4], gradients float32 [S, N, 84, 84, 4] (with
respect to observation * 1/255), actions int32 [S, N], probs float32 [S, N, A], values float32 [S, N].  Read per plane:
|gradients[..., p]| is the saliency of frame p of the history, the NEWEST frame in plane 3.
"""
import argparse
import os
import random
import time

import numpy as np

MAX_ROWS = 1024          # S * N of one file: 115 MB of gradients


def get_arg_parser():
    parser = argparse.ArgumentParser(description="Input-gradient saliency maps of the latest checkpoint of a training folder.")
    parser.add_argument("-f", "--folder", dest="folder", type=str, required=True, help="training folder: args.json and checkpoints/")
    parser.add_argument("-o", "--out", dest="out", type=str, required=True, help="the .npz file written")
    parser.add_argument("-tc", "--test_count", dest="test_count", type=int, default=8, help="environments N")
    parser.add_argument("--steps", dest="steps", type=int, default=64, help="steps S recorded")
    parser.add_argument("--target", dest="target", type=str, default="value", help="value: V(s); action: log pi(a | s) of the action chosen")
    parser.add_argument("-np", "--noops", dest="noops", type=int, default=30, help="upper bound of the random no-op steps before play")
    parser.add_argument("--eval_seed", dest="eval_seed", type=int, default=None, help="seed of the game instances (default: from the clock)")
    parser.add_argument("-d", "--device", dest="device", type=str, default="/gpu:0", help="'/gpu:N'")
    return parser


def check_flags(cli):
    """Start-up refusals (before anything touches the GPU)."""
    if cli.target not in ("value", "action"):
        raise ValueError("--target %r: expected value or action" % (cli.target,))
    if cli.test_count < 1 or cli.steps < 1:
        raise ValueError("-tc %d / --steps %d: expected positive counts" % (cli.test_count, cli.steps))
    if cli.test_count * cli.steps > MAX_ROWS:
        raise ValueError("-tc %d x --steps %d = %d observations: at most %d are recorded in one file (115 MB of gradients)"
                         % (cli.test_count, cli.steps, cli.test_count * cli.steps, MAX_ROWS))
    if cli.noops < 0:
        raise ValueError("noops %d is negative" % cli.noops)


def record(network, ctx, env_creator, session, test_count, steps, target, noops=30):
    """-> dict of the arrays of OUT.npz: `steps` steps of `test_count` host environments under the sampled policy."""
    import torch
    from .paac import PAACLearner
    environments = [env_creator.create_environment(i) for i in range(test_count)]
    states = np.stack([environment.get_initial_state() for environment in environments])
    for i, environment in enumerate(environments):
        for _ in range(random.randint(0, noops) if noops else 0):
            states[i] = environment.next(environment.get_noop())[0]
    A = env_creator.num_actions
    out = dict(observations=np.zeros((steps, test_count, 84, 84, 4), dtype=np.uint8),
               gradients=np.zeros((steps, test_count, 84, 84, 4), dtype=np.float32),
               actions=np.zeros((steps, test_count), dtype=np.int32), probs=np.zeros((steps, test_count, A), dtype=np.float32),
               values=np.zeros((steps, test_count), dtype=np.float32))
    for t in range(steps):
        actions, values, probs = PAACLearner.choose_next_actions(network, A, states, session)
        chosen = np.argmax(actions, axis=1).astype(np.int32)
        x = torch.from_numpy(np.ascontiguousarray(states, dtype=np.uint8)).to(network.torch_device)
        if target == "action":
            g = ctx.input_gradient(network.params, x, mode="logp_action", actions=torch.from_numpy(chosen).to(network.torch_device))
        else:
            g = ctx.input_gradient(network.params, x, mode="value")
        out["observations"][t], out["gradients"][t] = states, g.cpu().numpy()
        out["actions"][t], out["probs"][t], out["values"][t] = chosen, probs, np.reshape(values, -1)
        for j, environment in enumerate(environments):
            states[j], _, over = environment.next(actions[j])
            if over:
                states[j] = environment.get_initial_state()
    return out


def main(argv=None):
    cli = get_arg_parser().parse_args(argv)
    check_flags(cli)
    from . import hip_ops
    from .session import Session
    from .test import restore_settings
    from .train import get_network_and_environment_creator
    cli.gif_name, cli.sticky_action_p = None, None
    args = restore_settings(cli)
    seed = cli.eval_seed if cli.eval_seed is not None else int(np.random.RandomState(int(time.time())).randint(1000))
    random.seed(seed)
    np.random.seed(seed)
    network_creator, env_creator = get_network_and_environment_creator(args, random_seed=seed)
    network = network_creator()
    ctx = hip_ops.Context(network.arch_id, env_creator.num_actions, max_batch=cli.test_count,
                          device_index=network.torch_device.index or 0)
    session = Session(network, ctx)
    network.init(os.path.join(cli.folder, 'checkpoints'), network.make_saver(), session)
    try:
        arrays = record(network, ctx, env_creator, session, cli.test_count, cli.steps, cli.target, noops=cli.noops)
    finally:
        session.close()
        ctx.close()
    np.savez_compressed(cli.out, **arrays)
    print('Wrote {} steps of {} environments ({}) to {}'.format(cli.steps, cli.test_count, cli.target, cli.out))
    return arrays


if __name__ == '__main__':
    main()
