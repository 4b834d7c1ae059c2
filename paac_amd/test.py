"""Evaluation harness (the role of reference test.py:22-88): restore the latest network checkpoint of a training
folder, play `test_count` environments with the sampled policy (PAACLearner.choose_next_actions) after up to `noops`
random no-op steps, print mean / min / max / std of the episode scores.

  python -m paac_amd.test -f logs/ -tc 30 -np 30

Flags as upstream (-f, -tc, -np, -gn, -gf, -d).  One deliberate difference: the reference's loop
(`while not all(episodes_over)`, test.py:77-83) overwrites every environment's flag each step, so with test_count > 1
it only stops when all environments happen to finish on the same step and keeps adding post-episode rewards; here an
environment's score is frozen when its first episode ends.

--device_environments true (runs of --emulator catch|bricks|rally, and duel runs as rally) plays the games on the GPU instead
(paac_amd/evaluation.py: DeviceEvaluator): -tc up to 4096, --greedy true for the argmax action, --eval_seed for the game instances, the no-op counts
and the sampled actions; the summary gains a 'Mean length' line.  --gif_name is refused there.

--versus FOLDER_B (with --device_environments true; runs of --emulator rally|duel) plays -tc duel boards between the two folders'
checkpoints instead (paac_amd/match.py: DeviceMatch), -f's agent being player X: the summary is of its scores and gains a
'Wins / Draws / Losses' line.
"""
import argparse
import os
import random
import time

import numpy as np

from . import hip_ops, logger_utils, sticky
from .paac import PAACLearner, eval_env_spec
from .session import Session
from .train import bool_arg, get_network_and_environment_creator

# (option strings, dest, default, type, required, help) -- names and defaults are upstream's (test.py:22-30)
FLAGS = (
    (("-f", "--folder"), "folder", None, str, True, "training folder: holds args.json and checkpoints/"),
    (("-tc", "--test_count"), "test_count", 1, int, False, "number of environments, one scored episode each"),
    (("-np", "--noops"), "noops", 30, int, False, "upper bound of the random number of no-op steps before play"),
    (("-gn", "--gif_name"), "gif_name", None, str, False, "record every screen of environment i into <name><i>.gif"),
    (("-gf", "--gif_folder"), "gif_folder", "", str, False, "directory the gifs are written to"),
    (("-d", "--device"), "device", "/gpu:0", str, False, "'/gpu:N': which MI355X evaluates the policy"),
    (("--device_environments",), "device_environments", False, bool_arg, False,
     "play the games on the GPU (paac_amd/evaluation.py; --emulator catch|bricks|rally runs only): -tc up to 4096, no gifs"),
    (("--greedy",), "greedy", False, bool_arg, False,
     "with --device_environments true: the argmax action instead of a sampled one"),
    (("--eval_seed",), "eval_seed", None, int, False,
     "with --device_environments true: seed of the game instances, the no-op counts and the sampled actions (default: the "
     "training run's random_seed)"),
    (("--versus",), "versus", None, str, False,
     "with --device_environments true: a second training folder; -tc duel boards are played between the two checkpoints "
     "(paac_amd/match.py; --emulator rally|duel runs only), -f's agent on the bottom of the first half of the boards and on the "
     "top of the rest"),
    (("--sticky_action_p",), "sticky_action_p", None, float, False,
     "sticky actions during the evaluation (paac_amd/sticky.py; runs of --emulator catch|bricks|rally|duel|user, host loop and "
     "--device_environments true; --emulator ale: ALE's repeat_action_probability): P in [0, 1), default the training run's "
     "own value from args.json (0 for a run from before the flag); 0 gives the numbers of a plain evaluation; refused with "
     "--versus"),
)


def get_arg_parser():
    parser = argparse.ArgumentParser(description="Score the latest checkpoint of a training folder.")
    for options, dest, default, kind, required, text in FLAGS:
        parser.add_argument(*options, dest=dest, default=default, type=kind, required=required, help=text)
    return parser


class GifRecorder(object):
    """on_new_frame hook (environment.py:34-39): appends every screen an environment shows to one gif (30 fps)."""

    def __init__(self, path):
        try:
            import imageio
        except ImportError:
            raise ImportError("--gif_name needs the imageio package")
        self.writer = imageio.get_writer(path + '.gif', fps=30)

    def __call__(self, frame):
        self.writer.append_data(frame)


def get_save_frame(name):
    """Upstream's name for the hook factory (test.py:12-20)."""
    return GifRecorder(name)


def evaluate(network, env_creator, session, test_count, noops=30, max_steps=None, on_new_frame=None):
    """-> float32 [test_count]: score of the FIRST episode of each environment under the sampled policy."""
    environments = [env_creator.create_environment(i) for i in range(test_count)]
    if on_new_frame is not None:
        for i, environment in enumerate(environments):
            environment.on_new_frame = on_new_frame(i)
    states = np.stack([environment.get_initial_state() for environment in environments])
    for i, environment in enumerate(environments):          # random start: 0..noops no-op steps (test.py:69-73)
        for _ in range(random.randint(0, noops) if noops else 0):
            states[i] = environment.next(environment.get_noop())[0]
    scores = np.zeros(test_count, dtype=np.float32)
    playing = list(range(test_count))
    steps = 0
    while playing and (max_steps is None or steps < max_steps):
        actions, _, _ = PAACLearner.choose_next_actions(network, env_creator.num_actions, states, session)
        still = []
        for j in playing:
            states[j], reward, over = environments[j].next(actions[j])
            scores[j] += reward
            if not over:
                still.append(j)
        playing = still
        steps += 1
    return scores


def restore_settings(cli, folder=None):
    """The training run's args.json (of cli.folder, or of `folder`) with the evaluation overrides of test.py:32-48 applied on
    top."""
    settings = argparse.Namespace(**vars(cli))
    for k, v in logger_utils.load_args(os.path.join(folder or cli.folder, 'args.json')).items():
        setattr(settings, k, v)
    overrides = dict(device=cli.device, debugging_folder='/tmp/logs', max_global_steps=0, random_start=False,
                     single_life_episodes=False, actor_id=0)
    if cli.gif_name:
        overrides["visualize"] = 1
    if getattr(cli, "sticky_action_p", None) is not None:          # given by hand: instead of the training run's
        overrides["sticky_action_p"] = cli.sticky_action_p
    for k, v in overrides.items():
        setattr(settings, k, v)
    return settings


def check_device_flags(cli):
    """Start-up refusals of --device_environments true (before anything touches the GPU)."""
    from . import evaluation
    if cli.gif_name:
        raise ValueError("--gif_name cannot be combined with --device_environments true: the games run on the GPU and there "
                         "are no host screens to record")
    evaluation.check_count(cli.test_count, "test_count")
    if cli.noops < 0:
        raise ValueError("noops %d is negative" % cli.noops)


def evaluate_on_device(cli, args):
    """--device_environments true: the DeviceEvaluator (paac_amd/evaluation.py) in the place of evaluate() ->
    (scores float32 [test_count], lengths int32 [test_count])."""
    from . import evaluation
    seed = cli.eval_seed if cli.eval_seed is not None else int(getattr(args, "random_seed", 3))
    network_creator, env_creator = get_network_and_environment_creator(args, random_seed=seed)
    spec = eval_env_spec(getattr(env_creator, "device_env_spec", None))     # a duel run is scored on rally
    evaluation.check_env_spec(spec)
    p = sticky.check_flags(args)
    network = network_creator()
    ctx = hip_ops.Context(network.arch_id, env_creator.num_actions, max_batch=min(cli.test_count, evaluation.MAX_CHUNK),
                          device_index=network.torch_device.index or 0)
    session = Session(network, ctx)
    network.init(os.path.join(cli.folder, 'checkpoints'), network.make_saver(), session)
    evaluator = evaluation.DeviceEvaluator(network, ctx, spec, cli.test_count, noops=cli.noops, greedy=cli.greedy, seed=seed,
                                           sticky_p=p)
    try:
        return evaluator.run()
    finally:
        evaluator.close()
        session.close()
        ctx.close()


def check_versus_flags(cli):
    """Start-up refusals of --versus (before anything touches the GPU)."""
    if not cli.device_environments:
        raise ValueError("--versus plays its boards on the GPU: it needs --device_environments true")
    if cli.gif_name:
        raise ValueError("--versus cannot be combined with --gif_name: the boards are on the GPU and there are no host screens "
                         "to record")
    check_device_flags(cli)


def check_versus_runs(runs):
    """runs: [(folder, restored settings)] of the two players -> a ValueError naming the folder that cannot play a match."""
    from . import match
    from .build import parse_user_arch
    user = []
    for folder, args in runs:
        if getattr(args, "emulator", "synthetic") not in match.MATCH_KINDS:
            raise ValueError("--versus: %s is a run of --emulator %s; a match is played by agents of the duel board: --emulator "
                             "rally|duel" % (folder, getattr(args, "emulator", "synthetic")))
        if getattr(args, "user_arch", ""):
            user.append((folder, parse_user_arch(args.user_arch)))
    if len(user) == 2 and user[0][1] != user[1][1]:
        raise ValueError("--versus: %s was trained with --user_arch %s and %s with another one: a process loads ONE kernel "
                         "library, which serves one user architecture beside NIPS and NATURE"
                         % (user[1][0], runs[1][1].user_arch, user[0][0]))


def match_on_device(cli):
    """--versus: a DeviceMatch (paac_amd/match.py) between the checkpoints of cli.folder (X) and cli.versus (Y) ->
    (X's scores float32 [test_count], lengths int32 [test_count], the summary's fields)."""
    from . import evaluation, match
    runs = [(folder, restore_settings(cli, folder)) for folder in (cli.folder, cli.versus)]
    check_versus_runs(runs)
    for _, args in runs:
        sticky.check_flags(args, versus=cli.versus)          # a match has no sticky form: refused, whichever run asks for it
    seed = cli.eval_seed if cli.eval_seed is not None else int(getattr(runs[0][1], "random_seed", 3))
    # both creators before the first network: a user architecture chooses the library the process loads
    creators = [get_network_and_environment_creator(args, random_seed=seed) for _, args in runs]
    players, opened = [], []
    try:
        for (folder, _), (network_creator, env_creator) in zip(runs, creators):
            network = network_creator()
            ctx = hip_ops.Context(network.arch_id, env_creator.num_actions, max_batch=min(cli.test_count, evaluation.MAX_CHUNK),
                                  device_index=network.torch_device.index or 0)
            opened.append(ctx)
            session = Session(network, ctx)
            opened.append(session)
            network.init(os.path.join(folder, 'checkpoints'), network.make_saver(), session)
            players += [network.params, ctx]
        game = match.DeviceMatch(*players, count=cli.test_count, noops=cli.noops, greedy=cli.greedy, seed=seed, game_seed=seed)
        opened.append(game)
        scores, lengths, seconds = game.timed_run()
        return scores, lengths, game.summary(scores, lengths, seconds)
    finally:
        for x in reversed(opened):
            x.close()


def print_match_summary(cli, record):
    print('Performed {} matches: {} vs {}'.format(cli.test_count, cli.folder, cli.versus))
    for label, key in (('Mean', 'mean'), ('Min', 'min'), ('Max', 'max'), ('Std', 'std')):
        print('{0}: {1:.2f}'.format(label, record[key]))
    print('Wins / Draws / Losses: {0:.3f} / {1:.3f} / {2:.3f}'.format(record['wins'], record['draws'], record['losses']))
    print('Mean length: {0:.2f}'.format(record['mean_length']))


def print_summary(args, rewards, lengths=None):
    print('Performed {} tests for {}.'.format(args.test_count, args.game))
    if sticky.flag_of(args) > 0.0:
        print('Sticky actions: P = {0:g}'.format(sticky.flag_of(args)))
    for label, stat in (('Mean', np.mean), ('Min', np.min), ('Max', np.max), ('Std', np.std)):
        print('{0}: {1:.2f}'.format(label, stat(rewards)))
    if lengths is not None:
        print('Mean length: {0:.2f}'.format(np.mean(lengths)))


def main(argv=None):
    cli = get_arg_parser().parse_args(argv)
    if cli.versus is not None:
        check_versus_flags(cli)
        rewards, _, record = match_on_device(cli)
        print_match_summary(cli, record)
        return rewards
    if cli.device_environments:
        check_device_flags(cli)
        args = restore_settings(cli)
        rewards, lengths = evaluate_on_device(cli, args)
        print_summary(args, rewards, lengths)
        return rewards
    args = restore_settings(cli)
    sticky.check_flags(args)
    seed = int(np.random.RandomState(int(time.time())).randint(1000))
    network_creator, env_creator = get_network_and_environment_creator(args, random_seed=seed)
    # sticky actions (paac_amd/sticky.py): the twins come wrapped, on the evaluation's stream, keyed by --eval_seed (default:
    # the seed of this evaluation's games)
    env_creator.sticky_stream = sticky.EVAL_STREAM_STICKY
    env_creator.sticky_seed = cli.eval_seed if cli.eval_seed is not None else seed
    network = network_creator()
    ctx = hip_ops.Context(network.arch_id, env_creator.num_actions, max_batch=max(1, args.test_count),
                          device_index=network.torch_device.index or 0)
    session = Session(network, ctx)
    network.init(os.path.join(cli.folder, 'checkpoints'), network.make_saver(), session)
    hook = None
    if args.gif_name:
        hook = lambda i: get_save_frame(os.path.join(args.gif_folder, args.gif_name + str(i)))
    try:
        rewards = evaluate(network, env_creator, session, args.test_count, noops=args.noops, on_new_frame=hook)
    finally:
        session.close()
        ctx.close()
    print_summary(args, rewards)
    return rewards


if __name__ == '__main__':
    main()
