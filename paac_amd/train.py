"""Command line and creator wiring of the trainer (the role of reference train.py:14-109).

The flag NAMES, short forms, destinations and defaults are the reference's (train.py:79-98) -- they are the contract
a run script depends on -- and so are `get_network_and_environment_creator(args)`, `get_arg_parser()`, `bool_arg` and
`main(args)`.  The flags are kept as a table below; `BUILD_FLAGS` are this build's additions.

  python -m paac_amd.train -g breakout --arch NATURE -df logs/
"""
import argparse
import functools
import logging
import os
import signal
import sys

from . import duel_pool, environment_creator, evaluation, logger_utils, match, parallel, sticky, window_stats
from .paac import PAACLearner
from .policy_v_network import NaturePolicyVNetwork, NIPSPolicyVNetwork


def bool_arg(string):
    """'true' / 'false' (any case) -> bool; anything else is an argparse error."""
    try:
        return {"true": True, "false": False}[string.lower()]
    except KeyError:
        raise argparse.ArgumentTypeError("Expected True or False, but got {}".format(string))


def _game_path(string):
    """--device_game: the path made absolute (args.json records it so: paac_amd.test -f FOLDER finds the game again)."""
    return os.path.abspath(string) if string else ""


# (option strings, dest, default, type, help)
REFERENCE_FLAGS = (
    (("-g",), "game", "pong", None, "game to play"),
    (("-d", "--device"), "device", "/gpu:0", str, "'/gpu:N' selects the MI355X; '/cpu:0' is rejected (no CPU path)"),
    (("--rom_path",), "rom_path", "./atari_roms", None, "directory with the game ROMs (ALE environments only)"),
    (("-v", "--visualize"), "visualize", False, bool_arg, "call on_new_frame with every emulator screen"),
    (("--e",), "e", 0.1, float, "Epsilon for the Rmsprop and Adam optimizers (textbook Adam uses 1e-8; with Adam it is "
                                "added outside the square root)"),
    (("--alpha",), "alpha", 0.99, float, "RMSProp decay of the squared-gradient average (ignored by Adam)"),
    (("-lr", "--initial_lr"), "initial_lr", 0.0224, float, "learning rate at step 0"),
    (("-lra", "--lr_annealing_steps"), "lr_annealing_steps", 80000000, int,
     "global steps over which the learning rate falls linearly to zero"),
    (("--entropy",), "entropy_regularisation_strength", 0.02, float, "weight of the policy-entropy bonus"),
    (("--clip_norm",), "clip_norm", 3.0, float, "gradient norm the update is clipped to"),
    (("--clip_norm_type",), "clip_norm_type", "global", None, "'global' (global norm), 'local' (layer-wise norm: "
                                                             "each weight and bias tensor clipped on its own), "
                                                             "'ignore' (no clipping)"),
    (("--gamma",), "gamma", 0.99, float, "discount factor"),
    (("--max_global_steps",), "max_global_steps", 80000000, int, "environment steps to train for"),
    (("--max_local_steps",), "max_local_steps", 5, int, "t_max: steps per environment between updates"),
    (("--arch",), "arch", "NIPS", None, "'NIPS' or 'NATURE' (anything that is not NIPS selects NATURE)"),
    (("--single_life_episodes",), "single_life_episodes", False, bool_arg, "end an episode when a life is lost"),
    (("-ec", "--emulator_counts"), "emulator_counts", 32, int, "environments per learner (per GPU)"),
    (("-ew", "--emulator_workers"), "emulator_workers", 8, int, "host processes stepping host environments"),
    (("-df", "--debugging_folder"), "debugging_folder", "logs/", str, "checkpoints, args.json, metrics.jsonl"),
    (("-rs", "--random_start"), "random_start", True, bool_arg, "up to 30 no-op frames after every reset"),
)
BUILD_FLAGS = (
    (("--sampler",), "sampler", "philox", None,
     "device loop action sampler: 'numpy' = the reference's np.random.multinomial stream bit for bit, 'philox' = "
     "counter-based"),
    (("--sampler_seed",), "sampler_seed", 42, int, "seed of the counter-based sampler"),
    (("--host_environments",), "host_environments", False, bool_arg,
     "step BaseEnvironment plugins on the host even when a device twin exists"),
    (("--synthetic_terminal_p",), "synthetic_terminal_p", 0.01, float, "per-step terminal probability (synthetic)"),
    (("--synthetic_raw_frames",), "synthetic_raw_frames", False, bool_arg,
     "synthetic environments emit two raw 210x160 screens per step (GPU max + resize + history)"),
    (("--emulator",), "emulator", "synthetic", None,
     "'synthetic' (paac_amd/synthetic.py), 'catch' (paac_amd/catch.py: a learnable game on the GPU, 3 actions; -g, "
     "--synthetic_terminal_p and --synthetic_raw_frames do not apply), 'bricks' (paac_amd/bricks.py: a brick-wall game with "
     "three lives on the GPU, 3 actions, episodes of up to 500 steps; --single_life_episodes applies, -g, "
     "--synthetic_terminal_p, --synthetic_raw_frames and --random_start do not), 'rally' (paac_amd/rally.py: a two-paddle game "
     "against a scripted opponent on the GPU, the 6 actions of ALE Pong, rewards of both signs, first to five points, episodes "
     "of up to 1000 steps; --single_life_episodes, -g, --synthetic_terminal_p, --synthetic_raw_frames and --random_start do not "
     "apply), 'duel' (paac_amd/duel.py: rally played against the learner itself on the GPU -- -ec rows are -ec / 2 boards, the "
     "network plays both paddles, each row seeing the board from its own side; device loop only, -ec must be even, the logged "
     "returns average 0 by construction: use --eval_every, which scores the policy against rally's scripted opponent; "
     "--host_environments true is refused, --single_life_episodes, -g, --synthetic_terminal_p, --synthetic_raw_frames and "
     "--random_start do not apply), 'user' (with --device_game PATH: a user's own game compiled into the device loop, "
     "paac_amd/user_game.py; -g, --synthetic_terminal_p, --synthetic_raw_frames and --random_start do not apply, --duel_pool and "
     "--eval_match stay duel's) or 'ale' (Atari through an installed Arcade Learning Environment)"),
    (("--device_game",), "device_game", "", _game_path,
     "--emulator user: the game's specification module, a Python file (examples/patrol/patrol.py is one) that names the "
     "game's numbers, its host twin and the header with its device trait; the trait is compiled into a library of its own on "
     "first use (paac_amd/libpaac_hip_game_<file stem>.so) and the process loads that library; cannot be combined with "
     "--user_arch; args.json records the absolute path"),
    (("--device_preprocess",), "device_preprocess", False, bool_arg,
     "host environments hand out raw screen pairs; max + resize + frame history run on the GPU"),
    (("--user_arch",), "user_arch", "", None,
     "a user architecture instead of --arch (compiled on first use): filter counts of the 2 or 3 conv layers of the "
     "reference trunks' shapes (8x8/4, 4x4/2[, 3x3/1]) and the fc width, e.g. 32,64,64,1024 -- or filters:size:stride per "
     "layer, e.g. 32:8:4,64:5:2,64:3:1,512"),
    (("--optimizer",), "optimizer", "rmsprop", None,
     "update rule applied to the clipped gradients: 'rmsprop' (the reference's) or 'adam' (TF AdamOptimizer with --beta1, "
     "--beta2 and --e; --alpha is ignored)"),
    (("--beta1",), "beta1", 0.9, float, "Adam decay of the first-moment average"),
    (("--beta2",), "beta2", 0.999, float, "Adam decay of the second-moment average"),
    (("--gae_lambda",), "gae_lambda", 1.0, float,
     "advantage estimator: 1.0 = the reference's n-step return (bit for bit); a value in [0, 1) = generalized advantage "
     "estimation GAE(lambda) on the same rollout records, 0 being the one-step TD error"),
    (("--ppo_epochs",), "ppo_epochs", 1, int,
     "optimizer steps per rollout: 1 = the reference's single update (bit for bit, whatever --ppo_clip says); K in [2, 16] = "
     "PPO: epoch 1 is that update, epochs 2..K re-run the training forward on the same rollout under the clipped "
     "probability-ratio objective"),
    (("--ppo_clip",), "ppo_clip", 0.2, float, "PPO clip range EPS in (0, 1): the ratio is clipped to [1 - EPS, 1 + EPS]; read "
                                              "only when --ppo_epochs is above 1"),
    (("--ppo_vclip",), "ppo_vclip", 0.0, float,
     "PPO value clipping range EPSV: 0 = off; above 0, epochs 2..K use the critic term max((y - v)^2, (y - vc)^2) with vc = v "
     "clipped to within EPSV of the value epoch 1 computed; read only when --ppo_epochs is above 1"),
    (("--ppo_minibatches",), "ppo_minibatches", 1, int,
     "minibatches per PPO epoch: 1 = full-batch epochs; M in [2, 16] (a divisor of emulator_counts x max_local_steps, with "
     "ppo_epochs x M <= 64) = every epoch is M optimizer steps on a fresh shuffle of the rollout, drawn on the GPU from "
     "--sampler_seed; read only when --ppo_epochs is above 1"),
    (("--ppo_target_kl",), "ppo_target_kl", 0.0, float,
     "PPO KL early stopping D: 0 = off; above 0, an optimizer step of a rollout whose approx_kl (the mean of log p_old - log p "
     "over the step's own batch, the ranks' mean under data parallelism) exceeds 1.5 x D is skipped on the GPU together with "
     "every step after it in that rollout (the first full-batch step, whose ratio is 1, is never skipped); the skipped steps' "
     "forward and backward still run, so a cycle takes the same time; read only when --ppo_epochs is above 1"),
    (("--adv_norm",), "adv_norm", False, bool_arg,
     "normalise each rollout's advantages by their own mean and standard deviation before the actor term reads them (per "
     "rank under data parallelism); the critic target and the recorded advantages are unchanged"),
    (("--bootstrap_truncated",), "bootstrap_truncated", False, bool_arg,
     "--emulator bricks|rally: a step that ends its episode only because the game's step cap was reached (500 / 1000 steps) "
     "bootstraps its return from the value of the last state seen, r + gamma x V, instead of counting the state as worth "
     "nothing (partial-episode bootstrapping; either estimator, every update option, device and host loops); the step is "
     "still terminal and the environment still resets; accepted and without effect for catch, synthetic and ale"),
    (("--window_stats",), "window_stats", False, bool_arg,
     "off by default; true = every cycle is folded on the GPU into running statistics of the log window (one small launch per "
     "cycle behind the update, device and host loops; paac_amd/window_stats.py), and every 'progress' record is followed by a "
     "'window' record in metrics.jsonl: explained variance of the critic, value / return / advantage moments, action "
     "frequencies, the loss scalars and gradient norm averaged over all updates, and the statistics of all episodes finished "
     "in the window; one GPU only (refused under data parallelism).  Training is bit-identical with it on or off"),
    (("--eval_every",), "eval_every", 0, int,
     "device loop, --emulator catch|bricks|rally: score the current policy on --eval_count held-out game instances (seed random_seed "
     "+ 1, up to 30 no-op steps, whole episodes) at the first chunk boundary at or after every multiple of this many global "
     "steps, on the GPU, and write an 'eval' record to metrics.jsonl; 0 = off.  Training is bit-identical with it on or off"),
    (("--eval_count",), "eval_count", 64, int, "environments (one episode each) of an --eval_every evaluation, 1 to 4096"),
    (("--eval_greedy",), "eval_greedy", True, bool_arg,
     "--eval_every evaluations take the argmax action (true) or sample from the policy on a Philox stream of their own (false)"),
    (("--eval_match",), "eval_match", 0, int,
     "--emulator duel with --eval_every: at every evaluation the live weights also play this many duel boards (1 to 4096; 0 = "
     "off), one episode each, against a copy of the weights taken at the previous evaluation (at the first one: the weights "
     "the run started or resumed from), on the GPU (paac_amd/match.py), with --eval_greedy, up to 30 no-op steps and seed "
     "random_seed + 1, and a 'match' record goes to metrics.jsonl: the self-play learning curve.  Training is bit-identical "
     "with it on or off"),
    (("--duel_pool",), "duel_pool", 0, int,
     "--emulator duel: 0 = off (every board is played by the live weights on both sides); K in [1, 16] = -ec rows are -ec "
     "boards, every learner row the bottom player of its own board, and the top player is a frozen earlier copy of the policy "
     "drawn from a pool of up to K such copies (paac_amd/duel_pool.py); the logged training return is then the learner's "
     "against the pool, no longer 0 by construction; one GPU only; the pool is not checkpointed"),
    (("--duel_pool_every",), "duel_pool_every", 102400, int,
     "global steps between pool events: the live weights are frozen into the pool and the next opponent is drawn (a design "
     "choice, not a measured optimum); read only when --duel_pool is above 0"),
    (("--duel_pool_latest_p",), "duel_pool_latest_p", 0.5, float,
     "probability in [0, 1] that the opponent of the next period is the newest frozen copy rather than a uniformly drawn pool "
     "member (a design choice, not a measured optimum); read only when --duel_pool is above 0"),
    (("--sticky_action_p",), "sticky_action_p", 0.0, float,
     "sticky actions (Machado et al. 2018; paac_amd/sticky.py): at every step, with probability P in [0, 1), an environment "
     "executes the action it executed on its previous step instead of the one the agent chose (the agent is not told: the "
     "rollout records the chosen action); 0 = off, and nothing differs.  --emulator catch|bricks|rally|duel|user: decided on "
     "the GPU inside the game's step, by a counter-based draw keyed by the game seed, the environment and its step count "
     "(device and host loops agree record for record; --eval_every evaluates with the same P); --emulator ale: handed to ALE's "
     "repeat_action_probability; --emulator synthetic: accepted and without effect; refused with --duel_pool and --eval_match"),
    (("--checkpoint_format",), "checkpoint_format", "npz", None,
     "container of the checkpoints written: 'npz', or 'tf' = the reference's TensorFlow V2 tensor bundle "
     "(.index + .data-00000-of-00001); both are read"),
)


def get_arg_parser():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for options, dest, default, kind, text in REFERENCE_FLAGS + BUILD_FLAGS:
        kwargs = dict(dest=dest, default=default, help=text)
        if kind is not None:
            kwargs["type"] = kind
        if dest in ("sampler", "emulator", "checkpoint_format", "optimizer"):
            kwargs["choices"] = {"sampler": ["philox", "numpy"], "emulator": ["synthetic", "catch", "bricks", "rally", "duel", "user", "ale"],
                                 "checkpoint_format": ["npz", "tf"], "optimizer": ["rmsprop", "adam"]}[dest]
        parser.add_argument(*options, **kwargs)
    return parser


def get_network_and_environment_creator(args, random_seed=3):
    """-> (network_creator(name='local_learning'), environment creator); fills args.num_actions / args.random_seed
    the way train.py:52-56 does."""
    env_creator = environment_creator.EnvironmentCreator(args)
    args.num_actions = env_creator.num_actions
    args.random_seed = random_seed
    conf = dict(num_actions=args.num_actions, device=args.device, clip_norm=args.clip_norm,
                clip_norm_type=args.clip_norm_type,
                entropy_regularisation_strength=args.entropy_regularisation_strength)
    network_class = NIPSPolicyVNetwork if args.arch == 'NIPS' else NaturePolicyVNetwork
    if getattr(args, "user_arch", ""):
        # networks.py:117-120 / README.md:80-83: a new trunk mixed into PolicyVNetwork
        from .networks import define_architecture
        from .policy_v_network import PolicyVNetwork
        from .build import parse_user_arch
        trunk = define_architecture("USER", *parse_user_arch(args.user_arch))
        network_class = type("UserPolicyVNetwork", (PolicyVNetwork, trunk), {})

    def network_creator(name='local_learning'):
        return network_class(dict(conf, name=name))

    return network_creator, env_creator


check_eval_flags = evaluation.check_train_flags      # (args, world_size) -> on?; raises ValueError with the refusal


def _stop(learner, owner_pid, signum, frame):
    """First signal: ask the training loop to stop at the next cycle boundary (it then runs cleanup() itself, with
    nothing in flight on the GPU and, data parallel, every rank leaving at the same cycle).  Second signal: clean up
    right here, as upstream does (train.py:38-49)."""
    if os.getpid() != owner_pid:          # forked emulator workers inherit the handler: only the trainer reacts
        return
    if not learner.stop_requested:
        logging.info('Signal %s detected, stopping at the next cycle boundary.', signum)
        learner.stop_requested = True
        return
    if parallel.world_size() > 1:
        # data parallel: cleanup() is collective (the checkpoint barrier, the pending optimizer step's graph) and only THIS
        # rank was signalled twice -- running it here would hang this rank in the barrier and leave its peers one
        # collective out of step.  The first signal's agreed stop is the clean way out; a second one just leaves.
        logging.info('Signal %s detected again on a data-parallel rank: exiting without the collective cleanup.', signum)
        os._exit(1)
    logging.info('Signal %s detected again, cleaning up now.', signum)
    learner.cleanup()
    logging.info('Cleanup completed, shutting down...')
    sys.exit(0)


def setup_kill_signal_handler(learner):
    handler = functools.partial(_stop, learner, os.getpid())
    for signum in (signal.SIGTERM, signal.SIGINT):
        signal.signal(signum, handler)


def main(args):
    """train.py:24-35.  Under `python -m torch.distributed.run --nproc-per-node G -m paac_amd.train ...` every process
    is one data-parallel rank: its GPU is '/gpu:<LOCAL_RANK>', `-ec` environments PER GPU (global_step advances by
    G * ec per step), gradients are summed over RCCL once per update, rank 0 writes checkpoints / args / metrics."""
    world = parallel.init_from_env(args)          # before anything touches a GPU
    logging.debug('Configuration: %s', args)
    check_eval_flags(args, world)                 # --eval_every's refusals, before a learner exists
    match.check_train_flags(args)                 # ... and --eval_match's
    duel_pool.check_train_flags(args, world)      # ... and --duel_pool's
    window_stats.check_flags(args, world)         # ... and --window_stats'
    sticky.check_flags(args)                      # ... and --sticky_action_p's
    network_creator, env_creator = get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args)
    setup_kill_signal_handler(learner)
    logging.info('Starting training (%d data-parallel rank%s)', world, '' if world == 1 else 's')
    try:
        learner.train()
    except parallel.ReplicaMismatch as exc:
        # every rank raises at the same cycle (the comparison is itself a collective): no checkpoint of diverged weights,
        # no collective cleanup, a non-zero exit code for the launcher
        logging.error('%s -- stopping', exc)
        sys.exit(3)
    logging.info('Finished training')
    parallel.shutdown()


save_args = logger_utils.save_args      # logger_utils.py:15-20


if __name__ == '__main__':
    logging.basicConfig(stream=sys.stdout, level=logging.DEBUG)
    cli_args = get_arg_parser().parse_args()
    if int(os.environ.get("RANK", "0")) == 0:
        save_args(cli_args, cli_args.debugging_folder)
    main(cli_args)
