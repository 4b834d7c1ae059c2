"""Environment factory (mirrors reference environment_creator.py:1-15).

The reference probes an ALE ROM for `num_actions` and builds AtariEmulator instances.  ALE is a third-party
emulator that is out of this build's scope, so the factory creates the synthetic
environments of paac_amd/synthetic.py; `num_actions` per game is ALE's minimal action-set size (pinned for
breakout/qbert/seaquest by the reference's pretrained/*/checkpoints/*.index actor_output_biases shapes).
`--emulator catch` creates the catch game of paac_amd/catch.py instead (3 actions, whatever `-g` says), `--emulator bricks`
the brick-wall game of paac_amd/bricks.py (3 actions, lives: `--single_life_episodes` applies), `--emulator rally` the
two-paddle game of paac_amd/rally.py (6 actions, ALE Pong's minimal set; no lives), `--emulator duel` rally played against the
learner itself (paac_amd/duel.py: device loop only, an even `-ec`; the host environment created is rally's), `--emulator user
--device_game PATH` a user's own device game (paac_amd/user_game.py: the action count, the host twin and the device trait come
from the specification module at PATH).
A user environment plugs in exactly as in the reference: subclass BaseEnvironment and return it from
create_environment(i).
"""
from . import bricks, catch, duel, rally, sticky, user_game
from .synthetic import SyntheticEnvironment, terminal_threshold

# ALE minimal action set sizes.
GAME_NUM_ACTIONS = {
    "pong": 6, "breakout": 4, "qbert": 6, "seaquest": 18, "space_invaders": 6, "beam_rider": 9,
    "boxing": 18, "ms_pacman": 9, "name_this_game": 6,
}


# --emulator catch | bricks | rally: the spec module, its host environment, and the options both that environment's constructor
# and the device spec take (each read by the creator's method _<option>).
DEVICE_GAMES = {
    "catch": (catch, catch.CatchEnvironment, ()),
    "bricks": (bricks, bricks.BricksEnvironment, ("single_life",)),
    "rally": (rally, rally.RallyEnvironment, ()),
}

# --emulator duel: the paired games (paac.PAIRED_KINDS) -- the spec module and the HOST environment of the game a run is scored
# on (duel: rally against its scripted opponent; there is no host twin of the paired game itself).
PAIRED_GAMES = {
    "duel": (duel, rally.RallyEnvironment),
}


class EnvironmentCreator(object):
    def __init__(self, args):
        game = getattr(args, "game", "pong")
        self.args = args
        if getattr(args, "emulator", "synthetic") == "ale":
            # environment_creator.py:8-14: the ROM decides the action count; one AtariEmulator per actor.  No device
            # twin: these environments are stepped on the host (screens -> GPU with --device_preprocess true).
            from . import atari_emulator
            probe = atari_emulator._open_ale()
            probe.loadROM(("%s/%s.bin" % (args.rom_path, game)).encode())
            self.num_actions = len(probe.getMinimalActionSet())
            self.create_environment = lambda i: atari_emulator.AtariEmulator(i, args)
            self._device_twin = False
            return
        user_game.check_flags(args)               # --device_game without --emulator user and the reverse, --user_arch beside it
        self._device_twin = True
        self._game = getattr(args, "emulator", "synthetic")
        if self._game == user_game.KIND:
            # a user's device game (paac_amd/user_game.py): the module is validated, its library built or found and made the
            # process's, the game registered under the kind "user"; -g is ignored
            module = user_game.load(args.device_game)
            self._user_options = user_game.option_keys(module)
            self.num_actions = module.NUM_ACTIONS
            self.create_environment = self._sticky(lambda i: module.Environment(i, seed=self._seed(), **self._game_options()))
            return
        if self._game in DEVICE_GAMES:
            # games of their own (-g is ignored), with their own action counts; no raw-screen form
            if self._raw():
                raise ValueError("--emulator %s has no raw 210x160 frames: --synthetic_raw_frames applies to --emulator "
                                 "synthetic only" % self._game)
            module, env_class, _ = DEVICE_GAMES[self._game]
            self.num_actions = module.NUM_ACTIONS
            self.create_environment = self._sticky(lambda i: env_class(i, seed=self._seed(), **self._game_options()))
            return
        if self._game in PAIRED_GAMES:
            # a paired game (paac_amd/duel.py): device loop only -- a row needs its partner's action, and the host loop steps
            # environments one by one.  What is created for the host (paac_amd.test) is the game it is scored on.
            if self._raw():
                raise ValueError("--emulator %s has no raw 210x160 frames: --synthetic_raw_frames applies to --emulator "
                                 "synthetic only" % self._game)
            module, env_class = PAIRED_GAMES[self._game]
            if getattr(args, "host_environments", False):
                raise ValueError("--host_environments true cannot be combined with --emulator %s: the host loop would step %s "
                                 "and silently train against the scripted opponent" % (self._game, env_class.__name__))
            if int(getattr(args, "emulator_counts", 2)) % 2 or int(getattr(args, "emulator_counts", 2)) < 2:
                raise ValueError("-ec / --emulator_counts %s: --emulator %s plays two rows per board and needs an even number "
                                 "of environments per rank" % (getattr(args, "emulator_counts", None), self._game))
            self.num_actions = module.NUM_ACTIONS
            self.create_environment = lambda i: env_class(i, seed=self._seed())
            return
        self.num_actions = int(getattr(args, "num_actions_override", 0) or GAME_NUM_ACTIONS.get(game, 6))
        # args.random_seed is set by train.get_network_and_environment_creator AFTER this constructor runs
        # (train.py:52-56), so it is read when an environment is created, like atari_emulator.py:18 does.
        self.create_environment = lambda i: SyntheticEnvironment(
            i, self.num_actions, seed=self._seed(), terminal_p=self._terminal_p(), raw_frames=self._raw())

    def _seed(self):
        return int(getattr(self.args, "random_seed", 3))

    # --sticky_action_p P (paac_amd/sticky.py): the host twins of catch, bricks, rally and user games come wrapped when P > 0,
    # environment i keyed by (the game seed, i) on the training stream.  An evaluation sets sticky_stream (and sticky_seed,
    # where its key is not the game seed) on the creator before it creates its twins.  P = 0: the twins themselves, as always.
    sticky_stream = sticky.STICKY_STREAM
    sticky_seed = None

    def _sticky(self, create):
        def create_environment(i):
            p = sticky.flag_of(self.args)
            if p <= 0.0:
                return create(i)
            seed = self._seed() if self.sticky_seed is None else int(self.sticky_seed)
            return sticky.StickyEnvironment(create(i), p, seed, i, self.sticky_stream)
        return create_environment

    def _terminal_p(self):
        return float(getattr(self.args, "synthetic_terminal_p", 0.01))

    def _single_life(self):
        return bool(getattr(self.args, "single_life_episodes", False))

    def _game_options(self):
        """The options of the game (DEVICE_GAMES): keywords of the host environment and keys of the device spec alike."""
        keys = self._user_options if self._game == user_game.KIND else DEVICE_GAMES[self._game][2]
        return {key: getattr(self, "_" + key)() for key in keys}

    def _raw(self):
        return bool(getattr(self.args, "synthetic_raw_frames", False))

    @property
    def device_env_spec(self):
        """Device-batched twin of the same environments (PAACLearner uses it when present)."""
        if not self._device_twin:
            return None
        # --sticky_action_p P: the key exists only with P > 0 (read by the rollout and the evaluators: paac.sticky_p_of)
        p = sticky.flag_of(self.args)
        stuck = dict(sticky_p=p) if p > 0.0 else {}
        if self._game in DEVICE_GAMES or self._game == user_game.KIND:
            return dict(kind=self._game, seed=self._seed(), **self._game_options(), **stuck)
        if self._game in PAIRED_GAMES:
            # --duel_pool K (paac_amd/duel_pool.py): the rows are boards played against a pool of frozen opponents; the key
            # exists only with the pool on (read by the training rollout alone: evaluation and matches never see it)
            pool = int(getattr(self.args, "duel_pool", 0) or 0)
            return dict(kind=self._game, seed=self._seed(), **(dict(pool=pool) if pool > 0 else {}), **stuck)
        return dict(kind="synthetic", seed=self._seed(), terminal_threshold=terminal_threshold(self._terminal_p()),
                    raw_frames=self._raw())
