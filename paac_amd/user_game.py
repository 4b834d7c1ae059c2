"""--emulator user --device_game PATH: a user's game compiled into the device loop, without an edit inside the package.

The environment-side twin of --user_arch: a BaseEnvironment plugin runs in the host loop; a game that also states its step as
a device trait (csrc/game_dev.h's contract for a non-paired game) is compiled into a library of its own on first use
(paac_amd/build.py: build_user_game -- only csrc/games.hip is compiled again), the process loads that one library, and the game
runs through everything a built-in game runs through, under the kind "user".

PATH is a Python file, the game's SPECIFICATION MODULE (examples/patrol/patrol.py is the worked example).  It is loaded by path
with importlib and added to nothing global.  It defines
  NUM_ACTIONS          the policy's width, within [2, 32]                                (the trait's kActions)
  STATE_WORDS          int32 words of a device state record, a positive multiple of 4    (the trait's kWords)
  MAX_EPISODE_STEPS    the longest episode in steps: what bounds an evaluation           (the trait's kMaxSteps)
  TRUNCATES            bool: whether that length is a step cap --bootstrap_truncated may bootstrap at (the trait's advance
                       then reports *trunc), or the game's own rule
  STEP_OPTION          None, or "single_life": the trait's `opt` is --single_life_episodes (the one option key supported)
  DEVICE_HEADER        the header with the trait, a file name relative to the module
  DEVICE_TRAIT         the trait struct's name in that header (inside namespace paac, or qualified)
  Environment          the host twin: a BaseEnvironment with __init__(actor_id, seed=0, **options) (options: STEP_OPTION's key),
                       state_words() -> int32 [STATE_WORDS] and last_step_truncated -- exactly the shape of RallyEnvironment.
                       The twin and the trait must produce the same numbers; the package's tests hold one against the other
The library's tag is the module's file stem ([A-Za-z0-9_]+); two modules with one stem are refused, not silently shared.
A process holds ONE library: --device_game cannot be combined with --user_arch (combining the two sets of defines is not built).
"""
import importlib.util
import os

from . import _lib

KIND = "user"
OPTION_KEYS = ("single_life",)       # STEP_OPTION's values besides None; each is read by EnvironmentCreator._<key>()

_REQUIRED = (("NUM_ACTIONS", int), ("STATE_WORDS", int), ("MAX_EPISODE_STEPS", int), ("TRUNCATES", bool),
             ("STEP_OPTION", (type(None), str)), ("DEVICE_HEADER", str), ("DEVICE_TRAIT", str))

_loaded = {}                         # absolute path -> module: load() is idempotent within a process


def check_flags(args):
    """Start-up refusals of --device_game / --emulator user (a ValueError with the message); nothing is built or loaded."""
    path = getattr(args, "device_game", "") or ""
    emulator = getattr(args, "emulator", "synthetic")
    if path and emulator != KIND:
        raise ValueError("--device_game %s needs --emulator user (got --emulator %s)" % (path, emulator))
    if emulator == KIND and not path:
        raise ValueError("--emulator user needs --device_game PATH: the game's specification module (a Python file; "
                         "examples/patrol/patrol.py is one)")
    if path and getattr(args, "user_arch", ""):
        raise ValueError("--device_game cannot be combined with --user_arch %s: a process holds ONE kernel library, and a build "
                         "with both a user architecture and a user game in it is not built" % args.user_arch)
    if path and getattr(args, "synthetic_raw_frames", False):
        raise ValueError("--emulator user has no raw 210x160 frames: --synthetic_raw_frames applies to --emulator synthetic only")
    return bool(path)


def tag_of(path):
    """The library tag of specification module `path`: its file stem (build.user_game_library refuses a bad one)."""
    return os.path.splitext(os.path.basename(path))[0]


def import_module(path):
    """The specification module at `path`, loaded by path and validated: a ValueError names what is missing or mistyped."""
    path = os.path.abspath(path)
    if not os.path.isfile(path):
        raise FileNotFoundError("--device_game %s: no such file (the game's specification module; a run restored from "
                                "args.json needs the file where the training run had it)" % path)
    from .build import user_game_library
    user_game_library(tag_of(path))                        # a bad tag is refused before anything of the module runs
    spec = importlib.util.spec_from_file_location("paac_user_game_" + tag_of(path), path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    validate(module, path)
    return module


def validate(module, path="the module"):
    problems = []
    for name, types in _REQUIRED:
        if not hasattr(module, name):
            problems.append("%s is missing" % name)
        else:
            value = getattr(module, name)
            # (bool is an int: a number given as True is mistyped)
            if not isinstance(value, types) or (types is int and isinstance(value, bool)):
                expected = "None or str" if isinstance(types, tuple) else types.__name__
                problems.append("%s = %r is %s, expected %s" % (name, value, type(value).__name__, expected))
    if not hasattr(module, "Environment"):
        problems.append("Environment is missing")
    elif not isinstance(module.Environment, type):
        problems.append("Environment = %r is no class" % (module.Environment,))
    else:
        from .environment import BaseEnvironment
        if not issubclass(module.Environment, BaseEnvironment):
            problems.append("Environment %s is no BaseEnvironment" % module.Environment.__name__)
        if not callable(getattr(module.Environment, "state_words", None)):
            problems.append("Environment %s has no state_words()" % module.Environment.__name__)
    if problems:
        raise ValueError("device game %s: %s" % (path, "; ".join(problems)))
    if not 2 <= module.NUM_ACTIONS <= 32:
        raise ValueError("device game %s: NUM_ACTIONS = %d is outside [2, 32]" % (path, module.NUM_ACTIONS))
    if module.STATE_WORDS <= 0 or module.STATE_WORDS % 4:
        raise ValueError("device game %s: STATE_WORDS = %d is no positive multiple of 4" % (path, module.STATE_WORDS))
    if module.MAX_EPISODE_STEPS <= 0:
        raise ValueError("device game %s: MAX_EPISODE_STEPS = %d is not positive" % (path, module.MAX_EPISODE_STEPS))
    if module.STEP_OPTION is not None and module.STEP_OPTION not in OPTION_KEYS:
        raise ValueError("device game %s: STEP_OPTION = %r: expected None or one of %s" % (path, module.STEP_OPTION, OPTION_KEYS))
    if os.path.isabs(module.DEVICE_HEADER):
        raise ValueError("device game %s: DEVICE_HEADER = %r: expected a file name relative to the module" % (path, module.DEVICE_HEADER))


def option_keys(module):
    return () if module.STEP_OPTION is None else (module.STEP_OPTION,)


def load(path, verbose=False):
    """Validate the specification module at `path`, build or find its library, make it the process's library, check the
    numbers compiled into it against the module's, and register the game under the kind "user" (hip_ops.USER_GAMES,
    paac.USER_KINDS).  -> the module.  Every data-parallel rank calls this: the build runs under a file lock."""
    path = os.path.abspath(path)
    if path in _loaded:
        return _loaded[path]
    if _loaded:
        raise ValueError("device game %s: this process already holds the device game %s (one library per process)"
                         % (path, next(iter(_loaded))))
    module = import_module(path)
    from .build import build_user_game
    header = os.path.join(os.path.dirname(path), module.DEVICE_HEADER)
    lib = build_user_game(header, module.DEVICE_TRAIT, tag_of(path), verbose=verbose)
    _lib.use_library(lib)
    compiled = _lib.user_game()
    stated = (module.STATE_WORDS, module.NUM_ACTIONS, module.MAX_EPISODE_STEPS)
    if compiled != stated:
        raise ValueError("device game %s: the module states (STATE_WORDS, NUM_ACTIONS, MAX_EPISODE_STEPS) = %s, the trait %s in "
                         "%s was compiled with (kWords, kActions, kMaxSteps) = %s" % (path, stated, module.DEVICE_TRAIT, header, compiled))
    from . import hip_ops, paac
    hip_ops.register_user_game(module.STATE_WORDS, module.STEP_OPTION)
    paac.register_user_kind(option_keys(module), module.MAX_EPISODE_STEPS, module.TRUNCATES)
    _loaded[path] = module
    return module
