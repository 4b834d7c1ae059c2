"""--ppo_target_kl D: KL early stopping inside the optimizer step (include/paac_hip.h has the contract).  CPU side: the flag,
its refusals at learner construction, args.json files with and without it, and the header's declarations.  The GPU side is
tests/test_ppo_target_kl_gpu.py and tests/test_ppo_target_kl_dp_gpu.py."""
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_flag_default_and_args_json_round_trip(tmp_path):
    from paac_amd import logger_utils, train
    p = train.get_arg_parser()
    assert p.parse_args([]).ppo_target_kl == 0.0
    a = p.parse_args(["--ppo_epochs", "4", "--ppo_target_kl", "0.02"])
    assert a.ppo_target_kl == 0.02
    assert ("--ppo_target_kl",) in {f[0] for f in train.BUILD_FLAGS}
    logger_utils.save_args(a, str(tmp_path))
    assert logger_utils.load_args(str(tmp_path / "args.json"))["ppo_target_kl"] == 0.02


def _construct(**fields):
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner
    args = train.get_arg_parser().parse_args([])
    for k, v in fields.items():
        setattr(args, k, v)
    args.num_actions = 4
    return ActorLearner(None, None, args)


@pytest.mark.parametrize("value", [-0.01, -1, float("nan"), float("inf"), float("-inf"), "0.02", None, True, False, [0.02]])
@pytest.mark.parametrize("epochs", [1, 4])
def test_actor_learner_refuses_bad_values(value, epochs):
    """Negative, NaN, infinite, not a number, a bool: refused before anything touches a device, whatever --ppo_epochs says."""
    with pytest.raises(ValueError, match="ppo_target_kl"):
        _construct(ppo_target_kl=value, ppo_epochs=epochs)


def _probe(**fields):
    """The learner's fields as far as the constructor gets without a device: it fails behind every flag check, on the
    missing environment creator."""
    from paac_amd import train
    from paac_amd.actor_learner import ActorLearner

    class Probe(ActorLearner):
        def __init__(self, args):
            with pytest.raises(AttributeError, match="create_environment"):
                super(Probe, self).__init__(None, None, args)
    args = train.get_arg_parser().parse_args([])
    for k, v in fields.items():
        setattr(args, k, v)
    args.num_actions = 4
    return Probe(args)


@pytest.mark.parametrize("fields,on,thr", [
    (dict(ppo_target_kl=0.02), False, np.float32(0.03)),                     # D > 0 at --ppo_epochs 1: accepted and ignored
    (dict(ppo_target_kl=0.02, ppo_epochs=4), True, np.float32(0.03)),
    (dict(ppo_target_kl=0, ppo_epochs=4), False, np.float32(0)),
    (dict(ppo_target_kl=np.float32(0.5), ppo_epochs=2), True, np.float32(0.75)),
    (dict(ppo_target_kl=1e30, ppo_epochs=2), True, np.float32(1.5e30)),
    (dict(ppo_epochs=4), False, np.float32(0)),
])
def test_good_values_pass_the_checks(fields, on, thr):
    L = _probe(**fields)
    assert L.target_kl_on is on and L.kl_thr == float(thr) and L.ppo_target_kl == float(fields.get("ppo_target_kl", 0.0))
    assert L.is_gated_step(1) is on and not L.is_gated_step(0) and not L.is_gated_step(None)


def test_an_args_file_from_before_the_flag_means_off(tmp_path):
    """The learner reads the field with a default: a Namespace rebuilt from an old args.json has none and passes the checks;
    nothing in the evaluation reads it."""
    import argparse
    from paac_amd import logger_utils, train
    from paac_amd.actor_learner import ActorLearner
    a = train.get_arg_parser().parse_args(["--ppo_epochs", "4"])
    logger_utils.save_args(a, str(tmp_path))
    path = str(tmp_path / "args.json")
    old = json.load(open(path))
    assert old.pop("ppo_target_kl") == 0.0
    json.dump(old, open(path, "w"))
    loaded = logger_utils.load_args(path)
    assert "ppo_target_kl" not in loaded
    ns = argparse.Namespace(**loaded)
    ns.num_actions = 4
    with pytest.raises(AttributeError):                # past every flag check: off
        ActorLearner(None, None, ns)
    for name in ("test.py", "evaluation.py"):
        assert "ppo_target_kl" not in open(os.path.join(ROOT, "paac_amd", name)).read()


def test_threshold_is_the_float32_of_one_and_a_half_d():
    """thr = float32(1.5 * D), what the kernel compares in fp32; nothing is computed for D = 0."""
    L = _probe(ppo_epochs=3, ppo_target_kl=0.02)
    assert L.target_kl_on and L.kl_thr == float(np.float32(1.5 * 0.02)) and L.first_gated_step == 1
    assert [L.is_gated_step(s) for s in (None, 0, 1, 2, 3)] == [False, False, True, True, False]
    L = _probe(ppo_epochs=3, ppo_target_kl=0.02, ppo_minibatches=2, emulator_counts=32)
    assert L.first_gated_step == 0 and [L.is_gated_step(s) for s in (0, 5, 6)] == [True, True, False]
    L = _probe(ppo_epochs=1, ppo_target_kl=0.02, ppo_minibatches=2, emulator_counts=32)
    assert not L.target_kl_on and not L.is_gated_step(0)


def test_header_declares_the_entries_and_the_struct():
    from paac_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "paac_hip.h")).read()
    for name, twin, nargs in (("paac_clip_rmsprop_gated", "paac_clip_rmsprop", 16), ("paac_clip_adam_gated", "paac_clip_adam", 17)):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name + " missing from the header"
        assert len(m.group(1).split(",")) == len(_lib._SIGNATURES[name][1]) == nargs == len(_lib._SIGNATURES[twin][1]) + 1
        assert "const paac_kl_gate* gate" in m.group(1) and name in _lib.EXPORTED_SYMBOLS
        # the twin's arguments, then the gate, then the stream
        t = re.search(r"int\s+%s\s*\(([^;]*)\);" % twin, hdr).group(1)
        strip = lambda s: [" ".join(a.split()) for a in s.split(",")]
        assert strip(m.group(1)) == strip(t)[:-1] + ["const paac_kl_gate* gate", "paac_stream_t stream"]
    m = re.search(r"typedef struct \{([^}]*)\} paac_kl_gate;", hdr)
    assert m, "paac_kl_gate missing from the header"
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["const float* kl", "float scale", "float thr", "int first", "int32_t* stop", "int32_t* applied",
                      "float* checked"]
    assert [f[0] for f in _lib.KlGate._fields_] == ["kl", "scale", "thr", "first", "stop", "applied", "checked"]
    for text in ("--ppo_target_kl", r"float32\(1\.5 \* D\)", "A NaN stops too", "sticky"):
        assert re.search(text, hdr), text
