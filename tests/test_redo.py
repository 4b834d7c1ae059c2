"""--redo_every on the host (spec and twin: paac_amd/redo.py): the twin against the rule restated per element, the draw, the flags."""
import json
import os

import numpy as np
import pytest

from paac_amd import evaluation, redo


def tiny_layout():
    """Two conv layers of 16 channels (3x3 over 4 planes, 2x2), fc 64 behind 2 positions, 3 actions -- padded like paac_param_layout."""
    shapes = [("conv1_weights", (3, 3, 4, 16)), ("conv1_biases", (16,)), ("conv2_weights", (2, 2, 16, 16)), ("conv2_biases", (16,)),
              ("fc3_weights", (32, 64)), ("fc3_biases", (64,)), ("actor_output_weights", (64, 3)), ("actor_output_biases", (3,)),
              ("critic_output_weights", (64, 1)), ("critic_output_biases", (1,))]
    tensors, at = [], 0
    for name, shape in shapes:
        tensors.append(dict(name=name, shape=shape, offset=at, size=int(np.prod(shape))))
        at += (tensors[-1]["size"] + 3) // 4 * 4
    return dict(tensors=tensors, total=at)


@pytest.mark.parametrize("optimizer", [redo.RMSPROP, redo.ADAM])
def test_twin_equals_the_rule_element_by_element(optimizer):
    lay = tiny_layout()
    mask = np.zeros(16 + 16 + 64, dtype=np.int32)
    m1, m2, m3 = mask[:16], mask[16:32], mask[32:]
    m1[[0, 5]], m2[[5, 15]], m3[[0, 63]] = 1, 1, 1            # conv2 element [.., 5, 5] is both incoming and outgoing
    rs = np.random.RandomState(1)
    before = [rs.randn(lay["total"]).astype(np.float32) for _ in range(3)]
    params, s0, s1 = (b.copy() for b in before)
    counts = redo.recycle(lay, params, (s0, s1), mask, seed=3, event=2, optimizer=optimizer)
    fan = {"conv1": 36, "conv2": 64, "fc3": 32}
    want, touched = before[0].copy(), np.zeros(lay["total"], dtype=bool)
    rule = {"conv1_weights": (m1, None), "conv2_weights": (m2, m1), "fc3_weights": (m3, m2), "actor_output_weights": (None, m3),
            "critic_output_weights": (None, m3), "conv1_biases": (m1, None), "conv2_biases": (m2, None), "fc3_biases": (m3, None)}
    for t in lay["tensors"]:
        out, inp = rule.get(t["name"], (None, None))
        for index in np.ndindex(*t["shape"]):
            at = t["offset"] + int(np.ravel_multi_index(index, t["shape"]))
            c = index[-2] % len(inp) if inp is not None else 0          # (fc rows are p * C + c)
            if inp is not None and inp[c]:
                want[at], touched[at] = 0.0, True
            elif out is not None and out[index[-1]]:
                bias = t["name"].endswith("biases")
                want[at] = 0.0 if bias else redo.draw(3, 2, [at], fan[t["name"].split("_")[0]])[0]
                touched[at] = True
    assert np.array_equal(params.view(np.uint32), want.view(np.uint32))
    for slot, old, value in zip((s0, s1), before[1:], redo.FRESH_SLOTS[optimizer]):
        assert np.array_equal(slot.view(np.uint32), np.where(touched, np.float32(value), old).view(np.uint32))
    assert counts == redo.parameter_counts(lay, mask) and sum(counts.values()) == touched.sum()
    assert params[lay["tensors"][2]["offset"] + int(np.ravel_multi_index((1, 1, 5, 5), (2, 2, 16, 16)))] == 0.0          # outgoing wins


def test_draw_is_word0_of_the_stated_counter():
    idx = np.array([0, 7, 123456, 2 ** 31 + 5], dtype=np.uint64)
    word0 = evaluation.philox_word0(11 + (9 << 32), 4 << 32, idx, 0x5245444F)          # counter (index, 0, event 4, "REDO")
    d = np.float32(1.0 / np.sqrt(2592.0))
    want = -d + (d + d) * ((word0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24))
    got = redo.draw(11 + (9 << 32), 4, idx, 2592)
    assert got.dtype == np.float32 and np.array_equal(got, want) and (np.abs(got) <= d).all() and len(set(got)) == 4


def test_flags_are_refused_with_a_message():
    from paac_amd import train
    for argv, world, message in ((["--redo_every", "-1"], 1, "integer >= 0"), (["--redo_every", "2"], 1, "needs --feature_stats true"),
                                 (["--redo_every", "2", "--feature_stats", "true"], 2, "one GPU")):
        with pytest.raises(ValueError, match=message):
            redo.check_flags(train.get_arg_parser().parse_args(["--emulator", "catch"] + argv), world)


def test_flag_defaults_off_and_survives_args_json(tmp_path):
    import argparse
    from paac_amd import train
    parser = train.get_arg_parser()
    assert redo.check_flags(parser.parse_args([])) == 0 and redo.check_flags(argparse.Namespace()) == 0
    args = parser.parse_args(["--feature_stats", "true", "--redo_every", "3", "-df", str(tmp_path)])
    train.save_args(args, str(tmp_path))
    with open(os.path.join(str(tmp_path), "args.json")) as f:
        back = argparse.Namespace(**json.load(f))
    assert back.redo_every == 3 and redo.check_flags(back) == 3
