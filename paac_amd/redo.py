"""Recycling dormant units: `--redo_every W` follows every W-th `features` record of a `--feature_stats true` run with one
recycle of the units that record counted as dormant (ReDo, Sokar et al., arXiv 2302.12902): their incoming weights are drawn
afresh, their bias and outgoing weights zeroed, their optimizer slots reset.  The recycle runs eagerly at the progress-record
boundary, from the window's block before it is emptied; nothing of it is inside the captured cycle.

This is the SPEC; the same bits are produced
  * on the host by the plain-numpy `masks` / `recycle` below, and
  * on the device by paac_redo (csrc/redo.h, instantiated in csrc/optim.hip; include/paac_hip.h has the contract).

Spec
  layers       the slots of feature_stats.Layout: conv1, conv2 [, conv3], fc
  mask         unit u of a layer is recycled when it is dormant by feature_stats' rule on the window's sums: sum[u] * units <=
               tau * total, total = the sums added in index order in float64.  A layer whose total is 0 is fully dormant and is
               LEFT ALONE (mask all zero, `skipped`): re-drawing a whole layer is a restart, not a recycle.  A window without rows
               has total 0 in every layer, so it recycles nothing
  elements     over the flat padded layout of paac_param_layout (conv HWIO, fc [in, H] behind the HWC flatten, heads [H, A] and
               [H, 1]); a pure function of the element's tensor, its index and the masks:
                 incoming   weight element [..., o] of layer l with mask_l[o]: a fresh draw from U(-d, d), d = 1 / sqrt(fan-in)
                 bias       element [o] with mask_l[o]: 0 (the published implementation's choice)
                 outgoing   element [..., c, :] of the NEXT layer's weights with mask_l[c]: 0 -- conv to conv the input-channel
                            slice, last conv to fc the rows p * C + c of every position p, fc to actor and critic row c
                 both       0: outgoing wins (the published code zeroes second)
               every other element, and all padding, keeps its bits
  draw         philox4x32-10 (evaluation.philox_word0) on counter (flat index lo, flat index hi, event, STREAM), key (seed lo,
               seed hi); the seed is the run's random_seed, events count recycles from 1.  In float32, in this order:
               d = float32(1 / sqrt(float64(fan-in))); u = float32(word0 >> 8) * 2^-24 (exact); prod = (d + d) * u; x = -d + prod
  slots        a rewritten element (drawn or zeroed) gets a fresh run's slot values: RMSProp ms = 1, mom = 0; Adam m = v = 0
               (Adam's two bias-correction powers are global and stay)
"""
import numpy as np

from . import evaluation, feature_stats

STREAM = 0x5245444F                # "REDO": the fourth counter word
RMSPROP, ADAM = 0, 1               # PAAC_REDO_RMSPROP, PAAC_REDO_ADAM
OPTIMIZERS = {"rmsprop": RMSPROP, "adam": ADAM}
FRESH_SLOTS = {RMSPROP: (1.0, 0.0), ADAM: (0.0, 0.0)}


def masks(feature_layout, block, tau):
    """-> (mask int32[U], {layer name: dict(units, recycled, skipped)}) of the window in `block` (a feature_stats.Block)."""
    lay, tau = feature_layout, np.float64(tau)
    mask, layers = np.zeros(lay.U, dtype=np.int32), {}
    for _, name, units, at in lay.layers():
        sums = block.get("sum")[at:at + units]
        total = np.float64(0.0)
        for v in sums:
            total = total + v
        skipped = bool(total == 0.0)
        if not skipped:
            mask[at:at + units] = sums * np.float64(units) <= tau * total
        layers[name] = dict(units=int(units), recycled=int(mask[at:at + units].sum()), skipped=skipped)
    return mask, layers


def feature_layout_of(layout):
    """The feature_stats.Layout of a parameter layout (paac_param_layout's dict): the last axis of every conv / fc weight tensor."""
    nconv = (len(layout["tensors"]) - 6) // 2
    units = [layout["tensors"][2 * i]["shape"][-1] for i in range(nconv)]
    return feature_stats.Layout(units + [0] * (3 - nconv) + [layout["tensors"][2 * nconv]["shape"][-1]])


def tensor_rules(layout):
    """-> [(tensor dict, kind, out_off, in_off, cin, fan_in)] of the tensors a recycle can touch, in layout order.  kind "w" / "b";
    out_off / in_off: where the mask holds the tensor's unit axis / its rows' input units (None: no such rule); the input unit
    of row r of a weight tensor seen as [rows, width] is r % cin."""
    present = feature_layout_of(layout).layers()
    rules, tensors = [], layout["tensors"]
    for i, (_, _, units, at) in enumerate(present):
        w, b = tensors[2 * i], tensors[2 * i + 1]
        assert w["shape"][-1] == units and b["shape"] == (units,), (w, b, units)
        fan_in = int(np.prod(w["shape"][:-1]))
        before = present[i - 1] if i else None
        rules.append((w, "w", at, before[3] if before else None, before[2] if before else 1, fan_in))
        rules.append((b, "b", at, None, 1, fan_in))
    _, _, H, at = present[-1]
    for t in (tensors[2 * len(present)], tensors[2 * len(present) + 2]):          # actor and critic weights
        assert t["shape"][0] == H, t
        rules.append((t, "w", None, at, H, H))
    return rules


def draw(seed, event, flat_index, fan_in):
    """The fresh values of the elements at `flat_index` (their places in the flat padded buffer) at recycle `event`."""
    idx = np.asarray(flat_index, dtype=np.uint64)
    hi = idx >> np.uint64(32)
    assert not hi.any() and 1 <= int(event) <= 0xFFFFFFFF          # (counter word 1 is the index's high half: 0 below 2^32 floats)
    word0 = evaluation.philox_word0(seed, int(event) << 32, idx & np.uint64(0xFFFFFFFF), STREAM)
    d = np.float32(1.0 / np.sqrt(np.float64(fan_in)))
    u = (word0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    prod = (d + d) * u
    return (-d + prod).astype(np.float32)


def recycle(layout, params, slots, mask, seed, event, optimizer):
    """One recycle in place: params float32[total], slots (slot0, slot1) of the same layout, mask from `masks` ->
    dict(parameters_redrawn, parameters_zeroed)."""
    fresh = FRESH_SLOTS[optimizer]
    redrawn = zeroed = 0
    for t, kind, out_off, in_off, cin, fan_in in tensor_rules(layout):
        width = t["shape"][-1]
        e = np.arange(t["size"])
        row, col = e // width, e % width
        incoming = mask[out_off + col] != 0 if out_off is not None else np.zeros(t["size"], dtype=bool)
        outgoing = mask[in_off + row % cin] != 0 if in_off is not None else np.zeros(t["size"], dtype=bool)
        zero = outgoing | incoming if kind == "b" else outgoing
        drawn = incoming & ~zero
        where = t["offset"] + e
        params[where[drawn]] = draw(seed, event, where[drawn], fan_in)
        params[where[zero]] = np.float32(0.0)
        for slot, value in zip(slots, fresh):
            slot[where[drawn | zero]] = np.float32(value)
        redrawn += int(drawn.sum())
        zeroed += int(zero.sum())
    return dict(parameters_redrawn=redrawn, parameters_zeroed=zeroed)


def parameter_counts(layout, mask):
    """What `recycle` returns, from the mask alone (the record's parameters_redrawn / parameters_zeroed)."""
    redrawn = zeroed = 0
    for t, kind, out_off, in_off, cin, _ in tensor_rules(layout):
        width = t["shape"][-1]
        rows = t["size"] // width
        n_out = int(mask[out_off:out_off + width].sum()) if out_off is not None else 0
        rows_out = rows // cin * int(mask[in_off:in_off + cin].sum()) if in_off is not None else 0
        if kind == "b":
            zeroed += n_out
        else:
            zeroed += rows_out * width
            redrawn += (rows - rows_out) * n_out
    return dict(parameters_redrawn=redrawn, parameters_zeroed=zeroed)


def record(layers, counts, tau, event):
    """The `redo` record's fields behind global_step."""
    return dict(event=int(event), tau=float(tau), layers=layers, skipped_layers=[n for n, l in layers.items() if l["skipped"]],
                **counts)


def layers_of_counts(feature_layout, counts):
    """paac_redo's counts_out int32[12] -> {layer name: dict(units, recycled, skipped)}."""
    c = np.asarray(counts).reshape(4, 3)
    return {name: dict(units=int(c[l, 1]), recycled=int(c[l, 0]), skipped=bool(c[l, 2])) for l, name, _, _ in feature_layout.layers()}


DATA_PARALLEL_REFUSAL = "--redo_every is not built into the data-parallel cycle (as --feature_stats, which it needs): run it on one GPU"


def check_flags(args, world=1):
    """-> W of --redo_every (0 = off); a Namespace from before the flag means off.  Refused: anything but an integer >= 0, W > 0
    without --feature_stats true, W > 0 with more than one data-parallel rank."""
    every = getattr(args, "redo_every", 0)
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 0:
        raise ValueError("--redo_every %r: expected an integer >= 0 (0 = off)" % (every,))
    if every > 0 and int(world) > 1:
        raise ValueError("%s (got %d ranks)" % (DATA_PARALLEL_REFUSAL, int(world)))
    if every > 0 and not feature_stats.check_flags(args, world)[0]:
        raise ValueError("--redo_every %d needs --feature_stats true: the recycle is decided from the window's per-unit sums" % every)
    return int(every)
