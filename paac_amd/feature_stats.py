"""Feature statistics of the trunk: `--feature_stats true` folds every cycle's training activations -- the conv outputs and the
fc activations of the T * N rollout rows, as forwarded on the pre-update weights -- into one block of running accumulators on
the GPU, and the trainer writes one `features` record per `progress` record from it: the share of dormant units of every layer
(Sokar et al., arXiv 2302.12902) and the effective rank of the fc features (Kumar et al., arXiv 2010.14498).

This is the SPEC of the block, of the fold and of the record; the same numbers are produced
  * on the host by the plain-numpy `fold` / `finish` / `summary` below, and
  * on the device by paac_feature_fold / paac_feature_fold_ctx / paac_feature_finish (csrc/feature_stats.h, instantiated in
    csrc/misc.hip; include/paac_hip.h has the contract).  The fold only reads the activations: training is bit-identical
    with the flag on or off.

Spec
  layers       conv1, conv2 [, conv3], fc.  A conv CHANNEL is a unit, its samples are rows x output positions; an fc column is
               a unit, its samples are rows.  Activations are post-ReLU float32
  block        two arrays, acc_f float64 and acc_i int64, laid out by Layout(units): FIELDS_F / FIELDS_I map a field's name to
               (offset, length).  The live fields -- sum, gram / cycles, rows, samples, pos -- are the window's state: all zero
               bytes = an empty window.  The trailing part_* fields are the fold's scratch (per-workgroup partials between
               its launches): any content, never read before it is written
  unit sums    sum[u] += the unit's activations, every term converted to float64 before it is added (UNIT_FP32_TERMS = 1);
               pos[u] += the number of samples > 0.  The order of the float64 additions is fixed (thread-strided, then
               workgroups ascending), so two runs agree to the bit; the twin adds in numpy's order
  gram         G += H^T H over the fc activations, uncentred, the full symmetric matrix stored.  Rows are cut into chunks of
               CHUNK_ROWS; inside a chunk products and sums are float32 (fp32 matrix instructions on the device, a float32
               matmul here), chunk results are added in ascending order in float64, in up to GRAM_SPLITS_MAX contiguous
               groups of chunks whose float64 sums are then added in ascending order into the block.  Element (i, j), i <= j,
               is computed once and added to both G[i, j] and G[j, i]: the matrix is symmetric to the bit
  finish       trace and squared Frobenius norm of G in window_stats.strided_sum's order (squares rounded once); per layer
               total = the units' sums added in index order; unit u is dormant when sum[u] * units <= tau * total (its mean
               over the layer's mean of means is at most tau; a layer whose total is 0 is fully dormant), dead when pos[u] == 0
"""
import numpy as np

from .window_stats import strided_sum

CHUNK_ROWS = 128            # rows whose products are summed in float32 (hip_ops.FEATURE_CHUNK_ROWS is the library's)
GRAM_SPLITS_MAX = 8         # groups of chunks = workgroups along the rows of one tile
UNIT_WGS = 256              # workgroups per layer of the unit statistics at most
UNIT_FP32_TERMS = 1         # terms of a unit sum added in float32 before float64 takes over: every term is converted first
LAYER_NAMES = ("conv1", "conv2", "conv3", "fc")
FINISH_SCALARS = 20         # trace, frobenius^2, {dormant, dead, pos total} per layer slot, rows, cycles, samples per slot


def _table(entries):
    table, at = {}, 0
    for name, length in entries:
        table[name] = (at, length)
        at += length
    return table, at


class Layout(object):
    """The block of one geometry.  units: the unit count of each of the four layer slots (conv1, conv2, conv3, fc); 0 = the
    geometry has no such layer."""

    def __init__(self, units):
        self.units = tuple(int(u) for u in units)
        if len(self.units) != 4 or self.units[3] < 64 or self.units[3] % 64 or self.units[3] > 1024:
            raise ValueError("feature_stats.Layout: units %r (four slots, the fc width a multiple of 64 up to 1024)" % (units,))
        if any(u % 16 or u > 1024 for u in self.units[:3]):
            raise ValueError("feature_stats.Layout: channel counts %r must be multiples of 16 up to 1024" % (self.units[:3],))
        self.H = self.units[3]
        self.U = sum(self.units)
        self.unit_offset = tuple(int(v) for v in np.cumsum((0,) + self.units[:3]))
        n32 = self.H // 32
        self.tiles = n32 * (n32 + 1) // 2
        self.FIELDS_F, self.N_F = _table([("sum", self.U), ("gram", self.H * self.H),
                                          ("part_gram", GRAM_SPLITS_MAX * self.tiles * 1024), ("part_sum", UNIT_WGS * self.U)])
        self.FIELDS_I, self.N_I = _table([("cycles", 1), ("rows", 1), ("samples", 4), ("pos", self.U),
                                          ("part_pos", UNIT_WGS * self.U)])
        self.LIVE_F = self.FIELDS_F["part_gram"][0]
        self.LIVE_I = self.FIELDS_I["part_pos"][0]

    @classmethod
    def of_geometry(cls, convs, fc):
        """convs: [(filters, size, stride), ...] (hip_ops.arch_geometry)."""
        filters = [int(c[0]) for c in convs]
        return cls(filters + [0] * (3 - len(filters)) + [int(fc)])

    def layers(self):
        """[(slot, name, units, offset of its units)] of the layers present."""
        return [(l, LAYER_NAMES[l], self.units[l], self.unit_offset[l]) for l in range(4) if self.units[l]]


class Block(object):
    """The live part of an accumulator block on the host (the scratch behind it is dropped)."""

    def __init__(self, layout, acc_f=None, acc_i=None):
        self.layout = layout
        self.f = np.zeros(layout.LIVE_F, dtype=np.float64)
        self.i = np.zeros(layout.LIVE_I, dtype=np.int64)
        if acc_f is not None:
            self.f[:] = np.asarray(acc_f, dtype=np.float64).reshape(-1)[:layout.LIVE_F]
        if acc_i is not None:
            self.i[:] = np.asarray(acc_i, dtype=np.int64).reshape(-1)[:layout.LIVE_I]

    def get(self, name):
        table, array = (self.layout.FIELDS_F, self.f) if name in self.layout.FIELDS_F else (self.layout.FIELDS_I, self.i)
        at, length = table[name]
        return array[at] if length == 1 else array[at:at + length]

    def gram(self):
        return self.get("gram").reshape(self.layout.H, self.layout.H)


def gram_groups(rows):
    """-> [(first row, end row)] of the groups of chunks one fold of `rows` rows adds in float64, in order."""
    chunks = -(-int(rows) // CHUNK_ROWS)
    per = -(-chunks // GRAM_SPLITS_MAX)
    return [(g * per * CHUNK_ROWS, min((g + 1) * per * CHUNK_ROWS, int(rows))) for g in range(-(-chunks // per))]


def fold(acc, activations):
    """One cycle's contribution to the Block `acc`.  activations: one array per layer slot (None where the layout has no such
    layer): conv outputs [R, OH, OW, C], fc activations [R, H], float32."""
    lay = acc.layout
    h = np.ascontiguousarray(np.asarray(activations[3], dtype=np.float32))
    R = h.shape[0]
    if R < 1 or h.shape != (R, lay.H):
        raise ValueError("feature_stats.fold: fc activations %r, expected [rows >= 1, %d]" % (h.shape, lay.H))
    for l, _, units, at in lay.layers():
        if activations[l] is None:
            continue
        a = np.asarray(activations[l], dtype=np.float32)
        if a.shape[0] != R or a.shape[-1] != units:
            raise ValueError("feature_stats.fold: layer %s of shape %r, expected [%d, ..., %d]" % (LAYER_NAMES[l], a.shape, R, units))
        a = a.reshape(-1, units)
        acc.get("sum")[at:at + units] += a.astype(np.float64).sum(axis=0)
        acc.get("pos")[at:at + units] += (a > 0).sum(axis=0)
        acc.get("samples")[l] += a.shape[0]
    total = np.zeros((lay.H, lay.H), dtype=np.float64)
    for first, end in gram_groups(R):
        group = np.zeros((lay.H, lay.H), dtype=np.float64)
        for c0 in range(first, end, CHUNK_ROWS):
            chunk = h[c0:min(c0 + CHUNK_ROWS, end)]
            group = group + np.matmul(chunk.T, chunk).astype(np.float64)      # float32 products and sums inside a chunk
        total = total + group
    upper = np.triu(total)
    acc.gram()[:] += upper + np.triu(total, 1).T
    acc.i[lay.FIELDS_I["cycles"][0]] += 1
    acc.i[lay.FIELDS_I["rows"][0]] += R
    return acc


def finish(acc, tau):
    """-> float64[FINISH_SCALARS]: what paac_feature_finish computes from a block, in its order (integers are exact)."""
    lay = acc.layout
    out = np.zeros(FINISH_SCALARS, dtype=np.float64)
    G = acc.gram()
    out[0] = strided_sum(np.diagonal(G))
    out[1] = strided_sum(G.reshape(-1) * G.reshape(-1))
    tau = np.float64(tau)
    for l, _, units, at in lay.layers():
        sums, pos = acc.get("sum")[at:at + units], acc.get("pos")[at:at + units]
        total = np.float64(0.0)
        for v in sums:
            total = total + v
        out[2 + 3 * l] = int((sums * np.float64(units) <= tau * total).sum())
        out[3 + 3 * l] = int((pos == 0).sum())
        out[4 + 3 * l] = int(pos.sum())
    out[14], out[15] = acc.get("rows"), acc.get("cycles")
    out[16:20] = acc.get("samples")
    return out


def spectrum(gram):
    """-> (fc_srank, fc_top_eigen_share) of a downloaded Gram matrix; (None, None) when its trace is 0."""
    lam = np.maximum(np.linalg.eigvalsh(np.asarray(gram, dtype=np.float64)), 0.0)[::-1]
    if not lam.sum() > 0.0:
        return None, None
    sigma = np.sqrt(lam)
    share = np.cumsum(sigma) / sigma.sum()
    return int(min(np.searchsorted(share, 0.99) + 1, sigma.size)), float(lam[0] / lam.sum())


def summary(layout, scalars, tau, gram=None):
    """The `features` record of a window: plain floats and ints.  scalars: paac_feature_finish's output for the window's block
    and tau (or finish(block, tau), its twin); gram: the window's downloaded Gram matrix where the spectrum is due -- adds
    fc_srank / fc_top_eigen_share."""
    s = np.asarray(scalars, dtype=np.float64).reshape(FINISH_SCALARS)
    out = dict(cycles=int(s[15]), rows=int(s[14]), tau=float(tau), layers={})
    for l, name, units, _ in layout.layers():
        n = int(s[16 + l])
        out["layers"][name] = dict(units=units, dormant_fraction=float(s[2 + 3 * l] / units), dead_fraction=float(s[3 + 3 * l] / units),
                                   active_fraction=float(s[4 + 3 * l] / (n * units)) if n else None)
    out["fc_participation_ratio"] = float(s[0] * s[0] / s[1]) if s[0] > 0.0 else None
    if gram is not None:
        out["fc_srank"], out["fc_top_eigen_share"] = spectrum(gram)
    return out


DATA_PARALLEL_REFUSAL = ("--feature_stats true is not built into the data-parallel cycle (the gradient exchange between the "
                         "backward and the optimizer step): run it on one GPU")


def check_flags(args, world=1):
    """-> (on?, tau, rank_every) of --feature_stats / --dormant_tau / --feature_rank_every; a Namespace from before the flags
    means off.  Anything but True / False, a tau that is not a finite number in [0, 1], a negative or fractional rank_every and
    the flag on with more than one data-parallel rank are refused."""
    on = getattr(args, "feature_stats", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("--feature_stats %r: expected true or false" % (on,))
    tau = getattr(args, "dormant_tau", 0.025)
    if isinstance(tau, (bool, np.bool_)) or not isinstance(tau, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(tau) <= 1.0:          # (NaN fails the comparison)
        raise ValueError("--dormant_tau %r: expected a finite number in [0, 1]" % (tau,))
    every = getattr(args, "feature_rank_every", 64)
    if isinstance(every, (bool, np.bool_)) or not isinstance(every, (int, np.integer)) or every < 0:
        raise ValueError("--feature_rank_every %r: expected an integer >= 0 (0 = never)" % (every,))
    if on and int(world) > 1:
        raise ValueError("%s (got %d ranks)" % (DATA_PARALLEL_REFUSAL, int(world)))
    return bool(on), float(tau), int(every)
