"""A learned exploration bonus: `--explore_kind rnd` makes `--explore_bonus BETA` the scale of a Random Network Distillation
bonus (Burda et al., arXiv 1810.12894) instead of SimHash's count bonus (paac_amd/explore.py): a predictor network is trained
online, on the GPU and inside the captured cycle, to reproduce a fixed random target network on the observations the rollout
arrives in, and its error -- large where the predictor has seen little -- is the bonus.  Three launches per cycle, where
SimHash's one stands.

This is the SPEC; the same numbers are produced
  * on the host in float64 by `pool`, `forward`, `gradient` and `Twin.bonus` below, and
  * on the device by paac_rnd_bonus (csrc/rnd.h, instantiated in csrc/misc.hip; include/paac_hip.h has the contract) on fp32
    matrix instructions: the device agrees with the twin to fp32 accumulation error (tests/test_rnd_gpu.py has the bars).

Spec
  input        SimHash's rows: the T * N NEXT stacks of the cycle, states[parity * T + 1 : parity * T + T + 1], 28224 bytes each.
               Only the newest frame is read (plane 3 of the [84, 84, 4] stack), as in the paper
  features     a 14 x 14 thumbnail u[r, d], d = 14 * cy + cx, D = 196: s = the sum over dy, dx < 6 of x[r, 6 cy + dy, 6 cx + dx, 3],
               an exact integer of at most 9180; u = float32(s) / float32(9180).  The device games are boards of 6 x 6-pixel
               cells, so nothing is lost there; for other frames it is a thumbnail.  A design choice, not the paper's conv net
  networks     target and predictor have one shape: h = relu(u W1 + b1), o = h W2 + b2; W1 [196, 256], b1 [256], W2 [256, 64],
               b2 [64], flat in this order: NET = 66880 floats.  Both are drawn once on the host: element i of the flat buffer is
               U(-d, d), d = 1 / sqrt(fan-in) (196 for W1 and b1, 256 for W2 and b2), by redo.py's draw law on word 0 of
               philox4x32-10 (evaluation.philox_word0) on counter (i, 0, 0, STREAM), key the run's random_seed; STREAM is
               TARGET_STREAM or PREDICTOR_STREAM
  per call     1. forward of both nets on all R rows with the predictor's PRE-step weights; e = o_p - o_t;
                  raw[r] = (1 / 64) sum_j e[r, j] ** 2
               2. normaliser: m, a running mean of raw ** 2 -- the first call of a run sets m = mean_r raw[r] ** 2, every later one
                  m = 0.99 m + 0.01 mean_r raw[r] ** 2 (0.99: a design choice).  The state is two doubles, m and the call count.
                  The device takes the mean in float64 in a fixed order: lane l of one wave adds the rows l, l + 64, ... in
                  ascending order, then the 64 partials are added in lane order
               3. bonus[r] = float32(beta * raw[r] / (sqrt(m) + 1e-8)); rewards[r] += bonus[r]; bonus also goes to a [T, N] plane
               4. predictor step: L = (1 / R) sum_r raw[r]; exact gradients of the four predictor tensors, then textbook
                  bias-corrected Adam (t = the call count after this call): mom = b1 mom + (1 - b1) g; var = b2 var + (1 - b2) g g;
                  w -= lr * (mom / (1 - b1 ** t)) / (sqrt(var / (1 - b2 ** t)) + eps).  lr is --rnd_lr; b1 = 0.9, b2 = 0.999 and
                  eps = 1e-8 are arguments of the entry and no flags
  scores       stay extrinsic, as under SimHash
  not kept     the predictor, its Adam slots and the normaliser are NOT checkpointed: a resumed run starts a fresh predictor
"""
import math

import numpy as np

from . import evaluation

TARGET_STREAM, PREDICTOR_STREAM = 0x524E4454, 0x524E4450          # "RNDT", "RNDP": the fourth counter word
D, HIDDEN, OUT, CELL = 196, 256, 64, 6
W1, B1, W2, B2, NET = 0, D * HIDDEN, D * HIDDEN + HIDDEN, D * HIDDEN + HIDDEN + HIDDEN * OUT, D * HIDDEN + HIDDEN + HIDDEN * OUT + OUT
DECAY, BETA1, BETA2, EPS = 0.99, 0.9, 0.999, 1e-8
KINDS = ("simhash", "rnd")


def draw(seed, stream):
    """-> float32[NET]: a net of `seed` on `stream`, flat."""
    i = np.arange(NET)
    word0 = evaluation.philox_word0(seed, 0, i, stream)
    d = (1.0 / np.sqrt(np.where(i < W2, np.float64(D), np.float64(HIDDEN)))).astype(np.float32)
    u = (word0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (-d + (d + d) * u).astype(np.float32)


def tensors(flat):
    """Views (W1, b1, W2, b2) of a flat net."""
    return flat[W1:B1].reshape(D, HIDDEN), flat[B1:W2], flat[W2:B2].reshape(HIDDEN, OUT), flat[B2:NET]


def pool(states):
    """uint8 [rows, ...28224 bytes] -> u float32[rows, 196]."""
    x = np.asarray(states, dtype=np.uint8).reshape(-1, 84, 84, 4)[..., 3].astype(np.int64)
    s = x.reshape(-1, 14, CELL, 14, CELL).sum(axis=(2, 4)).reshape(-1, D)
    return s.astype(np.float32) / np.float32(CELL * CELL * 255)


def forward(u, flat):
    """-> (h, o) of the net `flat` on features u, in the dtype of u."""
    w1, b1, w2, b2 = tensors(flat)
    h = np.maximum(u @ w1 + b1, 0)
    return h, h @ w2 + b2


def loss(u, target, predictor):
    """L = (1 / R) sum_r raw[r]."""
    e = forward(u, predictor)[1] - forward(u, target)[1]
    return (e * e).mean(axis=1).mean()


def gradient(u, target, predictor):
    """-> (raw [rows], dL/d predictor flat [NET]) in the dtype of u."""
    h, o = forward(u, predictor)
    e = o - forward(u, target)[1]
    w2 = tensors(predictor)[2]
    do = e * u.dtype.type(2.0 / (OUT * len(u)))
    dh = (do @ w2.T) * (h > 0)
    return (e * e).mean(axis=1), np.concatenate([(u.T @ dh).ravel(), dh.sum(axis=0), (h.T @ do).ravel(), do.sum(axis=0)])


class Twin(object):
    """Both nets, the Adam slots and the normaliser of a run, and the bonus of one call after another.  dtype: float64 is the
    specification; float32 (numpy float32 matmuls) measures what fp32 accumulation costs (tests/test_rnd_gpu.py)."""

    def __init__(self, seed, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.target, self.predictor = draw(seed, TARGET_STREAM).astype(dtype), draw(seed, PREDICTOR_STREAM).astype(dtype)
        self.mom, self.var = np.zeros(NET, dtype), np.zeros(NET, dtype)
        self.m, self.calls = 0.0, 0

    def bonus(self, states, beta, lr, rewards=None, beta1=BETA1, beta2=BETA2, eps=EPS):
        """One call on uint8 states [rows, ...] -> (raw, bonus float32[rows], gradient [NET]); rewards float32[rows] is added
        to in place; the predictor is stepped."""
        ty = self.dtype.type
        raw, g = gradient(pool(states).astype(self.dtype), self.target, self.predictor)
        mean = float(np.mean(raw.astype(np.float64) ** 2))
        self.m = mean if self.calls == 0 else DECAY * self.m + (1.0 - DECAY) * mean
        self.calls += 1
        bonus = (float(beta) * raw.astype(np.float64) / (math.sqrt(self.m) + 1e-8)).astype(np.float32)
        if rewards is not None:
            rewards += bonus
        self.mom = ty(beta1) * self.mom + ty(1.0 - beta1) * g
        self.var = ty(beta2) * self.var + ty(1.0 - beta2) * g * g
        c1, c2 = ty(1.0 / (1.0 - beta1 ** self.calls)), ty(1.0 / (1.0 - beta2 ** self.calls))
        self.predictor = self.predictor - ty(lr) * (self.mom * c1) / (np.sqrt(self.var * c2) + ty(eps))
        return raw, bonus, g


def record(beta, lr, bonus, raw, m):
    """The `explore` record's fields behind global_step under rnd; bonus, raw: the last rollout's planes; m: the normaliser.
    (`explore_kind`, not `kind`: in metrics.jsonl `kind` is the record's own type, "explore".)"""
    return dict(explore_kind="rnd", beta=float(beta), lr=float(lr), bonus_mean=float(np.mean(bonus, dtype=np.float64)),
                bonus_max=float(np.max(bonus)), error_mean=float(np.mean(raw, dtype=np.float64)),
                error_rms_running=float(math.sqrt(m)))


DATA_PARALLEL_REFUSAL = "--explore_kind rnd is not built into the data-parallel cycle (the predictor is rank-local): run it on one GPU"


def check_flags(args, world=1):
    """-> (kind, lr) of --explore_kind / --rnd_lr; a Namespace from before the flags means simhash.  Refused: a kind that is
    neither simhash nor rnd, an lr that is not finite and > 0; rnd with --explore_bonus > 0 and --host_environments true (the
    host loop keeps no observation ring on the device) or more than one data-parallel rank."""
    kind, lr = getattr(args, "explore_kind", "simhash"), getattr(args, "rnd_lr", 1e-4)
    if kind not in KINDS:
        raise ValueError("--explore_kind %r: expected one of %s" % (kind, ", ".join(KINDS)))
    if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not (math.isfinite(lr) and lr > 0):
        raise ValueError("--rnd_lr %r: expected a finite value > 0" % (lr,))
    beta = getattr(args, "explore_bonus", 0.0)
    if kind == "rnd" and isinstance(beta, (int, float)) and beta > 0:
        if getattr(args, "host_environments", False):
            raise ValueError("--explore_kind rnd needs the device loop: with --host_environments true no observation ring is "
                             "kept on the GPU")
        if int(world) > 1:
            raise ValueError("%s (got %d ranks)" % (DATA_PARALLEL_REFUSAL, int(world)))
    return kind, float(lr)
