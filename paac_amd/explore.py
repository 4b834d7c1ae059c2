"""A count-based exploration bonus: `--explore_bonus BETA` adds BETA / sqrt(n) to every reward of the device loop's rollout, n =
how often a SimHash code of the observation the step arrived in has been seen in this run ("#Exploration", Tang et al., arXiv
1611.04717).  One launch per cycle, behind the rollout and in front of everything that reads the rewards plane; eager or captured.

This is the SPEC; the same bits are produced
  * on the host by the plain-numpy functions below (`signs`, `codes`, `slots`, `Twin.bonus`), and
  * on the device by paac_explore_signs / paac_explore_bonus (csrc/explore.h, instantiated in csrc/misc.hip; include/paac_hip.h
    has the contract).

Spec
  input        the NEXT observations of the cycle's rollout rows: row t * N + e is states[slot(t) + 1, e], the stack step t arrived
               in -- contiguous in the observation ring (states[parity * T + 1 : parity * T + T + 1]).  Each is K = 84 * 84 * 4 =
               28224 bytes in memory order
  centring     xc[k] = int8(x[k] ^ 0x80), i.e. x - 128
  signs        S[k, j] in {-1, +1}, k < 28224, j < 64: bit j % 32 of word 0 of philox4x32-10 (evaluation.philox_word0) on counter
               (k, j // 32, 0, STREAM), key (seed lo, seed hi); a set bit is +1.  seed = the run's random_seed
  projection   P[r, j] = sum_k xc[r, k] * S[k, j], exact in int32 (|P| <= 28224 * 128)
  code         code[r] = sum over j < bits of (P[r, j] >= 0) << j, bits in 1..64
  slot         slot[r] = finalise(code[r]) >> (64 - table_bits), table_bits in 4..26; finalise = splitmix64's finaliser, in uint64
               arithmetic: z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31).
               Colliding codes share a counter, as in the paper
  counts       int32[2 ** table_bits], zero at the start of a run, persistent across cycles, NOT checkpointed: a resumed run
               starts with an empty table
  bonus        two phases per call, so that the order of rows does not matter: every row adds 1 to its slot; then every row reads
               n = counts[slot[r]] with all of the call's increments in it, bonus[r] = float32(beta) / sqrt(float32(n)) -- both
               operations correctly rounded in float32 -- and rewards[r] += bonus[r].  bonus also goes to a [T, N] plane of its own
  scores       ep_reward, the finished-episode ring and --eval_every stay extrinsic: the step has accounted them before the bonus
               exists.  The rewards plane the returns and --window_stats read is the shaped one
"""
import math

import numpy as np

from . import evaluation

STREAM = 0x4558504C                # "EXPL": the fourth counter word (csrc/explore.h: kExpStream)
K, COLUMNS = 84 * 84 * 4, 64
BITS_RANGE, TABLE_BITS_RANGE = (1, 64), (4, 26)


def signs(seed):
    """-> S int8[K, 64] of `seed`."""
    k = np.arange(K)
    words = [evaluation.philox_word0(seed, half, k, STREAM) for half in range(COLUMNS // 32)]
    bit = np.concatenate([(w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1) for w in words], axis=1)
    return (2 * bit.astype(np.int8) - 1).astype(np.int8)


def project(states, S):
    """uint8 [rows, ...28224 bytes] -> P int64[rows, 64].  (Through float64: every product and partial sum is an integer below
    2 ** 22, so the sum is exact in any order.)"""
    xc = (np.asarray(states, dtype=np.uint8).reshape(-1, K) ^ np.uint8(0x80)).view(np.int8)
    S = S.astype(np.float64)
    return np.concatenate([(xc[r:r + 256].astype(np.float64) @ S).astype(np.int64) for r in range(0, len(xc), 256)])


def codes(P, bits):
    """-> uint64[rows]."""
    set_bits = (np.asarray(P)[:, :bits] >= 0).astype(np.uint64)
    return (set_bits << np.arange(bits, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def finalise(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def slots(code, table_bits):
    """-> int64[rows] in [0, 2 ** table_bits)."""
    return (finalise(code) >> np.uint64(64 - table_bits)).astype(np.int64)


class Twin(object):
    """The table of a run and the bonus of one call after another."""

    def __init__(self, seed, bits, table_bits):
        self.S, self.bits, self.table_bits = signs(seed), int(bits), int(table_bits)
        self.counts = np.zeros(1 << self.table_bits, dtype=np.int32)

    def bonus(self, states, beta, rewards=None):
        """One call on uint8 states [rows, ...] -> (codes uint64[rows], bonus float32[rows]); rewards float32[rows] is added to
        in place."""
        code = codes(project(states, self.S), self.bits)
        at = slots(code, self.table_bits)
        np.add.at(self.counts, at, 1)
        bonus = (np.float32(beta) / np.sqrt(self.counts[at].astype(np.float32))).astype(np.float32)
        if rewards is not None:
            rewards += bonus
        return code, bonus


def record(beta, bits, table_bits, bonus, occupied):
    """The `explore` record's fields behind global_step; bonus: the last rollout's plane."""
    return dict(beta=float(beta), bits=int(bits), table_bits=int(table_bits), bonus_mean=float(np.mean(bonus, dtype=np.float64)),
                bonus_max=float(np.max(bonus)), occupied_slots=int(occupied))


DATA_PARALLEL_REFUSAL = "--explore_bonus is not built into the data-parallel cycle (the table is rank-local): run it on one GPU"


def check_flags(args, world=1):
    """-> (beta, bits, table_bits) of --explore_bonus / --explore_bits / --explore_table_bits; beta 0 = off, and a Namespace from
    before the flags means off.  Refused: a beta that is negative or not finite, bits outside 1..64, table_bits outside 4..26;
    beta > 0 with --host_environments true (the host loop keeps no observation ring on the device) or with more than one
    data-parallel rank."""
    beta, found = getattr(args, "explore_bonus", 0.0), []
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not (
            math.isfinite(beta) and beta >= 0 and np.isfinite(np.float32(beta))):
        raise ValueError("--explore_bonus %r: expected a finite value >= 0 (0 = off)" % (beta,))
    for flag, default, (lo, hi) in (("explore_bits", 32, BITS_RANGE), ("explore_table_bits", 20, TABLE_BITS_RANGE)):
        v = getattr(args, flag, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("--%s %r: expected an integer in [%d, %d]" % (flag, v, lo, hi))
        found.append(int(v))
    if beta > 0 and getattr(args, "host_environments", False):
        raise ValueError("--explore_bonus %g needs the device loop: with --host_environments true no observation ring is kept on "
                         "the GPU" % beta)
    if beta > 0 and int(world) > 1:
        raise ValueError("%s (got %d ranks)" % (DATA_PARALLEL_REFUSAL, int(world)))
    return float(beta), found[0], found[1]
