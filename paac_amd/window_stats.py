"""Per-window training statistics: `--window_stats true` folds every cycle's rollout, update and finished episodes into one
small block of running accumulators on the GPU, and the trainer writes one `window` record per `progress` record from it.

This is the SPEC of the block and of the fold; the same numbers are produced
  * on the host by the plain-numpy `fold` / `fold_episodes` below, and
  * on the device by paac_window_fold (csrc/misc.hip: window_fold_kernel; include/paac_hip.h has the contract), one launch of
    one workgroup per cycle, issued by paac.DeviceRollout behind the cycle's last optimizer step (inside the captured cycle)
    and by the host loop eagerly; one process only -- with data parallelism's gradient exchange on, the flag is refused.  The
    fold only reads what the cycle left behind: training is bit-identical with it on or off.

Spec
  block        two arrays: acc_f float64[N_F] and acc_i int64[N_I]; FIELDS_F / FIELDS_I map a field's name to (offset, length)
               and nothing else names an offset.  A block of all zero bytes is an empty window
  rows         a cycle has B = T * N rows, row t * N + n.  Thread i of THREADS = 256 takes rows i, i + 256, ... in that order
               and accumulates each sum in float64 from the float32 inputs, every product and every sum a separate
               round-to-nearest operation (no fused multiply-add); the 256 partials of a sum are then added in index order,
               starting from 0.0, and the result is added to the block's field.  Squares of a float32 are exact in float64;
               (y - v) is rounded once and its square once.  Counts are integers
  update       loss[s] for the cycle's optimizer steps s < steps (row 0 from loss0 where given: a full-batch PPO cycle
               reports its first epoch through the learner's loss scalars), each column summed in step order; the ppo_stats
               columns over the steps s >= stats_first, column 2 (value_clip_fraction) only when live; opt_steps_applied counts
               applied[s] != 0 (all steps when there is no gate); grad_norm once per cycle
  episodes     the finished-episode ring {int32 count; int32 pad; float32 reward[4096]; int32 len[4096]}: entries j in
               [ring_cursor, count) live in slot j & 4095.  If count - ring_cursor > 4096 the overwritten entries are counted in
               episodes_dropped and only the surviving 4096 are folded.  Thread i takes surviving entries i, i + 256, ... in
               order, partials are combined in thread order.  Min and max are set by the fold that sees the window's first
               episode (episodes == 0 before it) and combined afterwards: the zeroing does not initialise them
  reset        a readout zeroes everything but ring_cursor (the last field of acc_i), which follows the ring, not the window
"""
import numpy as np

THREADS = 256
RING = 4096
MAX_ACTIONS = 32
MAX_STEPS = 64
LOSS_NAMES = ("loss", "actor_loss", "critic_loss", "entropy")
STAT_NAMES = ("clip_fraction", "approx_kl", "value_clip_fraction")


def _table(entries):
    table, at = {}, 0
    for name, length in entries:
        table[name] = (at, length)
        at += length
    return table, at


FIELDS_F, N_F = _table([
    ("sum_v", 1), ("sum_v2", 1), ("sum_y", 1), ("sum_y2", 1), ("sum_d", 1), ("sum_d2", 1), ("sum_adv", 1), ("sum_adv2", 1),
    ("max_abs_adv", 1), ("sum_reward", 1), ("sum_loss", 4), ("sum_stats", 3), ("sum_grad_norm", 1), ("max_grad_norm", 1),
    ("ep_return_sum", 1), ("ep_return_sq", 1), ("ep_length_sum", 1), ("ep_length_sq", 1), ("ep_return_min", 1),
    ("ep_return_max", 1), ("ep_length_min", 1), ("ep_length_max", 1)])
FIELDS_I, N_I = _table([
    ("cycles", 1), ("rows", 1), ("terminals", 1), ("truncated", 1), ("nonzero_rewards", 1), ("opt_steps", 1),
    ("opt_steps_applied", 1), ("stat_steps", 1), ("episodes", 1), ("episodes_dropped", 1), ("action_count", MAX_ACTIONS),
    ("ring_cursor", 1)])
# the eight row sums in block order (the kernel's partial index), then the ring's four
ROW_SUMS = ("sum_v", "sum_v2", "sum_y", "sum_y2", "sum_d", "sum_d2", "sum_adv", "sum_adv2", "sum_reward")
EPISODE_SUMS = ("ep_return_sum", "ep_return_sq", "ep_length_sum", "ep_length_sq")


class Block(object):
    """The accumulator block on the host: acc_f, acc_i and access by field name."""

    def __init__(self, acc_f=None, acc_i=None):
        self.f = np.zeros(N_F, dtype=np.float64) if acc_f is None else np.array(acc_f, dtype=np.float64).reshape(N_F)
        self.i = np.zeros(N_I, dtype=np.int64) if acc_i is None else np.array(acc_i, dtype=np.int64).reshape(N_I)

    def get(self, name):
        table, array = (FIELDS_F, self.f) if name in FIELDS_F else (FIELDS_I, self.i)
        at, length = table[name]
        return array[at] if length == 1 else array[at:at + length]

    def set(self, name, value):
        table, array = (FIELDS_F, self.f) if name in FIELDS_F else (FIELDS_I, self.i)
        at, length = table[name]
        array[at:at + length] = value

    def add(self, name, value):
        self.set(name, self.get(name) + value)

    def reset(self):
        """What a readout leaves: an empty window whose ring_cursor stays where the ring is."""
        cursor = self.get("ring_cursor")
        self.f[:] = 0.0
        self.i[:] = 0
        self.set("ring_cursor", cursor)

    def copy(self):
        return Block(self.f, self.i)


def strided_sum(terms):
    """The fold's order for one sum of float64 terms given in row order: thread i of THREADS adds terms i, i + THREADS, ...
    one after the other, then the THREADS partials are added in index order."""
    x = np.asarray(terms, dtype=np.float64).reshape(-1)
    passes = -(-x.size // THREADS) if x.size else 0
    padded = np.zeros(max(passes, 1) * THREADS, dtype=np.float64)          # (+ 0.0 changes no partial: they start at + 0.0)
    padded[:x.size] = x
    partial = np.zeros(THREADS, dtype=np.float64)
    for p in range(passes):
        partial = partial + padded[p * THREADS:(p + 1) * THREADS]
    total = np.float64(0.0)
    for v in partial:
        total = total + v
    return total


def _f32(a, n=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(-1)
    if n is not None and a.size != n:
        raise ValueError("window_stats.fold: a plane of %d elements, expected %d" % (a.size, n))
    return a


def fold_episodes(acc, returns, lengths):
    """The episode part of a fold on the new episodes given in order (float32 returns, integer lengths): the host loop's
    episodes, and the ring's surviving entries on the device."""
    r = np.asarray(returns, dtype=np.float32).astype(np.float64).reshape(-1)
    n = np.asarray(lengths, dtype=np.int64).astype(np.float64).reshape(-1)
    if r.size != n.size:
        raise ValueError("window_stats.fold_episodes: %d returns, %d lengths" % (r.size, n.size))
    if r.size == 0:
        return acc
    first = int(acc.get("episodes")) == 0
    for name, terms in zip(EPISODE_SUMS, (r, r * r, n, n * n)):
        acc.add(name, strided_sum(terms))
    for name, new, pick in (("ep_return_min", r.min(), min), ("ep_return_max", r.max(), max),
                            ("ep_length_min", n.min(), min), ("ep_length_max", n.max(), max)):
        acc.set(name, new if first else pick(acc.get(name), new))
    acc.add("episodes", r.size)
    return acc


def ring_entries(ring, cursor):
    """-> (count, dropped, returns, lengths): the entries of a finished-episode ring (int32 words, FINISHED_RING layout) that
    are new since `cursor`, in entry order, and how many were overwritten before they could be read."""
    ring = np.asarray(ring).view(np.int32).reshape(-1)
    count = int(ring[0])
    new = count - int(cursor)
    dropped = max(0, new - RING)
    slots = (np.arange(count - (new - dropped), count) & (RING - 1)).astype(np.int64)
    return count, dropped, ring[2:2 + RING].view(np.float32)[slots], ring[2 + RING:2 + 2 * RING][slots]


def fold(acc, cycle):
    """One cycle's contribution to the block `acc` (a Block), in the kernel's order.  `cycle`: T, N, A; the planes values,
    rewards, masks, actions, y, adv ([T, N] or [T*N]); truncs (None: no plane); loss [steps, 4] and loss0 (None, or [4]: row 0);
    ppo_stats ([steps, 2 or 3] or None) with stats_first; applied ([steps] or None); gnorm; ring (the finished-episode ring's
    int32 words, or None)."""
    T, N, A = int(cycle["T"]), int(cycle["N"]), int(cycle["A"])
    B = T * N
    if B < 1 or not 2 <= A <= MAX_ACTIONS:
        raise ValueError("window_stats.fold: T=%d N=%d A=%d" % (T, N, A))
    v, y, adv = (_f32(cycle[k], B).astype(np.float64) for k in ("values", "y", "adv"))
    r, m = _f32(cycle["rewards"], B), _f32(cycle["masks"], B)
    a = np.asarray(cycle["actions"], dtype=np.int64).reshape(-1)
    d = y - v
    for name, terms in zip(ROW_SUMS, (v, v * v, y, y * y, d, d * d, adv, adv * adv, r.astype(np.float64))):
        acc.add(name, strided_sum(terms))
    acc.set("max_abs_adv", max(acc.get("max_abs_adv"), np.abs(adv).max()))
    acc.add("terminals", int((m == 0.0).sum()))
    acc.add("nonzero_rewards", int((r != 0.0).sum()))
    if cycle.get("truncs") is not None:
        acc.add("truncated", int((_f32(cycle["truncs"], B) != 0.0).sum()))
    inside = (a >= 0) & (a < A)
    acc.add("action_count", np.bincount(a[inside], minlength=MAX_ACTIONS)[:MAX_ACTIONS])
    acc.add("cycles", 1)
    acc.add("rows", B)
    # the update
    loss = np.array(cycle["loss"], dtype=np.float32).reshape(-1, 4)
    steps = loss.shape[0]
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError("window_stats.fold: %d optimizer steps" % steps)
    if cycle.get("loss0") is not None:
        loss[0] = _f32(cycle["loss0"], 4)
    sums = np.zeros(4, dtype=np.float64)
    for s in range(steps):
        sums = sums + loss[s].astype(np.float64)
    acc.add("sum_loss", sums)
    acc.add("opt_steps", steps)
    applied = cycle.get("applied")
    acc.add("opt_steps_applied", steps if applied is None else int((np.asarray(applied).reshape(-1)[:steps] != 0).sum()))
    if cycle.get("ppo_stats") is not None:
        stats = np.asarray(cycle["ppo_stats"], dtype=np.float32).reshape(steps, -1)
        first = int(cycle.get("stats_first", 0))
        sums = np.zeros(3, dtype=np.float64)
        for s in range(first, steps):
            sums[:stats.shape[1]] = sums[:stats.shape[1]] + stats[s].astype(np.float64)
        acc.add("sum_stats", sums)
        acc.add("stat_steps", max(0, steps - first))
    g = np.float64(np.float32(np.asarray(cycle["gnorm"]).reshape(-1)[0]))
    acc.add("sum_grad_norm", g)
    acc.set("max_grad_norm", max(acc.get("max_grad_norm"), g))
    # the episodes
    if cycle.get("ring") is not None:
        count, dropped, returns, lengths = ring_entries(cycle["ring"], acc.get("ring_cursor"))
        fold_episodes(acc, returns, lengths)
        acc.add("episodes_dropped", dropped)
        acc.set("ring_cursor", count)
    return acc


def _moments(total, squares, n):
    """(mean, population std) from raw moments; (None, None) for an empty sum."""
    if n == 0:
        return None, None
    mean = total / n
    return float(mean), float(np.sqrt(max(0.0, squares / n - mean * mean)))


def summary(acc, num_actions=None, truncation=False, ppo=False, vclip=False):
    """The `window` record of a block: plain floats and ints (None where a mean has no terms).  num_actions: the length of
    action_freq (None: up to the last action played); truncation: the run carries a truncation plane; ppo: --ppo_epochs above
    1 (vclip: with --ppo_vclip on)."""
    g = acc.get
    rows, cycles, steps, episodes = int(g("rows")), int(g("cycles")), int(g("opt_steps")), int(g("episodes"))
    out = dict(cycles=cycles, rows=rows)
    v_mean, v_std = _moments(g("sum_v"), g("sum_v2"), rows)
    y_mean, y_std = _moments(g("sum_y"), g("sum_y2"), rows)
    d_mean, d_std = _moments(g("sum_d"), g("sum_d2"), rows)
    a_mean, a_std = _moments(g("sum_adv"), g("sum_adv2"), rows)
    ev = None
    if rows:
        var_y = g("sum_y2") / rows - (g("sum_y") / rows) ** 2
        var_d = g("sum_d2") / rows - (g("sum_d") / rows) ** 2
        ev = float(1.0 - var_d / var_y) if var_y > 0.0 else None
    mean = lambda total, n: float(total / n) if n else None
    out.update(explained_variance=ev, value_mean=v_mean, value_std=v_std, return_mean=y_mean, return_std=y_std,
               adv_mean=a_mean, adv_std=a_std, adv_abs_max=float(g("max_abs_adv")) if rows else None,
               reward_mean=mean(g("sum_reward"), rows), reward_nonzero_fraction=mean(float(g("nonzero_rewards")), rows),
               terminal_fraction=mean(float(g("terminals")), rows))
    if truncation:
        out["truncated_fraction"] = mean(float(g("truncated")), rows)
    counts = g("action_count")
    A = int(num_actions) if num_actions is not None else (int(np.nonzero(counts)[0].max()) + 1 if counts.any() else 0)
    out["action_freq"] = [float(c / rows) for c in counts[:A]] if rows else [None] * A
    for k, name in enumerate(LOSS_NAMES):
        out[name] = mean(g("sum_loss")[k], steps)
    out.update(grad_norm_mean=mean(g("sum_grad_norm"), cycles), grad_norm_max=float(g("max_grad_norm")) if cycles else None)
    if ppo:
        for k, name in enumerate(STAT_NAMES[:3 if vclip else 2]):
            out[name] = mean(g("sum_stats")[k], int(g("stat_steps")))
        out.update(opt_steps=steps, opt_steps_applied=int(g("opt_steps_applied")))
    r_mean, r_std = _moments(g("ep_return_sum"), g("ep_return_sq"), episodes)
    l_mean, _ = _moments(g("ep_length_sum"), g("ep_length_sq"), episodes)
    some = lambda name, kind: kind(g(name)) if episodes else None
    out.update(episodes=episodes, episodes_dropped=int(g("episodes_dropped")), episode_return_mean=r_mean,
               episode_return_min=some("ep_return_min", float), episode_return_max=some("ep_return_max", float),
               episode_return_std=r_std, episode_length_mean=l_mean, episode_length_min=some("ep_length_min", int),
               episode_length_max=some("ep_length_max", int))
    return out


DATA_PARALLEL_REFUSAL = ("--window_stats true is not built into the data-parallel cycle (the gradient exchange between the "
                         "backward and the optimizer step): run it on one GPU")


def check_flags(args, world=1):
    """--window_stats -> on?; anything but True / False is refused, a Namespace from before the flag means off.  On with more
    than one data-parallel rank is refused: the fold is not part of the data-parallel cycle."""
    on = getattr(args, "window_stats", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("--window_stats %r: expected true or false" % (on,))
    if on and int(world) > 1:
        raise ValueError("%s (got %d ranks)" % (DATA_PARALLEL_REFUSAL, int(world)))
    return bool(on)
