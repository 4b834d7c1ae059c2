// HBM-bound kernels of the PAAC hot path on gfx950: n-step returns, lr schedule, samplers,
// frame preprocessing / stacking, device-resident synthetic environments.  (Device games: games.hip; optimizer: optim.hip.)
#include "common.h"
#include "synth_dev.h"
#include "net_common.h"
#include "fc_heads.h"
#include "heads.h"

namespace paac {

#ifdef PAAC_DMM_STAMPS
__device__ unsigned long long* g_misc_stamps = nullptr;   // diagnostic build: phase stamps of the sampler workgroup
#define MISC_STAMP(i)                                                                       \
  do {                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    if (g_misc_stamps && threadIdx.x == 0) g_misc_stamps[(i)] = (unsigned long long)wall_clock64(); \
    __builtin_amdgcn_sched_barrier(0);                                                      \
  } while (0)
#else
#define MISC_STAMP(i)
#endif

// =============================================================================================
// The returns of one rollout, standalone: the n-step return (paac.py:140-149; fp64 scan like the reference's numpy buffers)
// or generalized advantage estimation, chosen at compile time.  One step is nstep_step / gae_step (common.h: the arithmetic
// contracts), shared with the scans inside the heads gradient kernels (heads.h).  gl = gamma * lambda, read by GAE alone.
// PLANE (--bootstrap_truncated): NoPlane -- the plain instantiations, whose code is what it was (the empty struct is one
// byte at the end of the kernel arguments, which no instruction reads) -- or the truncation plane's pointer: the scan then
// also loads the plane with the chunk and steps by nstep_step_tr / gae_step_tr.
struct NoPlane {};
template <int EST, class PLANE = NoPlane>
__global__ void returns_scan_kernel(const float* __restrict__ v_boot, const float* __restrict__ rewards,
                                    const float* __restrict__ masks, const float* __restrict__ values, int T, int N,
                                    double gamma, double gl, float* __restrict__ y, float* __restrict__ adv,
                                    const CycleTick ct, const PLANE truncs) {
  constexpr bool TR = !std::is_same<PLANE, NoPlane>::value;
  // 128 threads: wave 0 scans 64 environments, wave 1 of workgroup 0 does the cycle bookkeeping -- its
  // read-modify-write round trip runs beside the scan's instead of in front of it
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  if (threadIdx.x >= 64) {
    if (blockIdx.x == 0 && threadIdx.x == 64) cycle_tick(ct);
    return;
  }
  if (e >= N) return;
  // The scan is serial in t but its inputs are not: each chunk of CH steps is requested at once (one memory round
  // trip per chunk instead of one per step -- at t_max = 5 the whole kernel is a single round trip).
  constexpr int CH = 8;
  const float vb = v_boot[e];
  double S = 0.0, Vn = (double)vb;      // S: the return R (n-step) / the advantage A (GAE); Vn: GAE's V_{t+1}, v_boot at t = T - 1
  for (int t0 = T - 1; t0 >= 0; t0 -= CH) {
    float r[CH], m[CH], v[CH], tr[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 - u;
      const long i = (long)(t >= 0 ? t : 0) * N + e;
      r[u] = rewards[i];
      m[u] = masks[i];
      v[u] = values[i];
      if constexpr (TR) tr[u] = truncs[i];
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int t = t0 - u;
      if (t >= 0) {
        const long i = (long)t * N + e;
        const double V = (double)v[u];
        if constexpr (EST == kEstGae) {
          if constexpr (TR) gae_step_tr(gamma, gl, r[u], m[u], tr[u], V, Vn, S);
          else gae_step(gamma, gl, r[u], m[u], V, Vn, S);
          adv[i] = (float)S;
          y[i] = (float)__dadd_rn(S, V);
          Vn = V;
        } else {
          if constexpr (TR) nstep_step_tr(gamma, t == T - 1, vb, r[u], m[u], tr[u], V, S);
          else nstep_step(gamma, t == T - 1, vb, r[u], m[u], S);
          y[i] = (float)S;
          adv[i] = (float)__dsub_rn(S, V);
        }
      }
    }
  }
}

// --adv_norm (include/paac_hip.h has the contract): the B = T*N advantages of one rollout, normalised by their own mean and
// population standard deviation.  ONE workgroup of kNormThreads threads does everything, so the statistics need no second
// launch and no atomics: thread t owns rows t, t + kNormThreads, ... in every pass, a block sum is 32 column sums of 32
// per-thread values and then the sum of those 32, every step a separate round-to-nearest fp64 operation -- the same inputs
// give the same bits wherever the launch sits.  Two passes (the mean first, then the squared deviations from it).
constexpr int kNormThreads = 1024;
__device__ __forceinline__ double norm_block_sum(const double v, double* lds /* kNormThreads + 32 */) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  if (tid < 32) {
    double t = 0.0;
    for (int i = 0; i < kNormThreads / 32; ++i) t = __dadd_rn(t, lds[i * 32 + tid]);
    lds[kNormThreads + tid] = t;
  }
  __syncthreads();
  double r = 0.0;
  for (int c = 0; c < 32; ++c) r = __dadd_rn(r, lds[kNormThreads + c]);   // (every thread: the same order, the same value)
  __syncthreads();
  return r;
}
// adv / adv_n may be the same array; stats (nullable) = {mean, std}.  std == 0 (B = 1, identical advantages) gives zeros;
// a non-finite input makes mean and std non-finite and with them every output.
__device__ __forceinline__ void adv_normalize_block(const float* adv, const int B, float* adv_n, double* stats, double* lds) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < B; i += kNormThreads) acc = __dadd_rn(acc, (double)adv[i]);
  const double mean = norm_block_sum(acc, lds) / (double)B;
  acc = 0.0;
  for (int i = tid; i < B; i += kNormThreads) {
    const double d = __dsub_rn((double)adv[i], mean);
    acc = __dadd_rn(acc, __dmul_rn(d, d));
  }
  const double sd = sqrt(norm_block_sum(acc, lds) / (double)B);
  const double den = __dadd_rn(sd, 1e-8);
  for (int i = tid; i < B; i += kNormThreads)
    adv_n[i] = (sd == 0.0) ? 0.f : (float)(__dsub_rn((double)adv[i], mean) / den);
  if (tid == 0 && stats) {
    stats[0] = mean;
    stats[1] = sd;
  }
}
__global__ __launch_bounds__(kNormThreads) void adv_normalize_kernel(const float* adv, int B, float* adv_n, double* stats) {
  __shared__ double lds[kNormThreads + 32];
  adv_normalize_block(adv, B, adv_n, stats, lds);
}
// The returns of either estimator (heads.h: nstep_row_from / gae_row_from, the scans the backward's first launch runs -- every
// row rescans its own return, so y / adv equal returns_scan_kernel's bit for bit), the cycle bookkeeping of that kernel,
// and the normalisation above, in one launch.
template <class RT>
__global__ __launch_bounds__(kNormThreads) void returns_norm_kernel(const RT r, float* adv_n, double* stats) {
  __shared__ double lds[kNormThreads + 32];
  const int tid = threadIdx.x, B = r.T * r.N;
  for (int i = tid; i < B; i += kNormThreads) {
    float yv, av;
    returns_row(r, i, yv, av);
    r.y_out[i] = yv;
    r.adv_out[i] = av;        // (read back below by the thread that wrote it)
  }
  if (tid == 0) cycle_tick(r.ct);
  adv_normalize_block(r.adv_out, B, adv_n, stats, lds);
}

// --window_stats (spec and twin: paac_amd/window_stats.py; include/paac_hip.h has the contract): one cycle folded into the
// window's accumulator block.  ONE workgroup of kWinThreads threads and no atomics, so the order of every float64 sum is fixed:
// thread i takes rows i, i + 256, ... (and surviving ring entries i, i + 256, ...) in order, every product and sum a separate
// round-to-nearest operation, and one finishing thread per field adds the 256 partials in index order out of LDS and stores
// the field.  The four waves finish one part each -- row sums, counts, episodes, the update's scalars -- beside one another.
// The block's offsets (window_stats.FIELDS_F / FIELDS_I; paac_window_fields reports the two lengths):
constexpr int kWinThreads = 256;
enum : int { kWfRowSums = 0 /* v v2 y y2 d d2 adv adv2, max|adv|, reward */, kWfMaxAbsAdv = 8, kWfSumLoss = 10, kWfSumStats = 14,
             kWfSumGnorm = 17, kWfMaxGnorm = 18, kWfEpSums = 19 /* return, return2, length, length2 */,
             kWfEpRetMin = 23 /* return min, return max, length min, length max */, kWinFieldsF = 27 };
enum : int { kWiCycles = 0, kWiRows = 1, kWiTerminals = 2 /* terminals, truncated, nonzero rewards */, kWiOptSteps = 5,
             kWiOptApplied = 6, kWiStatSteps = 7, kWiEpisodes = 8, kWiDropped = 9, kWiActionCount = 10, kWiRingCursor = 42,
             kWinFieldsI = 43 };
constexpr int kWinRowFields = 10, kWinActions = 32, kWinRing = 4096;
static_assert(kWfEpRetMin == kWfEpSums + 4 && kWfMaxAbsAdv < kWinRowFields, "the finishing lanes index consecutive fields");
// One finishing thread's walk over the 256 partials of its field, in index order: kWinOpAdd from 0.0, or the min / max of the
// first `holders` partials.  16 partials are requested from LDS at a time and then combined one after the other -- the
// order is the contract, the loads need not wait for one another.
enum : int { kWinOpAdd = 0, kWinOpMin = 1, kWinOpMax = 2 };
__device__ __forceinline__ double window_partials(const double* src, const int op, const int holders) {
  double t = op == kWinOpAdd ? 0.0 : src[0];
  for (int i0 = 0; i0 < kWinThreads; i0 += 16) {
    double x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = src[i0 + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const double lo = fmin(t, x[u]), hi = fmax(t, x[u]);
      t = op == kWinOpAdd ? __dadd_rn(t, x[u]) : (i0 + u < holders ? (op == kWinOpMin ? lo : hi) : t);
    }
  }
  return t;
}
__device__ __forceinline__ int64_t window_counts(const int32_t* src) {
  int64_t t = 0;
  for (int i0 = 0; i0 < kWinThreads; i0 += 16) {
    int32_t x[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) x[u] = src[i0 + u];
#pragma unroll
    for (int u = 0; u < 16; ++u) t += x[u];
  }
  return t;
}
__global__ __launch_bounds__(kWinThreads) void window_fold_kernel(const paac_window_inputs w, double* __restrict__ acc_f,
                                                                  int64_t* __restrict__ acc_i) {
  __shared__ double row_p[kWinRowFields][kWinThreads];
  __shared__ double ep_p[8][kWinThreads];
  __shared__ int32_t cnt_p[3][kWinThreads];
  __shared__ int32_t hist[kWinActions][kWinThreads];      // a column per thread: private, so plain read-modify-write
  const int tid = threadIdx.x, B = w.T * w.N;
  const FinishedRing* fin = (const FinishedRing*)w.finished;
  // what the block and the ring say as the fold starts (each read once, before anything is stored)
  const int64_t cursor = acc_i[kWiRingCursor], episodes0 = acc_i[kWiEpisodes];
  const int64_t count = fin ? (int64_t)fin->count : cursor;
#pragma unroll
  for (int a = 0; a < kWinActions; ++a) hist[a][tid] = 0;
  // ---- rows ----
  double s[kWinRowFields];
#pragma unroll
  for (int q = 0; q < kWinRowFields; ++q) s[q] = 0.0;
  int terminals = 0, truncated = 0, nonzero = 0;
  constexpr int U = 4;      // passes requested at once: one memory round trip per U passes
  for (int i0 = tid; i0 < B; i0 += U * kWinThreads) {
    float v[U], y[U], ad[U], r[U], m[U], tr[U];
    int32_t a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * kWinThreads, j = i < B ? i : i0;
      v[u] = w.values[j];
      y[u] = w.y[j];
      ad[u] = w.adv[j];
      r[u] = w.rewards[j];
      m[u] = w.masks[j];
      a[u] = w.actions[j];
      tr[u] = w.truncs ? w.truncs[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i0 + u * kWinThreads < B) {
        const double V = (double)v[u], Y = (double)y[u], D = __dsub_rn(Y, V), A = (double)ad[u];
        s[0] = __dadd_rn(s[0], V);
        s[1] = __dadd_rn(s[1], __dmul_rn(V, V));
        s[2] = __dadd_rn(s[2], Y);
        s[3] = __dadd_rn(s[3], __dmul_rn(Y, Y));
        s[4] = __dadd_rn(s[4], D);
        s[5] = __dadd_rn(s[5], __dmul_rn(D, D));
        s[6] = __dadd_rn(s[6], A);
        s[7] = __dadd_rn(s[7], __dmul_rn(A, A));
        s[8] = fmax(s[8], fabs(A));
        s[9] = __dadd_rn(s[9], (double)r[u]);
        terminals += m[u] == 0.f;
        truncated += tr[u] != 0.f;
        nonzero += r[u] != 0.f;
        if ((uint32_t)a[u] < (uint32_t)w.A) hist[a[u]][tid] += 1;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kWinRowFields; ++q) row_p[q][tid] = s[q];
  cnt_p[0][tid] = terminals;
  cnt_p[1][tid] = truncated;
  cnt_p[2][tid] = nonzero;
  // ---- the ring's new entries: [count - kept, count), slot = entry & 4095 ----
  const int64_t fresh = count > cursor ? count - cursor : 0;
  const int64_t dropped = fresh > kWinRing ? fresh - kWinRing : 0;
  const int kept = (int)(fresh - dropped);
  double e[4] = {0.0, 0.0, 0.0, 0.0}, lo_r = 0.0, hi_r = 0.0, lo_l = 0.0, hi_l = 0.0;
  for (int k = tid; k < kept; k += kWinThreads) {
    const int slot = (int)((count - kept + k) & (kWinRing - 1));
    const double R = (double)fin->reward[slot], L = (double)fin->len[slot];
    e[0] = __dadd_rn(e[0], R);
    e[1] = __dadd_rn(e[1], __dmul_rn(R, R));
    e[2] = __dadd_rn(e[2], L);
    e[3] = __dadd_rn(e[3], __dmul_rn(L, L));
    const bool first = k == tid;
    lo_r = first ? R : fmin(lo_r, R);
    hi_r = first ? R : fmax(hi_r, R);
    lo_l = first ? L : fmin(lo_l, L);
    hi_l = first ? L : fmax(hi_l, L);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) ep_p[q][tid] = e[q];
  ep_p[4][tid] = lo_r;
  ep_p[5][tid] = hi_r;
  ep_p[6][tid] = lo_l;
  ep_p[7][tid] = hi_l;
  __syncthreads();
  // ---- finish: one thread per field, the partials in index order ----
  const int wave = tid >> 6, j = tid & 63;
  if (wave == 0) {
    if (j < kWinRowFields) {
      const bool is_max = j == kWfMaxAbsAdv;
      const double t = window_partials(row_p[j], is_max ? kWinOpMax : kWinOpAdd, kWinThreads);
      acc_f[kWfRowSums + j] = is_max ? fmax(acc_f[kWfRowSums + j], t) : __dadd_rn(acc_f[kWfRowSums + j], t);
    }
  } else if (wave == 1) {
    const bool is_action = j >= 8 && j < 8 + w.A;
    if (j < 3 || is_action) {      // (one walk for both kinds of count: the lanes differ in where they read and write)
      const int64_t t = window_counts(is_action ? hist[j - 8] : cnt_p[j]);
      acc_i[is_action ? kWiActionCount + j - 8 : kWiTerminals + j] += t;
    } else if (j == 48) {
      acc_i[kWiCycles] += 1;
      acc_i[kWiRows] += B;
    }
  } else if (wave == 2) {
    if (fin && j < 8 && kept > 0) {
      // j < 4: the four sums; above: min (j even) or max (j odd) over the threads that saw an entry, and the window's first
      // episode sets the field.  One walk for all eight lanes
      const bool is_sum = j < 4, is_max = j & 1;
      const double t = window_partials(ep_p[j], is_sum ? kWinOpAdd : (is_max ? kWinOpMax : kWinOpMin),
                                       kept < kWinThreads ? kept : kWinThreads);
      const double old = acc_f[kWfEpSums + j];      // (kWfEpRetMin == kWfEpSums + 4: the eight fields are consecutive)
      acc_f[kWfEpSums + j] = is_sum ? __dadd_rn(old, t) : (episodes0 == 0 ? t : (is_max ? fmax(old, t) : fmin(old, t)));
    } else if (fin && j == 8) {
      acc_i[kWiEpisodes] = episodes0 + kept;
      acc_i[kWiDropped] += dropped;
      acc_i[kWiRingCursor] = count;
    }
  } else {
    if (j < 4) {
      double t = 0.0;
      for (int k = 0; k < w.steps; ++k) t = __dadd_rn(t, (double)((k == 0 && w.loss0) ? w.loss0[j] : w.loss[k * 4 + j]));
      acc_f[kWfSumLoss + j] = __dadd_rn(acc_f[kWfSumLoss + j], t);
    } else if (j < 7) {
      if (w.ppo_stats && j - 4 < w.stats_cols) {
        double t = 0.0;
        for (int k = w.stats_first; k < w.steps; ++k) t = __dadd_rn(t, (double)w.ppo_stats[k * w.stats_cols + j - 4]);
        acc_f[kWfSumStats + j - 4] = __dadd_rn(acc_f[kWfSumStats + j - 4], t);
      }
    } else if (j == 7) {
      const double g = (double)w.gnorm[0];
      acc_f[kWfSumGnorm] = __dadd_rn(acc_f[kWfSumGnorm], g);
      acc_f[kWfMaxGnorm] = fmax(acc_f[kWfMaxGnorm], g);
      int applied = w.steps;
      if (w.applied) {
        applied = 0;
        for (int k = 0; k < w.steps; ++k) applied += w.applied[k] != 0;
      }
      acc_i[kWiOptSteps] += w.steps;
      acc_i[kWiOptApplied] += applied;
      if (w.ppo_stats) acc_i[kWiStatSteps] += w.steps - w.stats_first;
    }
  }
}

// actor_learner.py:119-123 evaluated after the cycle's increments (paac.py:127,156).
__global__ void lr_step_kernel(int64_t* global_step, int64_t inc, double lr0, int64_t anneal, float* lr_out) {
  cycle_tick(CycleTick{global_step, inc, lr0, anneal, lr_out, nullptr, 0});
}

__global__ void counter_add_kernel(uint64_t* c, uint64_t inc) { *c += inc; }

// Diagnostic: {shader-clock ticks (s_memtime), constant 100 MHz ticks (s_memrealtime)} -- the quotient of two
// samples' differences is the shader clock the chip actually held in between.
__global__ void clock_probe_kernel(uint64_t* out) {
  out[0] = (uint64_t)clock64();
  out[1] = (uint64_t)wall_clock64();
}

// =============================================================================================
// Philox4x32-10 throughput sampler (oracle/sampler.py:sample_philox; philox4x32_10: csrc/common.h).

__global__ void sample_philox_kernel(const float* __restrict__ probs, int N, int A, uint64_t seed,
                                     const uint64_t* __restrict__ step_base, uint64_t step_off, uint32_t env_offset,
                                     int32_t* __restrict__ actions) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const uint64_t step = (step_base ? *step_base : 0ull) + step_off;
  uint32_t c[4] = {env_offset + (uint32_t)e, (uint32_t)step, (uint32_t)(step >> 32), 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
  int act = A - 1;
  float cum = 0.f;
  for (int j = 0; j < A - 1; ++j) {
    cum += probs[(long)e * A + j];
    if (u < cum) {
      act = j;
      break;
    }
  }
  actions[e] = act;
}

// =============================================================================================
// --ppo_minibatches (include/paac_hip.h has the contract): the shuffles of one cycle, the gather that makes a shuffled
// epoch's rows contiguous, and the record pass's pick of p_old / v_old out of the finished training-side heads.

// Workgroup e = epoch e: B Philox keys, then a bitonic sort of 64-bit composites (key << 32 | row) in LDS.  The row index in
// the low half makes every composite distinct, so ascending composites ARE ascending (key, row) -- the stable argsort --
// whatever network sorts them.  Rows [B, P) of the power-of-two network hold (0xFFFFFFFF << 32 | row): a real key can be
// 0xFFFFFFFF too, and then the padding still compares larger on its row index (>= B).
constexpr int kPermMaxRows = 8192;        // 64 KB of LDS
constexpr int kPermThreads = 1024;
constexpr uint32_t kPermDomain = 0x504D0000u;      // counter word 3 of epoch e = kPermDomain + e (the sampler's is 0)

__global__ __launch_bounds__(kPermThreads) void minibatch_perms_kernel(int B, int P, uint64_t seed,
                                                                       const uint64_t* __restrict__ step_base,
                                                                       uint64_t step_off, int32_t* __restrict__ perms) {
  __shared__ uint64_t s[kPermMaxRows];
  const int e = blockIdx.x;
  const uint64_t step = (step_base ? *step_base : 0ull) + step_off;
  for (int i = threadIdx.x; i < P; i += kPermThreads) {
    uint32_t key = 0xFFFFFFFFu;
    if (i < B) {
      uint32_t c[4] = {(uint32_t)i, (uint32_t)step, (uint32_t)(step >> 32), kPermDomain + (uint32_t)e};
      philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
      key = c[0];
    }
    s[i] = ((uint64_t)key << 32) | (uint32_t)i;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += kPermThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // pair (lo, lo + j): bit j of lo is clear
        const int hi = lo | j;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == ((lo & k) == 0)) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < B; i += kPermThreads) perms[(long)e * B + i] = (int32_t)(uint32_t)s[i];
}

// states_out[r] = states[perm[r]] in 16-byte vectors (a row is 1764 of them; kGatherParts workgroups per row), and the same
// index map on the small arrays (any pair of them absent) in the launch's last workgroups, one row per lane.
constexpr int kRowVecs = PAAC_OBS_BYTES / 16;      // 1764
constexpr int kGatherParts = 4;                    // 441 vectors each
static_assert(kRowVecs % kGatherParts == 0 && kRowVecs * 16 == PAAC_OBS_BYTES, "row split");

struct GatherSmall {
  const int32_t* actions; int32_t* actions_out;
  const float* y; float* y_out;
  const float* adv; float* adv_out;
  const float* p_old; float* p_old_out;
  const float* v_old; float* v_old_out;
};

__global__ __launch_bounds__(256) void gather_minibatch_kernel(const int32_t* __restrict__ perm, int B,
                                                               const uint4* __restrict__ states, uint4* __restrict__ states_out,
                                                               const GatherSmall g) {
  const int state_groups = states ? B * kGatherParts : 0;
  if ((int)blockIdx.x < state_groups) {
    const int r = blockIdx.x / kGatherParts, part = blockIdx.x % kGatherParts;
    const int src = perm[r];
    if ((unsigned)src >= (unsigned)B) return;          // not a row index: nothing is read through it
    constexpr int V = kRowVecs / kGatherParts;
    const uint4* in = states + (long)src * kRowVecs + part * V;
    uint4* out = states_out + (long)r * kRowVecs + part * V;
    for (int v = threadIdx.x; v < V; v += 256) out[v] = in[v];
    return;
  }
  const int r = ((int)blockIdx.x - state_groups) * 256 + threadIdx.x;
  if (r >= B) return;
  const int src = perm[r];
  if ((unsigned)src >= (unsigned)B) return;
  if (g.actions) g.actions_out[r] = g.actions[src];
  if (g.y) g.y_out[r] = g.y[src];
  if (g.adv) g.adv_out[r] = g.adv[src];
  if (g.p_old) g.p_old_out[r] = g.p_old[src];
  if (g.v_old) g.v_old_out[r] = g.v_old[src];
}

// p_old[i] = probs[i, a_i] of the first `batch` rows, v_out[i] = values[i] of the first `vrows` rows of the training set.
__global__ __launch_bounds__(256) void record_policy_kernel(const float* __restrict__ probs, const float* __restrict__ values,
                                                            const int32_t* __restrict__ actions, int A, int batch, int vrows,
                                                            float* __restrict__ p_old, float* __restrict__ v_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (p_old && i < batch) {
    const int a = actions[i];
    if ((unsigned)a < (unsigned)A) p_old[i] = probs[(long)i * A + a];
  }
  if (v_out && i < vrows) v_out[i] = values[i];
}

int launch_record_policy(paac_ctx* ctx, const int32_t* actions, int batch, int vrows, float* p_old, float* v_out,
                         hipStream_t s) {
  const Workspace& W = ctx->ws[1];
  const int rows = batch > vrows ? batch : vrows;
  ProfScope ps(ctx, F_MISC, rows, s);
  launch_k(record_policy_kernel, dim3((rows + 255) / 256), dim3(256), s, PROF_WHOLE, (const float*)W.probs,
           (const float*)W.values, actions, ctx->cfg.num_actions, batch, vrows, p_old, v_out);
  return 0;
}

// =============================================================================================
// numpy-parity sampler: legacy MT19937 multinomial(1, p - epsneg) per env, ONE serial stream
// (paac.py:34-45; restated in oracle/sampler.py:sample_mt_restated).
// (mt_temper / mt_mix: csrc/mt_ahead.h)

// scratch layout (bytes): pj f64[N*(A-1)] | U f64[N*(A-1)] | blocks u32[nblk*624]
// LDSC > 0 (N*(A-1) <= mt_lds_d(LDSC)): the three work arrays live in LDS instead of the global scratch.
// LDS size classes of the sampler body: 0 = work arrays in the global scratch, 1 = small (the 32..64-environment shards),
// 2 = large (256 environments x 4 actions, 128 x 18: one workgroup with most of the CU's LDS)
// (MT_LDS_D = 1024 draws for class 1, MT_LDS_D2 = 2304 for class 2: csrc/mt_ahead.h)
constexpr int MT_TAB_MAX = 16384;         // class 1: entries of the first-hit table
constexpr int MT_TAB_MAX2 = 66560;        // class 2: 256 environments x 3 draws -> 65,536 + 256 entries
__host__ __device__ constexpr int mt_lds_d(int cls) { return cls == 2 ? MT_LDS_D2 : (cls == 1 ? MT_LDS_D : 1); }
__host__ __device__ constexpr int mt_lds_blk(int cls) { return cls == 0 ? 1 : (624 + 2 * mt_lds_d(cls)) / 624 + 2; }
__host__ __device__ constexpr int mt_tab_max(int cls) { return cls == 2 ? MT_TAB_MAX2 : (cls == 1 ? MT_TAB_MAX : 1); }
__host__ __device__ constexpr int mt_skip_max(int cls) { return cls == 2 ? 4352 : (cls == 1 ? 1280 : 1); }
// Phase 4a of sample_mt_body: jh(e, o) = first category hit when environment e starts drawing at stream offset o, for
// every reachable (e, o).  Environment e has e (J-1) + 1 reachable offsets (every earlier environment drew between 1
// and J doubles), so e is paired with N-1-e -- every pair has (N-1)(J-1) + 2 entries -- and each pair is filled by one
// 16-thread group.  JC > 0: J as a compile-time constant, thresholds in registers, the J draws of an entry requested
// before the compares.  JC == 0: any J, thresholds re-read per entry.
template <int JC>
__device__ __forceinline__ void mt_fill_table(const double* pj_buf, const double* u_buf, unsigned char* jh_tab, int N, int D,
                                              int Jdyn = 0) {
  const int J = JC > 0 ? JC : Jdyn;
  constexpr int JR = JC > 0 ? JC : 1;
  const int tid = threadIdx.x;
  const int grp = tid >> 4, k = tid & 15;
  const int npairs = (N + 1) / 2;
  auto threshold = [&](int e, int j, double& thr, bool& inv) {   // hit(U) == ((U > thr) != inv)
    const double pj = pj_buf[e * J + j];
    inv = !(pj <= 0.5);
    thr = inv ? 1.0 - (1.0 - pj) : 1.0 - pj;
  };
  for (int pe = grp; pe < npairs; pe += 16) {
    const int ea = pe, eb = N - 1 - pe;
    const int cnt_a = ea * (J - 1) + 1, cnt_b = (eb != ea) ? eb * (J - 1) + 1 : 0;
    const int base_a = ea + (J - 1) * ea * (ea - 1) / 2, base_b = eb + (J - 1) * eb * (eb - 1) / 2;
    double thr_a[JR], thr_b[JR];
    bool inv_a[JR], inv_b[JR];
    if constexpr (JC > 0) {
#pragma unroll
      for (int j = 0; j < JC; ++j) {
        threshold(ea, j, thr_a[j], inv_a[j]);
        threshold(eb, j, thr_b[j], inv_b[j]);
      }
    }
    if constexpr (JC > 0) {
      // four entries per iteration, every draw of all four requested before the first compare (the loop is LDS-latency
      // bound: one entry at a time spends ~400 cycles per entry, 256 entries per thread at 256 environments)
      constexpr int UNR = 4;
      const int total = cnt_a + cnt_b;
      for (int c0 = k; c0 < total; c0 += 16 * UNR) {
        double U[UNR][JR];
        bool first[UNR], live[UNR];
        int idx[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int c = c0 + 16 * u;
          live[u] = c < total;
          first[u] = c < cnt_a;
          idx[u] = first[u] ? c : c - cnt_a;
          const int o = (first[u] ? ea : eb) + (live[u] ? idx[u] : 0);
#pragma unroll
          for (int j = 0; j < JC; ++j) U[u][j] = u_buf[o + j < D ? o + j : D - 1];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          int jh = J;
#pragma unroll
          for (int j = JC - 1; j >= 0; --j) {
            const double thr = first[u] ? thr_a[j] : thr_b[j];
            const bool inv = first[u] ? inv_a[j] : inv_b[j];
            if ((U[u][j] > thr) != inv) jh = j;
          }
          if (live[u]) jh_tab[(first[u] ? base_a : base_b) + idx[u]] = (unsigned char)jh;
        }
      }
      continue;
    }
    for (int c = k; c < cnt_a + cnt_b; c += 16) {
      const bool first = c < cnt_a;
      const int e = first ? ea : eb;
      const int idx = first ? c : c - cnt_a;   // table slot of the pair member
      const int o = e + idx;                   // stream offset it stands for
      int jh = J;
      {
        for (int j = J - 1; j >= 0; --j) {
          double thr;
          bool inv;
          threshold(e, j, thr, inv);
          if ((u_buf[o + j < D ? o + j : D - 1] > thr) != inv) jh = j;
        }
      }
      jh_tab[(first ? base_a : base_b) + idx] = (unsigned char)jh;
    }
  }
}

// (mt_pack_threshold -- walk thresholds carry their sense in the sign bit: hit(U) == ((U > |t|) != signbit(t)) -- is
// csrc/fc_heads.h's, beside the heads finish that leaves them)
__device__ __forceinline__ bool mt_hit(const double U, const double t) {
  return (U > fabs(t)) != (__double_as_longlong(t) < 0);
}

// Small shards (up to 32 environments x up to 7 actions) without a table: the environments are cut into groups of QG (8,
// or 4 where the walks still fit the workgroup); group k can be entered at k QG (J-1) + 1 stream offsets, and one THREAD
// per (group, entry offset) walks its group from there, deciding each environment's first hit itself (J draws against
// the environment's J thresholds, all requested before the first compare) and recording the categories it meets -- QG
// dependent LDS round trips, all walks side by side (groups 0..31/QG: at most 256 threads).  Then one lane follows the
// group exits and every environment picks the record of the walk that really happened.  thr_s / inv_s: the thresholds
// phase 1 left behind.  Returns the consumed-draw count through *used_s.
__host__ __device__ constexpr int mt_walks(const int qg, const int c1) {      // walks of all 32 / qg groups
  return 32 / qg + qg * c1 * ((32 / qg) * (32 / qg - 1) / 2);
}
template <int JC, int QG>
__device__ __forceinline__ void mt_group_walks(const double* thr_s, const double* u_buf, const unsigned char* inv_s, unsigned short* rec_s,
                                               int* entry_s, int* used_s, const int N, const int D,
                                               int32_t* __restrict__ actions, int16_t* act_lds) {
  constexpr int C1 = JC - 1, NGRP = 32 / QG;
  static_assert(mt_walks(QG, C1) <= 256, "one thread per walk");
  const int tid = threadIdx.x;
  MISC_STAMP(5);
  unsigned char* act_h = reinterpret_cast<unsigned char*>(rec_s);                // [walk <= 256][QG hops]
  unsigned short* end_h = rec_s + 1024;                                           // [walk] exit offset
  auto first_walk = [&](const int k) { return k + QG * C1 * (k * (k - 1) / 2); };   // walks of groups 0..k-1
  int g = 0;
#pragma unroll
  for (int k = 1; k < NGRP; ++k) g = (tid >= first_walk(k)) ? k : g;
  const int h = tid - first_walk(g);
  if (g * QG < N && h < g * QG * C1 + 1) {
    int e = g * QG, o = e + h;
    for (int hop = 0; hop < QG; ++hop) {
      if (e < N) {
        double U[JC], T[JC];
#pragma unroll
        for (int j = 0; j < JC; ++j) {
          U[j] = u_buf[o + j < D ? o + j : D - 1];
          T[j] = thr_s[e * JC + j];
        }
        int jh = JC;
#pragma unroll
        for (int j = JC - 1; j >= 0; --j)
          if (mt_hit(U[j], T[j])) jh = j;
        act_h[tid * QG + hop] = (unsigned char)jh;
        o += (jh + 1 < JC) ? jh + 1 : JC;
        ++e;
      }
    }
    end_h[tid] = (unsigned short)o;
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int k = 0; k * QG < N; ++k) {
      const int w = first_walk(k) + o - k * QG;          // the walk of group k that really happens
      entry_s[k] = w;
      o = end_h[w];
    }
    *used_s = o;
  }
  __syncthreads();
  if (tid < N) {
    const int k = tid / QG;
    const int jh = act_h[entry_s[k] * QG + (tid - k * QG)];
    actions[tid] = jh;                                   // jh == J  <=>  no hit  <=>  action A-1 = J
    if (act_lds) act_lds[tid] = (int16_t)jh;
  }
}

// Large shards (256 environments x 4 actions, 128 x 18): the same group walks spread over SEVERAL workgroups of the launch.
// Every sampler workgroup rebuilds thresholds and doubles for itself (cheap next to a serial walk over all environments),
// takes 256 of the (group of 8 environments, entry offset) walks, and leaves their records in global memory; the workgroup
// that takes the last ticket follows the group exits, reads every environment's category out of the record of the walk
// that really happened, and goes on as the one sampler workgroup used to (stream position, bookkeeping).  Tickets are a
// counter that is never reset: every launch adds W to it (2^32 tickets = more than 10^8 launches for any W here; one
// scratch per (N, A)).
struct MultiWalk {
  unsigned char* rec;         // [walks][8] categories met
  unsigned short* exits;      // [walks] stream offset each walk leaves its group at
  unsigned int* counter;
  int W;                      // sampler workgroups of the launch; 0: single-workgroup sampler
};
constexpr int MW_G = 8;
__host__ __device__ inline long mw_first_walk(const int k, const int c1) { return k + (long)MW_G * c1 * ((long)k * (k - 1) / 2); }
__host__ __device__ inline long mw_walks(const int N, const int A) { return mw_first_walk((N + MW_G - 1) / MW_G, A - 2); }

// group of walk `wid`: the largest k with first_walk(k) <= wid  (first_walk(k) = a k^2 + (1 - a) k, a = 4 (J - 1))
__device__ __forceinline__ int mw_group_of(const long wid, const int c1, const int NG) {
  if (c1 == 0) return (int)wid;
  const float a = 4.0f * (float)c1;
  int k = (int)((sqrtf((1.f - a) * (1.f - a) + 4.f * a * (float)wid) - (1.f - a)) / (2.f * a));
  k = k < 0 ? 0 : (k > NG - 1 ? NG - 1 : k);
  while (k > 0 && mw_first_walk(k, c1) > wid) --k;
  while (k < NG - 1 && mw_first_walk(k + 1, c1) <= wid) ++k;
  return k;
}

// one hop of a walk: first category hit by environment e when it starts drawing at offset o (J = JC > 0, or Jdyn)
template <int JC>
__device__ __forceinline__ int mw_first_hit(const double* thr_s, const unsigned char* inv_s, const double* u_buf, const int e,
                                            const int o, const int D, const int Jdyn) {
  if constexpr (JC > 0) {
    double U[JC], T[JC];
#pragma unroll
    for (int j = 0; j < JC; ++j) {
      U[j] = u_buf[o + j < D ? o + j : D - 1];
      T[j] = thr_s[e * JC + j];
    }
    int jh = JC;
#pragma unroll
    for (int j = JC - 1; j >= 0; --j)
      if (mt_hit(U[j], T[j])) jh = j;
    return jh;
  } else {
    const int J = Jdyn;
    int jh = J;
    constexpr int CH = 6;                                // categories per round trip; a wave scans until its last walk has hit
    for (int j0 = 0; j0 < J && jh == J; j0 += CH) {
      double U[CH], T[CH];
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int j = j0 + q < J ? j0 + q : J - 1;
        U[q] = u_buf[o + j < D ? o + j : D - 1];
        T[q] = thr_s[e * J + j];
      }
#pragma unroll
      for (int q = CH - 1; q >= 0; --q)
        if (j0 + q < J && mt_hit(U[q], T[q])) jh = j0 + q;
    }
    return jh;
  }
}

// Returns 1 in the workgroup that took the last ticket (actions written, *used_s = draws consumed), 0 elsewhere.
// dist_zero: every workgroup has seen only ITS environments' probabilities (the heads were finished inside this launch) and
// reports an exactly-zero conditional probability among them with its ticket -- the count rides in the upper half of the
// ticket word, one atomic --; the last-ticket workgroup then returns 2 WITHOUT following the walks when any workgroup
// reported one (the caller takes the serial path over all environments).
template <int JC>
__device__ __forceinline__ int mt_multi_walks(const MultiWalk mw, const double* thr_s, const unsigned char* inv_s,
                                              const double* u_buf, unsigned short* exits_lds, int* entry_s, int* used_s,
                                              const int N, const int J, const int D, int32_t* __restrict__ actions,
                                              int16_t* act_lds, const bool dist_zero = false, const bool local_zero = false) {
  const int tid = threadIdx.x;
  const int c1 = J - 1, NG = (N + MW_G - 1) / MW_G;
  const long nwk = mw_first_walk(NG, c1);
  const long wid = (long)blockIdx.x * 256 + tid;
  if (wid < nwk) {
    const int k = mw_group_of(wid, c1, NG);
    int e = k * MW_G, o = e + (int)(wid - mw_first_walk(k, c1));
    unsigned int lo = 0, hi = 0;                         // the 8 categories met, one byte each
    for (int hop = 0; hop < MW_G; ++hop) {
      if (e < N) {
        const int jh = mw_first_hit<JC>(thr_s, inv_s, u_buf, e, o, D, J);
        if (hop < 4) lo |= (unsigned int)jh << (8 * hop);
        else hi |= (unsigned int)jh << (8 * (hop - 4));
        o += (jh + 1 < J) ? jh + 1 : J;
        ++e;
      }
    }
    reinterpret_cast<uint2*>(mw.rec)[wid] = make_uint2(lo, hi);
    mw.exits[wid] = (unsigned short)o;
  }
  MISC_STAMP(9);
  // hand-off: every storing thread first drains its own stores to the L2 (workgroup-scope release: s_waitcnt vmcnt(0), no
  // cache maintenance) -- the barrier alone does not wait for another wave's stores in flight --, then thread 0's
  // device-scope release (L2 write-back, then the ticket) publishes the whole workgroup's records: one write-back per
  // workgroup, not one per thread; the same on the acquiring side.  The workgroup that takes the last ticket puts the
  // counter back to 0 (every ticket of this launch has been taken; the next launch is stream-ordered behind this one), so
  // the counter never leaves [0, W] and cannot wrap.
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __shared__ int last_s;
  if (tid == 0) {
    __threadfence();
    const unsigned int add = 1u + ((dist_zero && local_zero) ? 0x10000u : 0u);
    const unsigned int old = atomicAdd(mw.counter, add);
    last_s = (old & 0xFFFFu) == (unsigned int)(mw.W - 1) ? (((old + add) >> 16) != 0u ? 2 : 1) : 0;
    if (last_s) {
      __threadfence();
      __hip_atomic_store(mw.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  if (!last_s) return 0;
  if (last_s == 2) return 2;
  MISC_STAMP(10);
  {
    const uint4* src = reinterpret_cast<const uint4*>(mw.exits);       // 8 exit offsets per load (the scratch is padded)
    uint4* dst = reinterpret_cast<uint4*>(exits_lds);
    for (long i = tid; i < (nwk + 7) / 8; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  MISC_STAMP(11);
  if (tid == 0) {
    int o = 0;
    for (int k = 0; k < NG; ++k) {
      const long w = mw_first_walk(k, c1) + o - k * MW_G;      // the walk of group k that really happens
      entry_s[k] = (int)w;
      o = exits_lds[w];
    }
    *used_s = o;
  }
  __syncthreads();
  MISC_STAMP(12);
  for (int e = tid; e < N; e += 256) {
    const int k = e / MW_G;
    const int jh = __builtin_nontemporal_load(mw.rec + (long)entry_s[k] * MW_G + (e - k * MW_G));
    actions[e] = jh;                                     // jh == J  <=>  no hit  <=>  action A-1 = J
    if (act_lds) act_lds[e] = (int16_t)jh;
  }
  __syncthreads();
  return 1;
}

// probs_lds (LDSC > 0 only, nullable): the probabilities are already in LDS (written by this workgroup, barrier passed);
// stw_pre (with probs_lds): the caller requested the 625 state words (3 per thread, clamped index) before producing them.
// probs_hook (with probs_lds): produces the probabilities in probs_lds and ends with a barrier.  It is called AFTER the
// state blocks and the doubles (which need nothing but the state words) so that whatever the hook waits on -- the loads
// of the head partials it requested earlier -- travels while those phases compute.
// Phase 1 of sample_mt_body for one (environment, category j): the row's first j + 1 probabilities requested at once (one
// LDS round trip instead of j dependent ones), then the reference's sequential fp64 subtraction order over the first j of
// them (paac.py:42: p - epsneg in float32; numpy's multinomial: remaining -= p_i in float64).
template <int R>
__device__ __forceinline__ void mt_row_inputs(const float* row_p, const int j, double& remaining, double& p) {
  float row[R];
#pragma unroll
  for (int i = 0; i < R; ++i) row[i] = row_p[i <= j ? i : j];
  remaining = 1.0;
#pragma unroll
  for (int i = 0; i < R; ++i)
    if (i < j) remaining -= (double)(row[i] - 5.9604644775390625e-08f);
  float pj_f = row[0];
#pragma unroll
  for (int i = 1; i < R; ++i) pj_f = (i == j) ? row[i] : pj_f;
  p = (double)(pj_f - 5.9604644775390625e-08f);
}

// A probabilities hook: operator()(dst, scratch, lo, hi) leaves the probabilities of environments [lo, hi) at
// dst[e * A + a] (dst = the body's LDS array unless the hook has its own; scratch = LDS free at that point) and ends with a
// barrier; kOwnRows: the hook serves only the rows asked for (the multi-workgroup sampler: every workgroup finishes the heads
// of ITS environments), so the exact-zero scan is distributed (mt_multi_walks: dist_zero).
struct NoProbsHook {
  __device__ __forceinline__ void operator()() const {}
};
// test hook (paac_debug_report_zero): sampler workgroup `g_dbg_zero_wg` of the heads-folding launch reports an exactly-zero
// conditional probability it has not seen, so that the protocol around it (count in the ticket word, the last-ticket
// workgroup finishing all heads and walking serially) runs on ordinary probabilities; -1 = off
__device__ int g_dbg_zero_wg = -1;
// The multi-workgroup sampler's hook (class 2): finishes the heads of environments [lo, hi) from the fc kernel's per-tile
// partials (csrc/fc_heads.h: the same sums in the same order as heads_from_partials), probabilities to dst[e * A + a] in LDS
// and -- with the values -- to global memory; ends with a barrier.  scratch: (hi - lo) * (A + 1) floats of LDS.
struct RowsHeadsHook {
  const float* partial;
  int ntiles, N, A;
  const float *ba, *bc;
  float *probs_out, *values_out;
  __device__ __forceinline__ void operator()(float* dst, float* scratch, const int lo, const int hi) const {
    const int tid = threadIdx.x;
    const int n_total = N * (A + 1), n = (hi - lo) * (A + 1);
    for (int i = tid; i < n; i += 256) {
      const int a = i % (A + 1);
      float acc = (a < A) ? ba[a] : bc[0];
      for (int t0 = 0; t0 < ntiles; t0 += 32) {
        float v[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) v[t] = partial[(size_t)(t0 + t < ntiles ? t0 + t : 0) * n_total + (size_t)lo * (A + 1) + i];
#pragma unroll
        for (int t = 0; t < 32; ++t) acc += (t0 + t < ntiles) ? v[t] : 0.f;
      }
      scratch[i] = acc;
    }
    __syncthreads();
    heads_softmax_store(hi - lo, A, scratch, dst + (size_t)lo * A, nullptr, probs_out + (size_t)lo * A, values_out + lo, nullptr,
                        nullptr, nullptr);
  }
};
template <class H> struct HookOwnRows { static constexpr bool value = false; };
template <> struct HookOwnRows<RowsHeadsHook> { static constexpr bool value = true; };
// The small shards' hook (up to 32 environments x 7 actions, the headline shape): heads finish AND phase 1 without leaving
// the registers -- heads_finish_fused (csrc/fc_heads.h) on the partials the caller requested before the sampler's own phases: no
// LDS round trip and no barrier between the partial sums and the thresholds (the separate hook + phase 1 take three).
// Leaves probs in probs_lds / probs_out, values in values_out, pj_buf / thr_s / *any_zero as phase 1 would; NO barrier.
struct FusedHeadsHook {
  const float (&pv)[64];
  float bias;
  int ntiles, N, A;
  float* probs_lds;
  float* probs_out;
  float* values_out;
  __device__ __forceinline__ void operator()(double* pj_buf, double* thr_s, int* any_zero) const {
    if (heads_finish_fused(pv, bias, ntiles, N, A, (int)threadIdx.x, probs_lds, probs_out, values_out, pj_buf, thr_s)) *any_zero = 1;
  }
};
// The same place in the body for a debt whose heads the conv tower launch in front of this one has finished (csrc/tower.h:
// RIDER; synth_dev.h: ActFinishRecord): the record's words, requested by the caller together with the state words -- one round
// trip --, are parked where the hook above leaves its results.  D = N (A - 1) <= 192 and NA = N A <= 224: one of each per thread.
struct ParkedRecordHook {
  double pj, thr;
  float pr;
  bool zero;
  int D, NA;
  float* probs_lds;
  __device__ __forceinline__ void operator()(double* pj_buf, double* thr_s, int* any_zero) const {
    const int tid = threadIdx.x;
    if (tid < D) {
      pj_buf[tid] = pj;
      if (thr_s) thr_s[tid] = thr;
    }
    if (tid < NA) probs_lds[tid] = pr;
    if (zero && tid == 0) *any_zero = 1;
  }
};
// The LDS arrays of sample_mt_body, one set per size class: a kernel that holds the body twice (two hooks: act_sample_body)
// reserves them once.  (Function-local arrays of the body itself are per instantiation, and the compiler does not overlay them.)
template <int LDSC>
struct MtLds {
  double pj[mt_lds_d(LDSC)];
  double u[mt_lds_d(LDSC)];
  uint32_t blocks[mt_lds_blk(LDSC) * 624];
  __attribute__((aligned(16))) unsigned char jh_tab[mt_tab_max(LDSC)];
  unsigned short skip_tab[mt_skip_max(LDSC)];
  int entry[33];
  uint32_t pos;
  int any_zero;
};
// (SET: a kernel that wants the two bodies on arrays of their own asks for set 1 -- synth_step_a_mth_kernel, which thereby
// reserves more than half of a CU's LDS and keeps the other workgroups of its launch off the sampler workgroup's CU: with
// one set, --raw-frames measured 0.2345 against 0.2317 ms per cycle, profiles/r08_secondary.txt)
template <int LDSC, int SET>
__device__ __forceinline__ MtLds<LDSC>& mt_lds() {
  __shared__ MtLds<LDSC> lds;
  return lds;
}
template <class H> struct HookFused { static constexpr bool value = false; };
template <> struct HookFused<FusedHeadsHook> { static constexpr bool value = true; };
template <> struct HookFused<ParkedRecordHook> { static constexpr bool value = true; };
template <int LDSC, class HOOK = NoProbsHook, int SET = 0>
__device__ __forceinline__ bool sample_mt_body(const float* __restrict__ probs, int N, int A,
                                               uint32_t* __restrict__ mt_state, double* __restrict__ pj_g,
                                               double* __restrict__ u_g, uint32_t* __restrict__ blocks_g,
                                               int32_t* __restrict__ actions, int16_t* act_lds,
                                               const float* probs_lds = nullptr, const uint32_t* stw_pre = nullptr,
                                               const HOOK probs_hook = HOOK(), const MultiWalk mw = MultiWalk{nullptr, nullptr, nullptr, 0},
                                               const MtAhead* __restrict__ ahead = nullptr) {
  constexpr bool HOOKED = !__is_same(HOOK, NoProbsHook);
  constexpr bool OWNROWS = HookOwnRows<HOOK>::value;      // the hook finishes the heads of this workgroup's environments only
  constexpr bool FUSED = HookFused<HOOK>::value;          // the hook does phase 1 too
  MISC_STAMP(0);
  constexpr bool LDSPATH = LDSC > 0;
  constexpr int PRW = LDSC == 2 ? 18 : 8;             // probability floats per thread of the one-round-trip load
  MtLds<LDSC>& lds = mt_lds<LDSC, SET>();
  double* const pj_s = lds.pj;
  double* const u_s = lds.u;
  uint32_t* const blocks_s = lds.blocks;
  double* pj_buf = LDSPATH ? pj_s : pj_g;
  double* u_buf = LDSPATH ? u_s : u_g;
  uint32_t* blocks = LDSPATH ? blocks_s : blocks_g;
  const int tid = threadIdx.x;
  const int J = A - 1;
  const int D = N * J;
  // N*A = D*A/(A-1) <= 2*D floats (a parked record's probabilities come in the caller's array: none of its own)
  __shared__ float probs_s[LDSPATH && !__is_same(HOOK, ParkedRecordHook) ? 2 * mt_lds_d(LDSC) : 1];
  uint32_t& pos_s = lds.pos;
  int& any_zero = lds.any_zero;  // some conditional probability is exactly 0 (the table chase needs none); later
                                 // reused for the consumed-draw count
  uint32_t pos;
  // csrc/mt_ahead.h (class 2 only): the step's doubles, made one launch ahead, travel with the state words and the
  // probabilities; they are used only if their key matches the stream state found here (pre_ok, uniform)
  constexpr int AHW = LDSC == 2 ? (MT_LDS_D2 + 255) / 256 : (LDSC == 1 ? MT_LDS_D / 256 : 1);
  double ahu[AHW];
  uint32_t ahk[5] = {0u, 0u, 0u, 0u, 0u};
  bool pre_ok = false;
  if (tid == 0) any_zero = 0;    // ordered before phase 1 by the barrier below (LDSPATH) / after phase 2's copy
  if constexpr (LDSPATH) {
    // ONE memory round trip: the 625 state words and the N*A probabilities are all requested before anything
    // is consumed (unrolled, clamped indices), then parked in LDS.
    uint32_t stw[3];
    float prw[PRW];
    if (ahead) {
#pragma unroll
      for (int k = 0; k < 5; ++k) ahk[k] = ahead->hdr[k];
#pragma unroll
      for (int k = 0; k < AHW; ++k) ahu[k] = ahead->u[min(tid + k * 256, MT_LDS_D2 - 1)];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) stw[k] = stw_pre ? stw_pre[k] : mt_state[min(tid + k * 256, 624)];
    if (!probs_lds && !OWNROWS) {
#pragma unroll
      for (int k = 0; k < PRW; ++k) prw[k] = probs[min(tid + k * 256, N * A - 1)];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int idx = tid + k * 256;
      if (idx < 624) blocks[idx] = stw[k];
      if (idx == 624) pos_s = stw[k];
    }
    if (!probs_lds && !OWNROWS) {
#pragma unroll
      for (int k = 0; k < PRW; ++k)
        if (tid + k * 256 < N * A) probs_s[tid + k * 256] = prw[k];
    }
    __syncthreads();
    pos = pos_s;
    if (ahead) {
      pre_ok = ahk[0] == pos && ahk[1] == blocks[0] && ahk[2] == blocks[1] && ahk[3] == blocks[623] && (int)ahk[4] >= N * J;
      if (pre_ok) {
#pragma unroll
        for (int k = 0; k < AHW; ++k)
          if (tid + k * 256 < N * J) u_buf[tid + k * 256] = ahu[k];
      }
    }
  } else {
    pos = mt_state[624];
  }
  MISC_STAMP(1);
  const float* pr = LDSPATH ? (probs_lds ? probs_lds : probs_s) : probs;
  const int nblk = (int)((pos + 2u * (uint32_t)D) / 624u) + 1;
  // the walks of the small shards (mt_group_walks) want thresholds: phase 1 leaves them behind too
  unsigned char* const jh_tab = lds.jh_tab;
  const bool multi = LDSC == 2 && mw.W > 0;          // group walks spread over mw.W workgroups of the launch
  const bool walk_ok = (LDSC == 1 && N <= 32 && 4 + 48 * (J - 1) <= 256) || multi;
  double* thr_s = reinterpret_cast<double*>(jh_tab);           // [D <= 1024]   (the first-hit table is not built then)
  unsigned char* inv_s = jh_tab + (LDSC == 0 ? 0 : 8 * mt_lds_d(LDSC));      // [D]
  static_assert(LDSC == 0 || mt_tab_max(LDSC) >= 9 * mt_lds_d(LDSC), "threshold arrays reuse the table's LDS");
  // phase 1: conditional probabilities p_j / remaining_j, one (env, category) per thread: the running
  // `remaining` is rebuilt with the reference's sequential fp64 subtraction order (cheap), so that only ONE fp64
  // division sits on each thread's critical path instead of J in a row
  auto phase1 = [&](const int e_lo, const int e_hi) {      // environments [e_lo, e_hi)
    for (int d = e_lo * J + tid; d < e_hi * J; d += 256) {
      const int e = d / J, j = d - e * J;
      double remaining = 1.0;
      double p;
      if (LDSPATH && J <= 4) mt_row_inputs<4>(pr + (long)e * A, j, remaining, p);
      else if (LDSPATH && J <= 17) mt_row_inputs<17>(pr + (long)e * A, j, remaining, p);
      else {
        for (int i = 0; i < j; ++i)
          remaining -= (double)(pr[(long)e * A + i] - 5.9604644775390625e-08f);
        p = (double)(pr[(long)e * A + j] - 5.9604644775390625e-08f);
      }
      const double cond = p / remaining;
      pj_buf[d] = cond;
      if (LDSPATH && cond == 0.0) any_zero = 1;
      if (walk_ok) thr_s[d] = mt_pack_threshold(cond);    // hit(U) == ((U > thr) != inv), as mt_fill_table
    }
  };
  // several sampler workgroups: each needs the thresholds of the environments ITS walks visit only; whether some
  // conditional probability is exactly zero (cond == 0  <=>  float32(p - epsneg) == 0) is read off the raw probabilities
  int p1_lo = 0, p1_hi = N;
  if (multi) {
    // (the last category of a row is never drawn for; it is tested like the others -- a division per element costs more
    // than the serial path taken once in 2^24 rows for nothing)
    if constexpr (!OWNROWS) {
      float pz[PRW];
#pragma unroll
      for (int k = 0; k < PRW; ++k) pz[k] = pr[min(tid + k * 256, N * A - 1)];     // N * A <= 2 D <= PRW * 256
      bool z = false;
#pragma unroll
      for (int k = 0; k < PRW; ++k) z = z || ((pz[k] - 5.9604644775390625e-08f) == 0.0f);
      if (z) any_zero = 1;
    }
    const int NGm = (N + MW_G - 1) / MW_G;
    const long nwk = mw_first_walk(NGm, J - 1);
    const long w0 = (long)blockIdx.x * 256, w1 = w0 + 255 < nwk - 1 ? w0 + 255 : nwk - 1;
    if (w0 < nwk) {
      p1_lo = mw_group_of(w0, J - 1, NGm) * MW_G;
      p1_hi = (mw_group_of(w1, J - 1, NGm) + 1) * MW_G;
      p1_hi = p1_hi < N ? p1_hi : N;
    } else {
      p1_hi = 0;
    }
  }
  MISC_STAMP(13);
  if constexpr (!HOOKED) phase1(p1_lo, p1_hi);
  MISC_STAMP(2);
  // phase 2: successive MT19937 state blocks
  if constexpr (!LDSPATH) {
    for (int i = tid; i < 624; i += 256) blocks[i] = mt_state[i];
  }
  __syncthreads();
  for (int b = 1; b < (pre_ok ? 1 : nblk); ++b) {      // (pre_ok: blocks and doubles came ready-made)
    const uint32_t* o = blocks + (long)(b - 1) * 624;
    uint32_t* nw = blocks + (long)b * 624;
    for (int k = tid; k < 227; k += 256) nw[k] = o[k + 397] ^ mt_mix(o[k], o[k + 1]);
    __syncthreads();
    for (int k = 227 + tid; k < 454; k += 256) nw[k] = nw[k - 227] ^ mt_mix(o[k], o[k + 1]);
    __syncthreads();
    for (int k = 454 + tid; k < 623; k += 256) nw[k] = nw[k - 227] ^ mt_mix(o[k], o[k + 1]);
    if (tid == 255) nw[623] = nw[396] ^ mt_mix(o[623], nw[0]);      // both inputs are older than this pass
    __syncthreads();
  }
  MISC_STAMP(3);
  // phase 3: the 53-bit doubles numpy would draw, in stream order
  for (int d = tid; d < (pre_ok ? 0 : D); d += 256) {
    const uint32_t q = pos + 2u * (uint32_t)d;
    const uint32_t a = mt_temper(blocks[q]) >> 5;
    const uint32_t b = mt_temper(blocks[q + 1]) >> 6;
    u_buf[d] = ((double)a * 67108864.0 + (double)b) * 1.1102230246251565404e-16;   // * 2^-53, exact
  }
  __syncthreads();
  if constexpr (HOOKED) {
    if constexpr (OWNROWS) {
      // the heads of this workgroup's environments (jh_tab is free until phase 1 parks the thresholds there), then the
      // exact-zero scan over them: what it finds travels with the ticket (mt_multi_walks: dist_zero)
      probs_hook(probs_s, reinterpret_cast<float*>(jh_tab), p1_lo, p1_hi);
      for (int i = p1_lo * A + tid; i < p1_hi * A; i += 256)
        if ((pr[i] - 5.9604644775390625e-08f) == 0.0f) any_zero = 1;
    } else if constexpr (FUSED) {
      probs_hook(pj_buf, walk_ok ? thr_s : nullptr, &any_zero);
    } else {
      probs_hook();          // ends with a barrier: the probabilities are in LDS
    }
    if constexpr (!FUSED) phase1(p1_lo, p1_hi);
    __syncthreads();
  }
  MISC_STAMP(4);
  // phase 4a (fast path): when every conditional probability is non-zero the stream offset after env e is
  // o + min(jh+1, J) with jh = first category hit when env e starts drawing at offset o.  jh is tabulated for
  // every reachable (e, o) in parallel (o <= e*J), then one lane chases the table: N dependent LDS byte reads
  // instead of N ballot/popcount/compare rounds.
  unsigned short* const skip_tab = lds.skip_tab;
  int* const entry_s = lds.entry;
  bool chased = false;
  if constexpr (LDSPATH) {
    // env e can only start at offsets e .. e J (every earlier env drew between 1 and J doubles)
    const long tab_entries = (long)N + (long)(J - 1) * N * (N - 1) / 2;
    bool walked = false;
    if constexpr (LDSC == 2) {
      if (multi) {
        if (!OWNROWS && any_zero) {
          if (blockIdx.x != 0) return false;          // the rare exact-zero case: workgroup 0 alone, the serial way
          phase1(0, N);
          __syncthreads();
        } else {
          unsigned short* exits_lds = reinterpret_cast<unsigned short*>(jh_tab + 9 * mt_lds_d(2));
          static_assert(mt_tab_max(2) >= 9 * MT_LDS_D2 + 2 * 16384, "exit offsets of up to 16 k walks next to the thresholds");
          int owner;
          const bool lz = OWNROWS && (any_zero != 0 || (int)blockIdx.x == g_dbg_zero_wg);
          switch (J) {
            case 1: owner = mt_multi_walks<1>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            case 2: owner = mt_multi_walks<2>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            case 3: owner = mt_multi_walks<3>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            case 5: owner = mt_multi_walks<5>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            // the 9- and 18-action sets: every category of a hop requested at once -- ONE LDS round trip per hop instead of
            // up to three dependent chunks (a wave waits for its slowest lane anyway): walks 8.4 -> 3 us at 128 x 18
            case 8: owner = mt_multi_walks<8>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            case 17: owner = mt_multi_walks<17>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
            default: owner = mt_multi_walks<0>(mw, thr_s, inv_s, u_buf, exits_lds, entry_s, &any_zero, N, J, D, actions, act_lds, OWNROWS, lz); break;
          }
          if (!owner) return false;
          if (owner == 2) {
            // some workgroup met an exactly-zero conditional probability among its environments: this one (the last
            // ticket) finishes ALL heads and walks the environments the serial way (phase 4b); the walks are discarded
            if constexpr (OWNROWS) probs_hook(probs_s, reinterpret_cast<float*>(jh_tab), 0, N);
            phase1(0, N);
            __syncthreads();
          } else {
            walked = true;
            chased = true;
          }
        }
      }
    }
    if constexpr (LDSC == 1) {
      if (!any_zero && walk_ok) {
        static_assert(mt_skip_max(1) >= 1024 + 256, "walk scratch");
        switch (J) {
#define PAAC_WALK_CASE(JJ) \
  case JJ: mt_group_walks<JJ, (mt_walks(4, JJ - 1) <= 256 ? 4 : 8)>(thr_s, u_buf, inv_s, skip_tab, entry_s, &any_zero, N, D, actions, act_lds); break;
          PAAC_WALK_CASE(1) PAAC_WALK_CASE(2) PAAC_WALK_CASE(3) PAAC_WALK_CASE(4) PAAC_WALK_CASE(5)
          default: mt_group_walks<6, 8>(thr_s, u_buf, inv_s, skip_tab, entry_s, &any_zero, N, D, actions, act_lds); break;
#undef PAAC_WALK_CASE
        }
        __syncthreads();
        walked = true;
        chased = true;
      }
    }
    if (!walked && tab_entries <= mt_tab_max(LDSC) && N <= 256) {
      if (!any_zero) {     // set in phase 1, visible since the barrier after phase 3
        // Table fill (mt_fill_table): the category count is dispatched to a compile-time constant, so the fill has
        // no branch per category
        switch (J) {
          case 1: mt_fill_table<1>(pj_buf, u_buf, jh_tab, N, D); break;
          case 2: mt_fill_table<2>(pj_buf, u_buf, jh_tab, N, D); break;
          case 3: mt_fill_table<3>(pj_buf, u_buf, jh_tab, N, D); break;
          case 4: mt_fill_table<4>(pj_buf, u_buf, jh_tab, N, D); break;
          case 5: mt_fill_table<5>(pj_buf, u_buf, jh_tab, N, D); break;
          case 6: mt_fill_table<6>(pj_buf, u_buf, jh_tab, N, D); break;
          case 7: mt_fill_table<7>(pj_buf, u_buf, jh_tab, N, D); break;
          case 8: mt_fill_table<8>(pj_buf, u_buf, jh_tab, N, D); break;
          default: mt_fill_table<0>(pj_buf, u_buf, jh_tab, N, D, J); break;
        }
        __syncthreads();
        MISC_STAMP(5);
        constexpr int G = 16;                           // environments per group of the two-level chase
        constexpr int MAXQ = (mt_skip_max(LDSC) / 8 + 31) / 32 + 1;   // walks per thread there (a pair of groups per 32 threads)
        const int NG = (N + G - 1) / G;
        const int c1 = J - 1, cg = G * (J - 1);
        // (at 32 environments the single-lane chase is the faster one: 5.3 k cycles against 7.5 k, tools/probe_sampler.py)
        const bool two_level = N > 64 && (NG - 1) * cg + 2 <= 32 * MAXQ && NG + cg * (NG * (NG - 1) / 2) <= mt_skip_max(LDSC);
        if (!two_level) {
          // one lane hops through the table: N dependent LDS byte reads
          if (tid == 0) {
            int o = 0, base = 0, ej = 0;               // base(e) - e = (J-1) e (e-1)/2, ej = e (J-1)
            for (int e = 0; e < N; ++e) {
              const int jh = jh_tab[base + o];         // slot base(e) + (o - e)
              actions[e] = jh;                            // jh == J  <=>  no hit  <=>  action A-1 = J
              if (act_lds) act_lds[e] = (int16_t)jh;
              o += (jh + 1 < J) ? jh + 1 : J;
              base += ej;
              ej += J - 1;
            }
            any_zero = o;                                 // reuse as the consumed-draw count
          }
        } else {
          // Two-level chase.  The stream offset after environment e is a function of the offset before it; environments are
          // cut into groups of G = 16, and for every group and every offset it can be entered at, the offset it is left at
          // is tabulated first: independent walks, each thread advancing its ~16 walks hop by hop without a branch so
          // that their table reads overlap (group k is paired with NG-1-k: every pair has the same number of entries).
          // Then one lane hops over the groups (N / 16 dependent reads instead of N) and one thread per group replays its
          // 16 environments from the true entry offset to emit the actions.
          auto tab_base = [&](const int e) { return e + c1 * (e * (e - 1) / 2); };      // slot of (e, o) = tab_base(e) + o - e
          auto skip_base = [&](const int k) { return k + cg * (k * (k - 1) / 2); };     // group k: entry offsets kG .. kGJ
          const int pr = tid >> 5, ln = tid & 31;         // 8 pairs of groups per pass
          for (int p0 = 0; p0 < (NG + 1) / 2; p0 += 8) {
            const int ka = p0 + pr, kb = NG - 1 - ka;
            const bool pair_ok = ka <= kb;
            const int cnt_a = pair_ok ? ka * cg + 1 : 0, cnt_b = (pair_ok && kb != ka) ? kb * cg + 1 : 0;
            int wo[MAXQ], we[MAXQ], wb[MAXQ], ws[MAXQ];    // offset, environment, table base of it, skip slot (-1: none)
#pragma unroll
            for (int q = 0; q < MAXQ; ++q) {
              const int c = ln + 32 * q;
              const bool live = c < cnt_a + cnt_b, first = c < cnt_a;
              const int k = first ? ka : kb, idx = first ? c : c - cnt_a;
              we[q] = live ? k * G : 0;
              wo[q] = we[q] + (live ? idx : 0);
              wb[q] = tab_base(we[q]);
              ws[q] = live ? skip_base(k) + idx : -1;
            }
            for (int hop = 0; hop < G; ++hop) {
#pragma unroll
              for (int q = 0; q < MAXQ; ++q) {
                const bool ok = ws[q] >= 0 && we[q] < N;
                const int jh = jh_tab[ok ? wb[q] + wo[q] - we[q] : 0];
                const int st = (jh + 1 < J) ? jh + 1 : J;
                wo[q] += ok ? st : 0;
                wb[q] += 1 + c1 * we[q];                  // tab_base(e + 1) - tab_base(e)
                we[q] += 1;
              }
            }
#pragma unroll
            for (int q = 0; q < MAXQ; ++q)
              if (ws[q] >= 0) skip_tab[ws[q]] = (unsigned short)wo[q];
          }
          __syncthreads();
          if (tid == 0) {
            int o = 0;
            for (int k = 0; k < NG; ++k) {
              entry_s[k] = o;
              o = skip_tab[skip_base(k) + o - k * G];
            }
            any_zero = o;                                 // reuse as the consumed-draw count
          }
          __syncthreads();
          if (tid < NG) {
            int o = entry_s[tid];
            const int e1 = min(N, tid * G + G);
            for (int e = tid * G; e < e1; ++e) {
              const int jh = jh_tab[tab_base(e) + o - e];
              actions[e] = jh;                            // jh == J  <=>  no hit  <=>  action A-1 = J
              if (act_lds) act_lds[e] = (int16_t)jh;
              o += (jh + 1 < J) ? jh + 1 : J;
            }
          }
        }
        __syncthreads();
        chased = true;
      }
    }
  }
  MISC_STAMP(6);
  // phase 4b (only when the fast paths above did not run): one wavefront walks the envs in index order; lane j owns
  // category j
  if (!chased) {
    if (tid < 64) {
      const int lane = tid;
      int o = 0;
      for (int e = 0; e < N; ++e) {
        const bool mine = lane < J;
        const double pj = mine ? pj_buf[(long)e * J + lane] : 0.0;
        const bool nzl = mine && (pj != 0.0);
        const unsigned long long nz = __ballot(nzl);
        const unsigned long long below = (lane == 0) ? 0ull : (nz & ((1ull << lane) - 1ull));
        bool hit = false;
        if (nzl) {
          const double U = u_buf[o + __popcll(below)];
          if (pj <= 0.5) {
            hit = U > 1.0 - pj;
          } else {
            const double q = 1.0 - pj;
            hit = !(U > 1.0 - q);
          }
        }
        const unsigned long long hm = __ballot(hit);
        int act, used;
        if (hm) {
          act = __ffsll((long long)hm) - 1;
          used = __popcll(nz & ((2ull << act) - 1ull));
        } else {
          act = A - 1;
          used = __popcll(nz);
        }
        if (lane == 0) {
          actions[e] = act;
          if (act_lds) act_lds[e] = (int16_t)act;
        }
        o += used;
      }
      if (lane == 0) any_zero = o;                       // the consumed-draw count, like the fast paths leave it
    }
    __syncthreads();
  }
  // Every path has passed a barrier since the actions were written: the caller may read act_lds without another one.
  // The stream position goes back in numpy's convention (pos in [0,624], regenerate lazily) -- by the LAST wave, so that
  // the first ones are already back in the caller's bookkeeping meanwhile.
  if (tid >= 192) {
    const int lane = tid - 192;
    const int o = any_zero;
    const uint32_t abs_pos = pos + 2u * (uint32_t)o;
    int fb = (int)(abs_pos / 624u);
    uint32_t np = abs_pos % 624u;
    if (np == 0 && abs_pos > 0) {
      fb -= 1;
      np = 624;
    }
    if (fb > 0) {
      if (pre_ok) {       // the blocks stayed in the record that came with the doubles
        for (int i = lane; i < 624; i += 64) mt_state[i] = ahead->blocks[(long)fb * 624 + i];
      } else {
        for (int i = lane; i < 624; i += 64) mt_state[i] = blocks[(long)fb * 624 + i];
      }
    }
    if (lane == 0) mt_state[624] = np;
  }
  return true;
}

template <int LDSC>
__global__ __launch_bounds__(256) void sample_mt_kernel(const float* __restrict__ probs, int N, int A,
                                                        uint32_t* __restrict__ mt_state, double* __restrict__ pj_g,
                                                        double* __restrict__ u_g, uint32_t* __restrict__ blocks_g,
                                                        int32_t* __restrict__ actions) {
  sample_mt_body<LDSC>(probs, N, A, mt_state, pj_g, u_g, blocks_g, actions, nullptr);
}

// =============================================================================================
// Frame preprocessing + stacking.
struct Lut84 {
  int v[84];
};
// PIL ImagingScaleAffine (nearest): position accumulated in double, then truncated
// (oracle/preprocess.py:_pil_nearest_lut; verified against PIL there).
constexpr Lut84 make_lut(int src) {
  Lut84 l{};
  const double s = (double)src / 84.0;
  double xo = 0.0 + s * 0.5;
  for (int x = 0; x < 84; ++x) {
    l.v[x] = (int)xo;
    xo += s;
  }
  return l;
}
__constant__ Lut84 kRowLut = make_lut(210);
__constant__ Lut84 kColLut = make_lut(160);

__device__ __forceinline__ uint32_t gray601(uint32_t r, uint32_t g, uint32_t b) {
  return (r * 19595u + g * 38470u + b * 7471u + 32768u) >> 16;
}

constexpr int PRE_ROWS_PER_BAND = 12;  // 84 output rows = PRE_BANDS (7) bands of 12

// grid (N, 7), 256 threads: a workgroup builds 12 output rows of one environment in ONE pass.
//   stage   the 2 x 12 source rows the band's output rows map to (PIL nearest: kRowLut) go to LDS with one 16-byte load per
//           thread (gray: 240 of the 256 threads, 3,840 B; RGB: three loads per thread, 11,520 B) -- whole 160- / 480-byte
//           rows, so every 128-byte line fetched is used in full;
//   gather  after the one barrier, thread q < 252 owns output quad (row q / 21, pixels 4 (q % 21) ..+3): four column
//           gathers per frame from LDS (kColLut), max of the two frames (atari_emulator.py:72: max before resize == after),
//           and the 4-deep history shift on whole pixels: out = (old >> 8) | (new << 24)  (channel 0 = oldest = lowest
//           byte; environment.py:66-71) -- one 16-byte load of the old stack (requested before the staging loads, so it
//           travels with them) and one 16-byte store per thread.
// In-place (stack_out == stack_in) is safe: a thread reads and writes the same 16 bytes.
template <bool RGB>
__global__ __launch_bounds__(256) void preprocess_stack_kernel(const uint8_t* __restrict__ raw, int N,
                                                               const uint32_t* stack_in, uint32_t* stack_out,
                                                               uint32_t* __restrict__ stack_out2,
                                                               const uint8_t* __restrict__ push_mask,
                                                               const uint8_t* __restrict__ reset_mask,
                                                               const float* __restrict__ reset_when_zero) {
  constexpr int ROWB = RGB ? 480 : 160;           // bytes per source row
  constexpr int VPR = ROWB / 16;                  // 16-byte vectors per source row
  constexpr int SRC_VEC = PRE_ROWS_PER_BAND * 2 * VPR;      // 240 (gray) / 720 (RGB)
  constexpr int QPR = OBS_W / 4;                  // 21 output quads per row
  __shared__ uint4 rows[SRC_VEC];                 // [band row][frame][ROWB bytes]
  const int e = blockIdx.x;
  const int band = blockIdx.y;
  const int tid = threadIdx.x;
  const bool push = push_mask ? (push_mask[e] != 0) : true;
  bool reset = reset_mask ? (reset_mask[e] != 0) : false;
  if (reset_when_zero) reset = reset || (reset_when_zero[e] == 0.0f);
  const bool has_quad = tid < PRE_ROWS_PER_BAND * QPR;       // 252
  const int qy = tid / QPR, qx = tid - qy * QPR;
  const long quad = ((long)e * OBS_PIX + (band * PRE_ROWS_PER_BAND + qy) * OBS_W) / 4 + qx;
  uint4 old = make_uint4(0u, 0u, 0u, 0u);
  if (has_quad) old = reinterpret_cast<const uint4*>(stack_in)[quad];
  if (push) {
    const uint8_t* fr = raw + (long)e * 2 * PAAC_RAW_H * ROWB;
#pragma unroll
    for (int v = tid; v < SRC_VEC; v += 256) {
      const int r = v / (2 * VPR), rem = v - r * (2 * VPR);
      const int f = rem / VPR, c = rem - f * VPR;
      const int ry = kRowLut.v[band * PRE_ROWS_PER_BAND + r];
      rows[v] = *reinterpret_cast<const uint4*>(fr + ((long)f * PAAC_RAW_H + ry) * ROWB + c * 16);
    }
  }
  __syncthreads();
  if (!has_quad) return;
  uint4 outv = old;
  if (push) {
    const uint8_t* r0 = reinterpret_cast<const uint8_t*>(rows) + (qy * 2) * ROWB;
    const uint8_t* r1 = r0 + ROWB;
    const uint32_t o[4] = {old.x, old.y, old.z, old.w};
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cx = kColLut.v[qx * 4 + k];
      uint32_t v0, v1;
      if (RGB) {
        v0 = gray601(r0[cx * 3], r0[cx * 3 + 1], r0[cx * 3 + 2]);
        v1 = gray601(r1[cx * 3], r1[cx * 3 + 1], r1[cx * 3 + 2]);
      } else {
        v0 = r0[cx];
        v1 = r1[cx];
      }
      const uint32_t nv = v0 > v1 ? v0 : v1;
      w[k] = ((reset ? 0u : o[k]) >> 8) | (nv << 24);
    }
    outv = make_uint4(w[0], w[1], w[2], w[3]);
  }
  reinterpret_cast<uint4*>(stack_out)[quad] = outv;
  if (stack_out2) reinterpret_cast<uint4*>(stack_out2)[quad] = outv;
}

// =============================================================================================
// Synthetic environments (spec: paac_amd/synthetic.py); device helpers in synth_dev.h.
// Path A: one new 84x84 plane per step.  grid (N, 7), 256 threads; one dword (pixel x 4 channels) per thread-iteration.
// force_reset: step 0 of every environment from an empty history (paac_synth_reset; st.stack_in == st.stack_out, no records).
__global__ __launch_bounds__(256) void synth_step_a_kernel(const SynthStep st, const int32_t* __restrict__ actions,
                                                           int force_reset) {
  const int e = blockIdx.x;
  const int band = blockIdx.y;
  const uint64_t id = force_reset ? 0ull : st.id();
  if (!force_reset && band == 0 && threadIdx.x == 0)
    synth_bookkeep(synth_key(st.seed, st.env_offset + (uint32_t)e, id), e, actions, st.thresh, st.rec);
  synth_shift_band(st.seed, st.env_offset, id, st.thresh, e * PRE_BANDS + band, st.stack_in, st.stack_out, st.stack_out2,
                   force_reset != 0);
}

// One (environment, band) unit of the step's frame work: path B's raw screen pair (the preprocess launch follows) or the shift.
__device__ __forceinline__ void step_unit(const SynthStep& st, uint64_t id, int unit) {
  if (st.raw) synth_raw_unit(st.seed, st.env_offset, id, unit, st.raw);
  else synth_shift_band(st.seed, st.env_offset, id, st.thresh, unit, st.stack_in, st.stack_out, st.stack_out2);
}

// Path A with the numpy-parity sampler folded in: workgroup 0 runs the (inherently serial) MT19937 sampler and then
// the per-env bookkeeping, the other N*7 workgroups shift the observation stacks meanwhile -- the new frame and the
// terminal flag of the synthetic environments do not depend on the action, only reward bookkeeping does.  One launch
// per time step instead of two.  LDSC = 2 (large shards: up to 2304 draws): the sampler workgroup takes most of a CU's LDS,
// which every workgroup of the launch then reserves -- so the stacks are shifted by one workgroup per environment (all 7
// bands) instead of one per band.
template <int LDSC, bool FOLD = false>
__global__ __launch_bounds__(256) void synth_step_a_mt_kernel(const float* __restrict__ probs, int A,
                                                              uint32_t* __restrict__ mt_state,
                                                              int32_t* __restrict__ actions, const SynthStep st,
                                                              const MultiWalk mw, const MtAhead* __restrict__ ahead,
                                                              const RowsHeadsHook hs) {
  const int N = st.N;
  const uint64_t id = st.id();
  const int samplers = mw.W > 0 ? mw.W : 1;          // sampler workgroups in front of the shift workgroups
  if ((int)blockIdx.x < samplers) {
    __shared__ int16_t act_s[mt_lds_d(LDSC)];
    // the running episode totals do not depend on the sampler: request them before it (first 256 environments)
    const int e0 = threadIdx.x < N ? threadIdx.x : 0;
    // (no step: sampler only -- launch_sample_mt_probs; one workgroup)
    const float ep_reward0 = st.active() ? st.rec.ep_reward[e0] : 0.f;
    const int32_t ep_len0 = st.active() ? st.rec.ep_len[e0] : 0;
    // (ends past a barrier; with several sampler workgroups only the one that finishes the walks goes on)
    // hs.partial: the heads were NOT finished by a launch of their own -- every sampler workgroup finishes those of the
    // environments its walks visit (paac_act_step_mt, large shards); otherwise `probs` holds all of them
    // (FOLD is a template argument: the two bodies' LDS arrays would otherwise both count against the workgroup)
    bool go_on;
    if constexpr (FOLD)
      go_on = sample_mt_body<LDSC, RowsHeadsHook>(nullptr, N, A, mt_state, nullptr, nullptr, nullptr, actions, act_s, nullptr, nullptr,
                                                  hs, mw, ahead);
    else
      go_on = sample_mt_body<LDSC>(probs, N, A, mt_state, nullptr, nullptr, nullptr, actions, act_s, nullptr, nullptr,
                                   NoProbsHook(), mw, ahead);
    if (!go_on || !st.active()) return;
    MISC_STAMP(7);
    for (int e = threadIdx.x; e < N; e += 256) {
      const uint32_t key = synth_key(st.seed, st.env_offset + (uint32_t)e, id);
      if (e < 256)
        synth_bookkeep_with(key, e, act_s[e], st.thresh, ep_reward0, ep_len0, st.rec);
      else
        synth_bookkeep_with(key, e, act_s[e], st.thresh, st.rec.ep_reward[e], st.rec.ep_len[e], st.rec);
    }
    MISC_STAMP(8);
    return;
  }
  if constexpr (LDSC == 2) {
    // every workgroup of this launch reserves the sampler's LDS, so a CU holds one: the (environment, band) units are dealt
    // over as many shift workgroups as fit beside the sampler workgroups in ONE round of the CUs
    const int nshift = (int)gridDim.x - samplers;
    for (int u = (int)blockIdx.x - samplers; u < N * PRE_BANDS; u += nshift) {
      step_unit(st, id, u);
    }
  } else {
    step_unit(st, id, (int)blockIdx.x - samplers);
  }
}

// Heads finish + sampler + bookkeeping of one acting step, by one workgroup's first 256 threads: sums the fc kernel's per-tile
// head partials (csrc/fc_heads.h), adds the biases, takes the softmax -- probabilities straight into LDS for the sampler (and
// to HBM for the learner's records) -- then samples and does the environments' bookkeeping (rewards_out == nullptr: none, the
// host environments' policy + sampler).  Called by workgroup 0 of the step launch below and by the workgroup that rides the
// NEXT fc launch in the pipelined step (ActRiderDev) or the flush launch: one routine, the same bits.
// id: the step's id; lg_s: kFcHeadsMaxRows * 33 floats of LDS.  ONE_SET: the two sampler bodies share one set of LDS arrays
// (the riders, which must leave room for an fc workgroup on their CU); otherwise each has its own (mt_lds).
// FIN (a second front end, the ridden fc launch behind a conv tower that carried the heads finish: `finished` holds what the
// hook would compute): the record's words are requested with the state words in one round trip and parked where the hook leaves
// its results (ParkedRecordHook); everything behind that point -- walks, the exact-zero fallback, bookkeeping -- is the same
// code.  Such a kernel holds neither the hook nor its 64 partials per thread.
template <bool ONE_SET, bool FIN = false>
__device__ __forceinline__ void act_sample_body(const float* __restrict__ partial, int ntiles, const float* __restrict__ ba,
                                                const float* __restrict__ bc, float* __restrict__ probs_out,
                                                float* __restrict__ values_out, int A, uint32_t* __restrict__ mt_state,
                                                int32_t* __restrict__ actions, uint64_t seed, uint32_t env_offset, int N,
                                                uint32_t thresh, uint64_t id, float* rewards_out, float* masks_out,
                                                float* ep_reward, int32_t* ep_len, FinishedRing* fin,
                                                const MtAhead* __restrict__ ahead, float* lg_s,
                                                const ActFinishRecord* __restrict__ finished = nullptr) {
  __shared__ int16_t act_s[kFcHeadsMaxRows];
  __shared__ float probs_sh[kFcHeadsMaxRows * 32];
  MISC_STAMP(14);
  // nothing below depends on these: request them before the head sums
  uint32_t stw[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) stw[k] = mt_state[min((int)threadIdx.x + k * 256, 624)];
  const int e0 = threadIdx.x < N ? threadIdx.x : 0;
  const bool env_step = rewards_out != nullptr;          // SynthStep::active(); false: policy + sampler only (host environments)
  const float ep_reward0 = env_step ? ep_reward[e0] : 0.f;
  const int32_t ep_len0 = env_step ? ep_len[e0] : 0;
  // ... and the action-independent half of environment e0's bookkeeping
  const uint32_t key0 = synth_key(seed, env_offset + (uint32_t)e0, id);
  const uint32_t hr5 = synth_reward_slot(key0);
  const bool term0 = synth_terminal(key0, thresh);
  if constexpr (FIN) {
    static_assert(ONE_SET, "the finished front end is the riders'");
    const int tid = threadIdx.x, D = N * (A - 1), NA = N * A;      // D <= 192, NA <= 224 (kActFinMaxN, kActFinMaxA)
    const double pj = finished->pj[tid < D ? tid : 0], thr = finished->thr[tid < D ? tid : 0];
    const float pr = finished->probs[tid < NA ? tid : 0];
    const bool zero = (finished->any_zero[0] | finished->any_zero[1] | finished->any_zero[2] | finished->any_zero[3]) != 0;
    sample_mt_body<1, ParkedRecordHook, 0>(nullptr, N, A, mt_state, nullptr, nullptr, nullptr, actions, act_s, probs_sh, stw,
                                           ParkedRecordHook{pj, thr, pr, zero, D, NA, probs_sh},
                                           MultiWalk{nullptr, nullptr, nullptr, 0}, ahead);
  } else if (N <= kActFinMaxN && A <= kActFinMaxA && ntiles <= kActFinMaxTiles) {
    // (row = tid >> 3, output = tid & 7): the partials are requested now; summed, turned into probabilities and into
    // conditional probabilities in registers after the sampler's state blocks and doubles (FusedHeadsHook)
    float pv[64];
    float bias;
    heads_partials_request(partial, ntiles, ba, bc, N, A, (int)threadIdx.x, pv, bias);
    sample_mt_body<1, FusedHeadsHook, ONE_SET ? 0 : 1>(nullptr, N, A, mt_state, nullptr, nullptr, nullptr, actions, act_s, probs_sh, stw,
                      FusedHeadsHook{pv, bias, ntiles, N, A, probs_sh, probs_out, values_out},
                      MultiWalk{nullptr, nullptr, nullptr, 0}, ahead);
  } else {
    heads_from_partials(partial, ntiles, N, A, ba, bc, lg_s, probs_sh, nullptr, probs_out, values_out, nullptr, nullptr,
                        nullptr);
    sample_mt_body<1>(nullptr, N, A, mt_state, nullptr, nullptr, nullptr, actions, act_s, probs_sh, stw, NoProbsHook(),
                      MultiWalk{nullptr, nullptr, nullptr, 0}, ahead);
  }
  MISC_STAMP(7);
  // (the sampler body ends past a barrier; its last wave is still writing the stream position back)
  if (env_step && (int)threadIdx.x < N)       // N <= 64 here: one environment per thread
    synth_bookkeep_hashed(hr5, term0, e0, act_s[e0], ep_reward0, ep_len0, StepRecords{rewards_out, masks_out, ep_reward, ep_len, fin});
  MISC_STAMP(8);
}

// The step launch with the heads finish in front of the sampler: workgroup 0 is act_sample_body, the other N * 7 shift the
// observation stacks meanwhile.  One launch per step for heads + sampler + env step.
// (The step's arguments one by one, not a SynthStep by value like the other step kernels: with the block by value the compiler
// fetches all of it in the entry block, the values the bookkeeping needs after the sampler then sit in SGPRs through the sampler
// instead of being loaded behind it, and the launch measured 7.16 us against 6.84 us at 32 x 4.  DESIGN.md.)
__global__ __launch_bounds__(256) void synth_step_a_mth_kernel(const float* __restrict__ partial, int ntiles,
                                                               const float* __restrict__ ba, const float* __restrict__ bc,
                                                               float* __restrict__ probs_out, float* __restrict__ values_out,
                                                               int A, uint32_t* __restrict__ mt_state,
                                                               int32_t* __restrict__ actions, uint64_t seed,
                                                               uint32_t env_offset, int N, uint32_t thresh,
                                                               const uint64_t* __restrict__ step_base, uint64_t step_off,
                                                               const uint32_t* __restrict__ stack_in,
                                                               uint32_t* __restrict__ stack_out,
                                                               uint32_t* __restrict__ stack_out2, float* rewards_out,
                                                               float* masks_out, float* ep_reward, int32_t* ep_len,
                                                               FinishedRing* fin, uint32_t* __restrict__ raw,
                                                               const MtAhead* __restrict__ ahead) {
  const uint64_t id = (step_base ? *step_base : 0ull) + step_off + 1ull;
  if (blockIdx.x == 0) {
    __shared__ float lg_s[kFcHeadsMaxRows * 33];
    act_sample_body<false>(partial, ntiles, ba, bc, probs_out, values_out, A, mt_state, actions, seed, env_offset, N, thresh, id,
                    rewards_out, masks_out, ep_reward, ep_len, fin, ahead, lg_s);
    return;
  }
  if (raw) synth_raw_unit(seed, env_offset, id, (int)blockIdx.x - 1, raw);     // path B: the preprocess launch follows
  else synth_shift_band(seed, env_offset, id, thresh, (int)blockIdx.x - 1, stack_in, stack_out, stack_out2);
}

// The pipelined acting step (csrc/api.hip: paac_act_step_pipe): the sampler leaves the dependent chain tower -> fc -> sampler.
// In the path-A synthetic environments the new frame and the terminal flag depend on (seed, env, step id) only -- what the
// step launch above already relies on to shift beside the sampler -- so the shift of step t needs nothing step t computes,
// tower(t + 1) needs only that shift, and nobody reads step t's sample before the update.  fc(t)'s launch therefore carries
// (fc_heads.h: RIDER) the shift of step t, dealt over the fc workgroups, and one extra workgroup, first in the grid, that is
// act_sample_body of step t - 1 on the partial region fc(t - 1) wrote (fc(t) writes the other one).  No workgroup waits for
// another: every rider reads only what an earlier launch wrote.  (Device games, whose frame depends on the action, keep their
// routes.)  The fc kernels run 448 or 576 threads, the sampler body and the shift are written for 256: a rider workgroup's
// surplus waves return before the first barrier, an fc workgroup's take no part in the shift.
template <bool FIN>
struct ActRiderDev {
  ActRider r;
  unsigned front_wgs() const { return r.owed.partial ? 1u : 0u; }      // the owed sample's workgroup
  __device__ __forceinline__ bool front(int& bid, int& nfc, float* lds) const {
    const int ns = r.owed.partial ? 1 : 0;
    if (bid < ns) {
      if (threadIdx.x >= 256) return true;
      const ActSample& o = r.owed;
      const uint64_t id = (o.step_base ? *o.step_base : 0ull) + o.step_off + 1ull;
      act_sample_body<true, FIN>(o.partial, o.ntiles, o.ba, o.bc, o.probs_out, o.values_out, o.A, o.mt_state, o.actions, o.seed,
                                 o.env_offset, o.N, o.thresh, id, o.rec.rewards, o.rec.masks, o.rec.ep_reward, o.rec.ep_len,
                                 o.rec.fin, nullptr, lds, o.finished);
      return true;
    }
    bid -= ns;
    nfc -= ns;
    return false;
  }
  // fc workgroup `bid` of nfc shifts units bid, bid + nfc, ...: the first one around its K loop, the others behind it
  __device__ __forceinline__ uint4 shift_load(const int bid) const {
    const SynthStep& st = r.shift;
    if (st.stack_in == nullptr || threadIdx.x >= 256 || bid >= st.N * PRE_BANDS) return make_uint4(0u, 0u, 0u, 0u);
    return synth_shift_load(bid, st.stack_in);
  }
  __device__ __forceinline__ void shift_store(const int bid, const int nfc, const uint4 old) const {
    const SynthStep& st = r.shift;
    if (st.stack_in == nullptr || threadIdx.x >= 256) return;
    const uint64_t id = st.id();
    const int units = st.N * PRE_BANDS;
    if (bid < units) synth_shift_store(st.seed, st.env_offset, id, st.thresh, bid, old, st.stack_out, st.stack_out2);
    for (int u = bid + nfc; u < units; u += nfc)
      synth_shift_band(st.seed, st.env_offset, id, st.thresh, u, st.stack_in, st.stack_out, st.stack_out2);
  }
};

// The flush: the owed sample as a launch of its own (one workgroup), for a caller that ends a run of pipelined steps without
// a forward behind it.
__global__ __launch_bounds__(256) void act_sample_flush_kernel(const ActSample o) {
  __shared__ float lg_s[kFcHeadsMaxRows * 33];
  const uint64_t id = (o.step_base ? *o.step_base : 0ull) + o.step_off + 1ull;
  act_sample_body<true>(o.partial, o.ntiles, o.ba, o.bc, o.probs_out, o.values_out, o.A, o.mt_state, o.actions, o.seed, o.env_offset,
                  o.N, o.thresh, id, o.rec.rewards, o.rec.masks, o.rec.ep_reward, o.rec.ep_len, o.rec.fin, nullptr, lg_s);
}

// Path B, stage 1: generate the two raw 210x160 gray frames of this step + bookkeeping.
// grid (N, 8), 256 threads; 16800 dwords per env.
__global__ __launch_bounds__(256) void synth_raw_kernel(const SynthStep st, const int32_t* __restrict__ actions,
                                                        int force_reset) {
  const int e = blockIdx.x;
  const uint64_t id = force_reset ? 0ull : st.id();
  const uint32_t key = synth_key(st.seed, st.env_offset + (uint32_t)e, id);
  if (!force_reset && blockIdx.y == 0 && threadIdx.x == 0) synth_bookkeep(key, e, actions, st.thresh, st.rec);
  uint32_t* __restrict__ raw = st.raw;
  const uint32_t rkey = key ^ 0x5bd1e995u;
  constexpr int WORDS = 2 * PAAC_RAW_H * PAAC_RAW_W / 4;  // 16800
  uint4* out = reinterpret_cast<uint4*>(raw + (long)e * WORDS);
  for (int q = blockIdx.y * 256 + threadIdx.x; q < WORDS / 4; q += 256 * gridDim.y)     // one 16-byte store per 4 words
    out[q] = make_uint4(synth_word(rkey, (uint32_t)(4 * q)), synth_word(rkey, (uint32_t)(4 * q + 1)),
                        synth_word(rkey, (uint32_t)(4 * q + 2)), synth_word(rkey, (uint32_t)(4 * q + 3)));
}

// Path B, second launch of a step: the observation stacks from the raw screen pairs the step launch has just written
// (max of the two screens, PIL-nearest resize, history push; environments whose mask is 0 -- terminal -- restart from an
// empty history, like paac_synth_step's path B).
static void launch_preprocess_after_step(const SynthStep& st, hipStream_t s) {
  ProfScope ps(g_prof_ctx, F_PREPROCESS_STACK, st.N, s);
  launch_k(preprocess_stack_kernel<false>, dim3(st.N, PRE_BANDS), dim3(256), s, PROF_WHOLE, (const uint8_t*)st.raw, st.N,
           st.stack_in, st.stack_out, st.stack_out2, (const uint8_t*)nullptr, (const uint8_t*)nullptr,
           (const float*)st.rec.masks);
}

// The arguments of one environment step as an entry point receives them -> st, behind the refusals the step entries share:
// null stacks or records (`what`: the entry's words for that), and, where the entry forbids it, stacks shifted in place.
int synth_step_of(const char* fn, const char* what, bool in_place_ok, SynthStep* st, uint64_t seed, uint32_t env_offset, int N,
                  uint32_t thresh, const uint64_t* step_base, uint64_t step_off, const uint8_t* stack_in, uint8_t* stack_out,
                  uint8_t* stack_out2, float* rewards, float* masks, float* ep_reward, int32_t* ep_len, void* finished,
                  uint8_t* raw_scratch) {
  PAAC_REQUIRE(stack_in && stack_out && rewards && masks && ep_reward && ep_len, "%s: %s", fn, what);
  PAAC_REQUIRE(in_place_ok || (stack_in != stack_out && stack_in != stack_out2), "%s: the step cannot shift the stacks in place",
               fn);
  *st = SynthStep{seed, env_offset, N, thresh, step_base, step_off, (const uint32_t*)stack_in, (uint32_t*)stack_out,
                  (uint32_t*)stack_out2, StepRecords{rewards, masks, ep_reward, ep_len, (FinishedRing*)finished},
                  (uint32_t*)raw_scratch};
  return 0;
}

// (st.N rows; an inactive st -- no environment step -- runs workgroup 0 alone: heads finish + sampler)
int launch_sample_env_step_heads(const HeadsPartials& hp, float* probs_out, int A, uint32_t* mt_state, int32_t* actions,
                                 const SynthStep& st, const void* mt_ahead, hipStream_t s) {
  {
    ProfScope ps(g_prof_ctx, F_SAMPLE_ENV_STEP, st.N, s);
    launch_k(synth_step_a_mth_kernel, dim3(st.active() ? 1 + st.N * PRE_BANDS : 1), dim3(256), s, PROF_WHOLE, hp.partial,
             hp.ntiles, hp.ba, hp.bc, probs_out, hp.values_out, A, mt_state, actions, st.seed, st.env_offset, st.N, st.thresh,
             st.step_base, st.step_off, st.stack_in, st.stack_out, st.stack_out2, st.rec.rewards, st.rec.masks, st.rec.ep_reward,
             st.rec.ep_len, st.rec.fin, st.raw, reinterpret_cast<const MtAhead*>(mt_ahead));
  }
  if (st.raw) launch_preprocess_after_step(st, s);
  return 0;
}

int launch_act_sample_flush(const ActSample& owed, hipStream_t s) {
  ProfScope ps(g_prof_ctx, F_SAMPLE_ENV_STEP, owed.N, s);
  launch_k(act_sample_flush_kernel, dim3(1), dim3(256), s, PROF_WHOLE, owed);
  return 0;
}

// The acting fc launch with its riders, as csrc/net_fwd.hip asks for it (fc_heads.h: launch_fc_heads; the ridden instantiations
// are compiled here, beside the sampler they carry).
// Two forms: a debt whose heads the conv tower in front has finished -- the instantiation with the record front end alone
// (Nature: the tower that carries the finish is its) --, otherwise the sampler with the heads finish of its own.  (A launch with
// nothing to carry -- that tower shifted the frames and no sample is owed -- is the forward's plain one.)
int launch_fc_heads_rider(bool nature, const FcHeadsArgs& a, const ActRider& r, hipStream_t s) {
  if (r.owed.partial && r.owed.finished) {
    if (nature) return launch_fc_heads<NatureNet>(a, ActRiderDev<true>{r}, s);
    set_error("fc launch riders: a finished debt needs the Nature conv tower in front");
    return -1;
  }
  if (nature) return launch_fc_heads<NatureNet>(a, ActRiderDev<false>{r}, s);
  return launch_fc_heads<OtherNet>(a, ActRiderDev<false>{r}, s);
}

// (arguments validated by paac_returns_norm_tick, csrc/api.hip)
int launch_returns_norm(const paac_returns* ret, const float* v_boot, float* adv_n, double* stats, hipStream_t s) {
  const TruncArgs rt = returns_args(ret, v_boot);
  if (rt.truncs) {
    launch_k(returns_norm_kernel<TruncArgs>, dim3(1), dim3(kNormThreads), s, PROF_WHOLE, rt, adv_n, stats);
  } else if (rt.gae) {
    const GaeArgs& rg = rt;
    launch_k(returns_norm_kernel<GaeArgs>, dim3(1), dim3(kNormThreads), s, PROF_WHOLE, rg, adv_n, stats);
  } else {
    const ReturnsArgs& rn = rt;
    launch_k(returns_norm_kernel<ReturnsArgs>, dim3(1), dim3(kNormThreads), s, PROF_WHOLE, rn, adv_n, stats);
  }
  return 0;
}

// The standalone scan behind paac_nstep_returns[_tick] / paac_gae_returns[_tick], which check what is theirs alone (lambda,
// the bookkeeping pointers): `name` is the entry point's, for the message.
static int launch_returns_scan(const char* name, int estimator, const float* v_boot, const float* rewards, const float* masks,
                               const float* values, int T, int N, double gamma, double gae_lambda, float* y, float* adv,
                               const CycleTick& ct, paac_stream_t stream, const float* truncs = nullptr) {
  PAAC_REQUIRE(T > 0 && N > 0, "%s: T=%d N=%d", name, T, N);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(g_prof_ctx, F_NSTEP_RETURNS, N * T, s);
  if (truncs) {       // --bootstrap_truncated: the truncation-aware scan (paac_returns_scan with a plane)
    auto* kernel = estimator == kEstGae ? returns_scan_kernel<kEstGae, const float*> : returns_scan_kernel<kEstNstep, const float*>;
    launch_k(kernel, dim3((N + 63) / 64), dim3(128), s, PROF_WHOLE, v_boot, rewards, masks, values, T, N, gamma,
             gamma * gae_lambda, y, adv, ct, truncs);
    PAAC_CHECK_HIP(hipGetLastError());
    return 0;
  }
  auto* kernel = estimator == kEstGae ? returns_scan_kernel<kEstGae> : returns_scan_kernel<kEstNstep>;
  launch_k(kernel, dim3((N + 63) / 64), dim3(128), s, PROF_WHOLE, v_boot, rewards, masks, values, T, N, gamma,
           gamma * gae_lambda, y, adv, ct, NoPlane{});
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace paac

using namespace paac;

// =============================================================================================
// C-ABI wrappers
extern "C" {

#ifdef PAAC_DMM_STAMPS
void paac_debug_set_misc_stamps(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_misc_stamps), &p, sizeof(p)); }
#endif

int paac_nstep_returns(const float* v_boot, const float* rewards, const float* masks, const float* values, int T, int N,
                       double gamma, float* y, float* adv, paac_stream_t stream) {
  return launch_returns_scan("paac_nstep_returns", kEstNstep, v_boot, rewards, masks, values, T, N, gamma, 0.0, y, adv,
                             CycleTick{}, stream);
}

int paac_nstep_returns_tick(const float* v_boot, const float* rewards, const float* masks, const float* values, int T,
                            int N, double gamma, float* y, float* adv, int64_t* global_step_dev, int64_t increment,
                            double initial_lr, int64_t lr_annealing_steps, float* lr_out_dev, uint64_t* tick_dev,
                            uint64_t tick_inc, paac_stream_t stream) {
  PAAC_REQUIRE(global_step_dev && lr_out_dev && lr_annealing_steps > 0, "paac_nstep_returns_tick: bad arguments");
  return launch_returns_scan("paac_nstep_returns_tick", kEstNstep, v_boot, rewards, masks, values, T, N, gamma, 0.0, y, adv,
                             CycleTick{global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc},
                             stream);
}

int paac_gae_returns(const float* v_boot, const float* rewards, const float* masks, const float* values, int T, int N,
                     double gamma, double gae_lambda, float* y, float* adv, paac_stream_t stream) {
  PAAC_REQUIRE(gae_lambda >= 0.0 && gae_lambda <= 1.0, "paac_gae_returns: gae_lambda %g outside [0, 1]", gae_lambda);
  return launch_returns_scan("paac_gae_returns", kEstGae, v_boot, rewards, masks, values, T, N, gamma, gae_lambda, y, adv,
                             CycleTick{}, stream);
}

int paac_gae_returns_tick(const float* v_boot, const float* rewards, const float* masks, const float* values, int T,
                          int N, double gamma, double gae_lambda, float* y, float* adv, int64_t* global_step_dev,
                          int64_t increment, double initial_lr, int64_t lr_annealing_steps, float* lr_out_dev,
                          uint64_t* tick_dev, uint64_t tick_inc, paac_stream_t stream) {
  PAAC_REQUIRE(gae_lambda >= 0.0 && gae_lambda <= 1.0, "paac_gae_returns_tick: gae_lambda %g outside [0, 1]", gae_lambda);
  PAAC_REQUIRE(global_step_dev && lr_out_dev && lr_annealing_steps > 0, "paac_gae_returns_tick: bad arguments");
  return launch_returns_scan("paac_gae_returns_tick", kEstGae, v_boot, rewards, masks, values, T, N, gamma, gae_lambda, y, adv,
                             CycleTick{global_step_dev, increment, initial_lr, lr_annealing_steps, lr_out_dev, tick_dev, tick_inc},
                             stream);
}

// The four entries above from the argument block (estimator and bookkeeping by its fields), with the truncation plane.
int paac_returns_scan(const paac_returns* ret, paac_stream_t stream) {
  PAAC_REQUIRE(ret && ret->v_boot && ret->rewards && ret->masks && ret->values && ret->y_out && ret->adv_out,
               "paac_returns_scan: null argument");
  PAAC_REQUIRE(returns_estimator(ret) == PAAC_RETURNS_NSTEP || returns_estimator(ret) == PAAC_RETURNS_GAE,
               "paac_returns_scan: estimator %d (PAAC_RETURNS_NSTEP = 0, PAAC_RETURNS_GAE = 1)", returns_estimator(ret));
  PAAC_REQUIRE(ret->gae_lambda >= 0.0 && ret->gae_lambda <= 1.0, "paac_returns_scan: gae_lambda %g outside [0, 1]",
               ret->gae_lambda);
  PAAC_REQUIRE(!ret->global_step_dev || (ret->lr_out_dev && ret->lr_annealing_steps > 0),
               "paac_returns_scan: schedule bookkeeping needs lr_out_dev and lr_annealing_steps");
  const CycleTick ct{ret->global_step_dev, ret->increment, ret->initial_lr, ret->lr_annealing_steps, ret->lr_out_dev,
                     ret->tick_dev, ret->tick_inc};
  const bool gae = returns_estimator(ret) == PAAC_RETURNS_GAE;
  return launch_returns_scan("paac_returns_scan", gae ? kEstGae : kEstNstep, ret->v_boot, ret->rewards, ret->masks, ret->values,
                             ret->T, ret->N, ret->gamma, gae ? ret->gae_lambda : 0.0, ret->y_out, ret->adv_out, ct, stream,
                             returns_truncs(ret));
}

int paac_adv_normalize(const float* adv, int B, float* adv_n_out, double* stats_out, paac_stream_t stream) {
  PAAC_REQUIRE(adv && adv_n_out, "paac_adv_normalize: null argument");
  PAAC_REQUIRE(B > 0, "paac_adv_normalize: B=%d", B);
  launch_k(adv_normalize_kernel, dim3(1), dim3(kNormThreads), (hipStream_t)stream, PROF_WHOLE, adv, B, adv_n_out, stats_out);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_window_fields(int* n_f, int* n_i) {
  if (n_f) *n_f = kWinFieldsF;
  if (n_i) *n_i = kWinFieldsI;
  return 0;
}

int paac_window_fold(const paac_window_inputs* in, double* acc_f, int64_t* acc_i, paac_stream_t stream) {
  PAAC_REQUIRE(in, "paac_window_fold: in is null");
  PAAC_REQUIRE(acc_f, "paac_window_fold: acc_f is null");
  PAAC_REQUIRE(acc_i, "paac_window_fold: acc_i is null");
  PAAC_REQUIRE(in->values, "paac_window_fold: values is null");
  PAAC_REQUIRE(in->rewards, "paac_window_fold: rewards is null");
  PAAC_REQUIRE(in->masks, "paac_window_fold: masks is null");
  PAAC_REQUIRE(in->actions, "paac_window_fold: actions is null");
  PAAC_REQUIRE(in->y, "paac_window_fold: y is null");
  PAAC_REQUIRE(in->adv, "paac_window_fold: adv is null");
  PAAC_REQUIRE(in->loss, "paac_window_fold: loss is null");
  PAAC_REQUIRE(in->gnorm, "paac_window_fold: gnorm is null");
  PAAC_REQUIRE(in->T >= 1 && in->N >= 1 && (int64_t)in->T * in->N <= INT32_MAX, "paac_window_fold: T=%d N=%d (T * N < 1)", in->T,
               in->N);
  PAAC_REQUIRE(in->A >= 2 && in->A <= kWinActions, "paac_window_fold: A=%d outside [2, %d]", in->A, kWinActions);
  PAAC_REQUIRE(in->steps >= 1 && in->steps <= PAAC_PPO_STEPS_MAX, "paac_window_fold: steps=%d outside [1, %d]", in->steps,
               PAAC_PPO_STEPS_MAX);
  PAAC_REQUIRE(!in->ppo_stats || in->stats_cols == 2 || in->stats_cols == 3, "paac_window_fold: stats_cols=%d (2, or 3 with "
               "value_clip_fraction live)", in->stats_cols);
  PAAC_REQUIRE(!in->ppo_stats || (in->stats_first >= 0 && in->stats_first <= in->steps),
               "paac_window_fold: stats_first=%d outside [0, steps]", in->stats_first);
  launch_k(window_fold_kernel, dim3(1), dim3(kWinThreads), (hipStream_t)stream, PROF_WHOLE, *in, acc_f, acc_i);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_lr_step(int64_t* global_step_dev, int64_t increment, double initial_lr, int64_t lr_annealing_steps,
                 float* lr_out_dev, paac_stream_t stream) {
  PAAC_REQUIRE(global_step_dev && lr_out_dev && lr_annealing_steps > 0, "paac_lr_step: bad arguments");
  hipLaunchKernelGGL(lr_step_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, global_step_dev, increment, initial_lr,
                     lr_annealing_steps, lr_out_dev);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_counter_add(uint64_t* counter_dev, uint64_t inc, paac_stream_t stream) {
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter_dev, inc);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_debug_clock(uint64_t* out2_dev, paac_stream_t stream) {
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, out2_dev);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_sample_philox(const float* probs, int N, int A, uint64_t seed, const uint64_t* step_base_dev,
                       uint64_t step_offset, uint32_t env_offset, int32_t* actions, paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && A >= 2 && A <= 32, "paac_sample_philox: N=%d A=%d", N, A);
  ProfScope ps(g_prof_ctx, F_SAMPLE_PHILOX, N, (hipStream_t)stream);
  launch_k(sample_philox_kernel, dim3((N + 63) / 64), dim3(64), (hipStream_t)stream, PROF_WHOLE, probs, N, A, seed,
           step_base_dev, step_offset, env_offset, actions);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_minibatch_perms(int B, int epochs, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                         int32_t* perms_out, paac_stream_t stream) {
  PAAC_REQUIRE(perms_out, "paac_minibatch_perms: null perms_out");
  PAAC_REQUIRE(B > 0 && B <= PAAC_MINIBATCH_MAX_ROWS, "paac_minibatch_perms: B=%d outside [1, %d] (one workgroup's LDS sort)", B,
               PAAC_MINIBATCH_MAX_ROWS);
  PAAC_REQUIRE(epochs > 0 && epochs <= PAAC_PPO_EPOCHS_MAX, "paac_minibatch_perms: epochs=%d outside [1, %d]", epochs,
               PAAC_PPO_EPOCHS_MAX);
  static_assert(PAAC_MINIBATCH_MAX_ROWS == kPermMaxRows, "the sort's LDS array");
  int P = 1;
  while (P < B) P <<= 1;
  ProfScope ps(g_prof_ctx, F_MISC, B, (hipStream_t)stream);
  launch_k(minibatch_perms_kernel, dim3(epochs), dim3(kPermThreads), (hipStream_t)stream, PROF_WHOLE, B, P, seed, step_base_dev,
           step_offset, perms_out);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_gather_minibatch(const int32_t* perm, int B, const uint8_t* states, uint8_t* states_out, const int32_t* actions,
                          int32_t* actions_out, const float* y, float* y_out, const float* adv, float* adv_out,
                          const float* p_old, float* p_old_out, const float* v_old, float* v_old_out, paac_stream_t stream) {
  PAAC_REQUIRE(perm, "paac_gather_minibatch: null perm");
  PAAC_REQUIRE(B > 0 && B <= PAAC_MINIBATCH_MAX_ROWS, "paac_gather_minibatch: B=%d outside [1, %d]", B, PAAC_MINIBATCH_MAX_ROWS);
  // every array comes with its output; an output that overlaps its input would be read after it was written
  auto pair_ok = [&](const void* in, const void* out, size_t bytes, const char* name) {
    if ((in == nullptr) != (out == nullptr)) {
      set_error("paac_gather_minibatch: %s and %s_out must both be given or both be NULL", name, name);
      return false;
    }
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
    if (in && a < b + bytes && b < a + bytes) {
      set_error("paac_gather_minibatch: %s_out overlaps %s (the gather cannot run in place)", name, name);
      return false;
    }
    return true;
  };
  if (!pair_ok(states, states_out, (size_t)B * PAAC_OBS_BYTES, "states") || !pair_ok(actions, actions_out, (size_t)B * 4, "actions") ||
      !pair_ok(y, y_out, (size_t)B * 4, "y") || !pair_ok(adv, adv_out, (size_t)B * 4, "adv") ||
      !pair_ok(p_old, p_old_out, (size_t)B * 4, "p_old") || !pair_ok(v_old, v_old_out, (size_t)B * 4, "v_old"))
    return -1;
  PAAC_REQUIRE(((uintptr_t)states | (uintptr_t)states_out) % 16 == 0, "paac_gather_minibatch: states / states_out must be "
               "16-byte aligned");
  const bool small = actions || y || adv || p_old || v_old;
  PAAC_REQUIRE(states || small, "paac_gather_minibatch: nothing to gather");
  const GatherSmall g{actions, actions_out, y, y_out, adv, adv_out, p_old, p_old_out, v_old, v_old_out};
  const unsigned grid = (states ? (unsigned)B * kGatherParts : 0u) + (small ? (unsigned)(B + 255) / 256 : 0u);
  ProfScope ps(g_prof_ctx, F_MISC, B, (hipStream_t)stream);
  launch_k(gather_minibatch_kernel, dim3(grid), dim3(256), (hipStream_t)stream, PROF_WHOLE, perm, B,
           reinterpret_cast<const uint4*>(states), reinterpret_cast<uint4*>(states_out), g);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int64_t paac_sample_mt_scratch_bytes(int N, int A) {
  const int64_t D = (int64_t)N * (A - 1);
  const int64_t nblk = (624 + 2 * D) / 624 + 2;
  return D * 8 * 2 + nblk * 624 * 4 + 64;
}

int paac_sample_mt(const float* probs, int N, int A, uint32_t* mt_state, void* scratch, int32_t* actions,
                   paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && A >= 2 && A <= 32, "paac_sample_mt: N=%d A=%d", N, A);
  PAAC_REQUIRE(scratch && mt_state, "paac_sample_mt: null scratch/state");
  const int64_t D = (int64_t)N * (A - 1);
  double* pj = (double*)scratch;
  double* u = pj + D;
  uint32_t* blocks = (uint32_t*)(u + D);
  ProfScope ps(g_prof_ctx, F_SAMPLE_MT, N, (hipStream_t)stream);
  if (D <= MT_LDS_D)
    launch_k(sample_mt_kernel<1>, dim3(1), dim3(256), (hipStream_t)stream, PROF_WHOLE, probs, N, A, mt_state, pj, u,
             blocks, actions);
  else if (D <= MT_LDS_D2)
    launch_k(sample_mt_kernel<2>, dim3(1), dim3(256), (hipStream_t)stream, PROF_WHOLE, probs, N, A, mt_state, pj, u,
             blocks, actions);
  else
    launch_k(sample_mt_kernel<0>, dim3(1), dim3(256), (hipStream_t)stream, PROF_WHOLE, probs, N, A, mt_state, pj, u,
             blocks, actions);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_preprocess_stack(const uint8_t* raw, int is_rgb, int N, const uint8_t* stack_in, uint8_t* stack_out,
                          const uint8_t* push_mask, const uint8_t* reset_mask, paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && raw && stack_in && stack_out, "paac_preprocess_stack: bad arguments");
  dim3 grid(N, PRE_BANDS);
  ProfScope ps(g_prof_ctx, F_PREPROCESS_STACK, N, (hipStream_t)stream);
  if (is_rgb)
    launch_k(preprocess_stack_kernel<true>, grid, dim3(256), (hipStream_t)stream, PROF_WHOLE, raw, N,
             (const uint32_t*)stack_in, (uint32_t*)stack_out, (uint32_t*)nullptr, push_mask, reset_mask,
             (const float*)nullptr);
  else
    launch_k(preprocess_stack_kernel<false>, grid, dim3(256), (hipStream_t)stream, PROF_WHOLE, raw, N,
             (const uint32_t*)stack_in, (uint32_t*)stack_out, (uint32_t*)nullptr, push_mask, reset_mask,
             (const float*)nullptr);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_synth_reset(uint64_t seed, uint32_t env_offset, int N, uint8_t* stack_out, uint8_t* raw_scratch,
                     paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && stack_out, "paac_synth_reset: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  SynthStep st{};              // what a forced reset reads: the key, and the stacks shifted in place from an empty history
  st.seed = seed, st.env_offset = env_offset, st.N = N;
  st.stack_in = st.stack_out = (uint32_t*)stack_out, st.raw = (uint32_t*)raw_scratch;
  if (!raw_scratch) {
    hipLaunchKernelGGL(synth_step_a_kernel, dim3(N, PRE_BANDS), dim3(256), 0, s, st, (const int32_t*)nullptr, 1);
  } else {
    hipLaunchKernelGGL(synth_raw_kernel, dim3(N, 8), dim3(256), 0, s, st, (const int32_t*)nullptr, 1);
    // reset_mask = every env: reuse push semantics with an all-zero "mask" float is not available here,
    // so clear the stack first and push with reset handled by the zero fill.
    PAAC_CHECK_HIP(hipMemsetAsync(stack_out, 0, (size_t)N * PAAC_OBS_BYTES, s));
    hipLaunchKernelGGL((preprocess_stack_kernel<false>), dim3(N, PRE_BANDS), dim3(256), 0, s, raw_scratch, N,
                       (const uint32_t*)stack_out, (uint32_t*)stack_out, (uint32_t*)nullptr, (const uint8_t*)nullptr,
                       (const uint8_t*)nullptr, (const float*)nullptr);
  }
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_synth_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, uint32_t terminal_threshold,
                    const uint64_t* step_base_dev, uint64_t step_offset, const uint8_t* stack_in, uint8_t* stack_out,
                    uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                    void* finished, uint8_t* raw_scratch, paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && actions, "paac_synth_step: bad arguments");
  SynthStep st;
  if (synth_step_of("paac_synth_step", "bad arguments", true, &st, seed, env_offset, N, terminal_threshold, step_base_dev,
                    step_offset, stack_in, stack_out, stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished, raw_scratch))
    return -1;
  hipStream_t s = (hipStream_t)stream;
  {
    ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
    if (!raw_scratch) launch_k(synth_step_a_kernel, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, st, actions, 0);
    else launch_k(synth_raw_kernel, dim3(N, 8), dim3(256), s, PROF_WHOLE, st, actions, 0);
  }
  if (raw_scratch) launch_preprocess_after_step(st, s);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_debug_report_zero(int sampler_workgroup) {
  PAAC_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_zero_wg), &sampler_workgroup, sizeof(int)));
  return 0;
}

int64_t paac_walk_scratch_bytes(int N, int A) {
  if (N <= 0 || A < 2) return 0;
  const long nwk = mw_walks(N, A);
  return 64 + ((nwk * 2 + 63) / 64) * 64 + nwk * 8;
}

int paac_sample_mt_synth_step(const float* probs, int A, uint32_t* mt_state, int32_t* actions, uint64_t seed,
                              uint32_t env_offset, int N, uint32_t terminal_threshold, const uint64_t* step_base_dev,
                              uint64_t step_offset, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                              float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                              void* walk_scratch, int64_t walk_scratch_bytes, uint8_t* raw_scratch, paac_stream_t stream) {
  SynthStep st;
  if (synth_step_of("paac_sample_mt_synth_step", "null argument", true, &st, seed, env_offset, N, terminal_threshold,
                    step_base_dev, step_offset, stack_in, stack_out, stack_out2, rewards_out, masks_out, ep_reward, ep_len,
                    finished, raw_scratch))
    return -1;
  return launch_sample_mt_synth_step(probs, A, mt_state, actions, st, walk_scratch, walk_scratch_bytes, nullptr,
                                     (hipStream_t)stream, nullptr);
}

}  // extern "C"

namespace paac {
size_t mt_ahead_bytes() { return sizeof(MtAhead); }

// the step launch of launch_sample_mt_synth_step is the large-LDS sampler with its walks spread over several workgroups:
// only then can those workgroups finish the heads themselves (HeadsPartials)
static bool sampler_is_large(int N, int A) {
  return (int64_t)N * (A - 1) > MT_LDS_D || (long)N + (long)(A - 2) * N * (N - 1) / 2 > MT_TAB_MAX;
}
bool sampler_folds_heads(int N, int A, const void* walk_scratch) {
  return sampler_is_large(N, A) && walk_scratch != nullptr && mw_walks(N, A) <= 16384 && N <= 256 && A <= 32;
}

int launch_sample_mt_probs(const float* probs, int A, uint32_t* mt_state, int32_t* actions, int N, hipStream_t stream) {
  PAAC_REQUIRE(probs && mt_state && actions && N > 0 && N <= 64 && A >= 2 && A <= 32 && (int64_t)N * (A - 1) <= MT_LDS_D,
               "launch_sample_mt_probs: N=%d A=%d", N, A);
  SynthStep st{};              // no environment step: the sampler workgroup alone
  st.N = N;
  {
    ProfScope ps(g_prof_ctx, F_SAMPLE_ENV_STEP, N, stream);
    launch_k(synth_step_a_mt_kernel<1>, dim3(1), dim3(256), stream, PROF_WHOLE, probs, A, mt_state, actions, st,
             MultiWalk{nullptr, nullptr, nullptr, 0}, (const MtAhead*)nullptr,
             RowsHeadsHook{nullptr, 0, N, A, nullptr, nullptr, nullptr, nullptr});
  }
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// mt_ahead (nullable): the record a spare workgroup of the preceding fc launch left (csrc/mt_ahead.h)
int launch_sample_mt_synth_step(const float* probs, int A, uint32_t* mt_state, int32_t* actions, const SynthStep& st,
                                void* walk_scratch, int64_t walk_scratch_bytes, const void* mt_ahead, hipStream_t stream,
                                const HeadsPartials* heads) {
  const int N = st.N;
  PAAC_REQUIRE(N > 0 && A >= 2 && A <= 32, "paac_sample_mt_synth_step: N=%d A=%d", N, A);
  PAAC_REQUIRE((int64_t)N * (A - 1) <= MT_LDS_D2, "paac_sample_mt_synth_step: N*(A-1)=%ld exceeds the fused kernel's limit %d "
               "(use paac_sample_mt + paac_synth_step)", (long)N * (A - 1), MT_LDS_D2);
  PAAC_REQUIRE(probs && mt_state && actions, "paac_sample_mt_synth_step: null argument");
  RowsHeadsHook hs{nullptr, 0, N, A, nullptr, nullptr, nullptr, nullptr};
  {
  ProfScope ps(g_prof_ctx, F_SAMPLE_ENV_STEP, N, stream);
  // small shards: the small-LDS sampler, one shift workgroup per band; beyond 1024 draws or 64 environments (where the
  // two-level chase needs the large first-hit table): the large-LDS sampler, one shift workgroup per environment
  const bool large = sampler_is_large(N, A);
  PAAC_REQUIRE(!(heads && heads->partial) || sampler_folds_heads(N, A, walk_scratch),
               "paac_sample_mt_synth_step: unfinished heads need the multi-workgroup sampler (N=%d A=%d)", N, A);
  MultiWalk mw{nullptr, nullptr, nullptr, 0};
  if (large && walk_scratch != nullptr) {
    // the caller lent a (zero-initialised, otherwise untouched) scratch: the walks go out over several workgroups
    const long nwk = mw_walks(N, A);
    PAAC_REQUIRE(walk_scratch_bytes >= paac_walk_scratch_bytes(N, A), "paac_sample_mt_synth_step: walk scratch of %ld bytes, "
                 "%ld needed (paac_walk_scratch_bytes)", (long)walk_scratch_bytes, (long)paac_walk_scratch_bytes(N, A));
    if (nwk <= 16384 && N <= 256 && A <= 32) {
      char* base = static_cast<char*>(walk_scratch);
      mw.counter = reinterpret_cast<unsigned int*>(base);
      mw.exits = reinterpret_cast<unsigned short*>(base + 64);
      mw.rec = reinterpret_cast<unsigned char*>(base + 64 + ((nwk * 2 + 63) / 64) * 64);
      mw.W = (int)((nwk + 255) / 256);
    }
  }
  if (heads && heads->partial && large)             // the sampler workgroups finish the heads themselves
    hs = RowsHeadsHook{heads->partial, heads->ntiles, N, A, heads->ba, heads->bc, const_cast<float*>(probs), heads->values_out};
  const int samplers = mw.W > 0 ? mw.W : 1;
  int nshift = N * PRE_BANDS;                       // large path: one round of the 256 CUs (one workgroup per CU there)
  if (nshift > 256 - samplers) nshift = 256 - samplers > 32 ? 256 - samplers : 32;
  const auto launch = [&](auto kernel, int grid, const void* ahead) {
    launch_k(kernel, dim3(grid), dim3(256), stream, PROF_WHOLE, probs, A, mt_state, actions, st, mw,
             reinterpret_cast<const MtAhead*>(ahead), hs);
  };
  if (large && hs.partial) launch(synth_step_a_mt_kernel<2, true>, samplers + nshift, mt_ahead);
  else if (large) launch(synth_step_a_mt_kernel<2>, samplers + nshift, mt_ahead);
  else launch(synth_step_a_mt_kernel<1>, 1 + N * PRE_BANDS, nullptr);
  }
  if (st.raw) launch_preprocess_after_step(st, stream);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}
}  // namespace paac
