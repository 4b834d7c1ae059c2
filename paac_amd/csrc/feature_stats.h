// --feature_stats (spec and numpy twin: paac_amd/feature_stats.py): the fold of one cycle's training activations into the
// window's block, and the finish of a window.  Instantiated in misc.hip alone.
//
// feature_gram_kernel -- G += H^T H over the fc activations h fp32 [R, H] (H a multiple of 64 up to 1024, any R >= 1)
//   * Both operands of the product are the same matrix, read in place: with v_mfma_f32_32x32x2_f32 the A operand (M = unit i,
//     K = row) of lane l is h[r + l / 32][i0 + l % 32] and the B operand (K = row, N = unit j) is h[r + l / 32][j0 + l % 32] --
//     32 consecutive floats per row either way, so a fragment is one coalesced 128-byte load per row and there is no
//     transpose, no LDS and no packing pass.  fp32 matrix instructions, not the three-plane bf16 split: the split pays when
//     an operand is split once and read many times; here the operand is this cycle's activations, a split would cost a pass
//     of its own over the very bytes the kernel reads, and at these sizes the kernel is latency, not MFMA rate.
//   * Work split: a workgroup of four waves owns one 64 x 64 tile of the UPPER triangle of G (grid x) and one group of row
//     chunks (grid y); wave w owns the 32 x 32 quarter (w / 2, w % 2).  On a diagonal tile the quarter (1, 0) is the mirror of
//     (0, 1): its wave leaves at once, and the diagonal quarters pass the same register as A and B -- one column panel read,
//     not two.  A wave requests 8 K steps (16 rows) of both panels before its first MFMA of the batch.
//   * Rows: chunks of kFeatChunkRows; inside a chunk the 16 accumulators are the MFMA's fp32; behind each chunk they are added
//     to 16 fp64 registers and cleared.  A workgroup walks the consecutive chunks of its group in ascending order and leaves its
//     fp64 quarter in the block's scratch, in accumulator order (lane-contiguous stores).  Rows at or beyond R are never
//     read: their lanes carry 0.
//   * feature_reduce_kernel, the launch behind it, adds the groups' quarters in ascending group order in fp64 and adds
//     element (i, j), i <= j, to G[i][j] and to G[j][i].  No atomics, no ticket: the order is the launch order.
// unit_stats_kernel -- per-unit sum and count of positives of every layer, one launch (grid y = layer slot)
//   * activations [samples, C] with C a multiple of 16: thread (q, p) of a workgroup owns the four channels of quad q and
//     every tpq-th sample of the workgroup's contiguous sample range, 16-byte loads, fp64 sums and int32 counts in registers;
//     the workgroup's threads of one quad are then added in thread order out of LDS and the result goes to the scratch;
//     feature_reduce_kernel adds the workgroups in ascending order into the block.
// feature_finish_kernel -- once per window: trace and squared Frobenius norm of G, dormant / dead / positive counts per layer.
#pragma once
#include "common.h"

namespace paac {

constexpr int kFeatChunkRows = PAAC_FEATURE_CHUNK_ROWS;      // feature_stats.CHUNK_ROWS
constexpr int kFeatSplitsMax = 8;        // feature_stats.GRAM_SPLITS_MAX
constexpr int kFeatUnitWgs = 256;        // feature_stats.UNIT_WGS
constexpr int kFeatScalars = PAAC_FEATURE_SCALARS;         // feature_stats.FINISH_SCALARS
constexpr int kFeatBatchSteps = 8;       // K steps of two rows requested together

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The block's offsets for the unit counts of the four layer slots (feature_stats.Layout).
struct FeatLayout {
  int units[4], unit_off[4];
  int H, U, n32, tiles;
  int64_t f_sum, f_gram, f_part_gram, f_part_sum, n_f;
  int64_t i_cycles, i_rows, i_samples, i_pos, i_part_pos, n_i;
};
inline FeatLayout feat_layout(const int units[4]) {
  FeatLayout L{};
  int at = 0;
  for (int l = 0; l < 4; ++l) {
    L.units[l] = units[l];
    L.unit_off[l] = at;
    at += units[l];
  }
  L.U = at;
  L.H = units[3];
  L.n32 = L.H / 32;
  L.tiles = L.n32 * (L.n32 + 1) / 2;
  L.f_sum = 0;
  L.f_gram = L.U;
  L.f_part_gram = L.f_gram + (int64_t)L.H * L.H;
  L.f_part_sum = L.f_part_gram + (int64_t)kFeatSplitsMax * L.tiles * 1024;
  L.n_f = L.f_part_sum + (int64_t)kFeatUnitWgs * L.U;
  L.i_cycles = 0;
  L.i_rows = 1;
  L.i_samples = 2;
  L.i_pos = 6;
  L.i_part_pos = L.i_pos + L.U;
  L.n_i = L.i_part_pos + (int64_t)kFeatUnitWgs * L.U;
  return L;
}

// index of the 32 x 32 tile (bi, bj), bi <= bj, among the upper triangle's tiles in row-major order
__host__ __device__ inline int feat_tile_index(int bi, int bj, int n32) { return bi * n32 - bi * (bi - 1) / 2 + (bj - bi); }

struct FeatFold {
  const float* act[4];       // conv outputs [rows, positions, units] / fc activations [rows, H]; nullptr: no such layer
  int positions[4];
  int wgs[4];                // workgroups of unit_stats_kernel that work on the layer
  int rows;
  int chunks_per_group, groups;
  FeatLayout L;
};

__global__ __launch_bounds__(256) void feature_gram_kernel(const FeatFold f, double* __restrict__ acc_f) {
  const int H = f.L.H, R = f.rows, n64 = H / 64;
  // the 64 x 64 tile of the upper triangle: row-major over (ti <= tj)
  int ti = 0, left = blockIdx.x;
  while (left >= n64 - ti) {
    left -= n64 - ti;
    ++ti;
  }
  const int tj = ti + left;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bi = 2 * ti + (wave >> 1), bj = 2 * tj + (wave & 1);
  if (bi > bj) return;                                   // the mirror quarter of a diagonal tile
  const bool diag = bi == bj;
  const float* __restrict__ h = f.act[3];
  const int ca = bi * 32 + (lane & 31), cb = bj * 32 + (lane & 31), half = lane >> 5;
  double sum[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) sum[v] = 0.0;
  const int c_first = blockIdx.y * f.chunks_per_group;
  for (int c = c_first; c < c_first + f.chunks_per_group; ++c) {
    const int r_begin = c * kFeatChunkRows;
    if (r_begin >= R) break;
    const int r_end = min(r_begin + kFeatChunkRows, R);
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int r0 = r_begin; r0 < r_end; r0 += 2 * kFeatBatchSteps) {
      float fa[kFeatBatchSteps], fb[kFeatBatchSteps];
#pragma unroll
      for (int s = 0; s < kFeatBatchSteps; ++s) {
        const int r = r0 + 2 * s + half;
        const bool ok = r < r_end;
        const size_t row = (size_t)(ok ? r : r_begin) * H;       // (a masked lane reads a row that exists, and drops it)
        const float va = h[row + ca];
        fa[s] = ok ? va : 0.f;
        if (!diag) {
          const float vb = h[row + cb];
          fb[s] = ok ? vb : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < kFeatBatchSteps; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], diag ? fa[s] : fb[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) sum[v] += (double)acc[v];
  }
  double* part = acc_f + f.L.f_part_gram + ((size_t)blockIdx.y * f.L.tiles + feat_tile_index(bi, bj, f.L.n32)) * 1024;
#pragma unroll
  for (int v = 0; v < 16; ++v) part[v * 64 + lane] = sum[v];
}

__global__ __launch_bounds__(256) void unit_stats_kernel(const FeatFold f, double* __restrict__ acc_f, int64_t* __restrict__ acc_i) {
  const int l = blockIdx.y, b = blockIdx.x;
  if (!f.act[l] || b >= f.wgs[l]) return;
  const int C = f.L.units[l], cq = C / 4, tpq = 256 / cq;
  const int64_t samples = (int64_t)f.rows * f.positions[l];
  const int64_t per = (samples + f.wgs[l] - 1) / f.wgs[l];
  const int64_t s0 = b * per, s1 = min(s0 + per, samples);
  const int t = threadIdx.x, q = t % cq, p = t / cq;
  __shared__ double lds_s[256 * 4];
  __shared__ int lds_p[256 * 4];
  double sum[4] = {0.0, 0.0, 0.0, 0.0};
  int pos[4] = {0, 0, 0, 0};
  if (p < tpq) {
    const f32x4* __restrict__ a = reinterpret_cast<const f32x4*>(f.act[l]);
#pragma unroll 4
    for (int64_t s = s0 + p; s < s1; s += tpq) {
      const f32x4 v = a[s * cq + q];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sum[e] += (double)v[e];
        pos[e] += v[e] > 0.f ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lds_s[t * 4 + e] = sum[e];
    lds_p[t * 4 + e] = pos[e];
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    double s = 0.0;
    int64_t n = 0;
    for (int k = 0; k < tpq; ++k) {
      s += lds_s[(k * cq + c / 4) * 4 + (c & 3)];
      n += lds_p[(k * cq + c / 4) * 4 + (c & 3)];
    }
    const size_t at = (size_t)b * f.L.U + f.L.unit_off[l] + c;
    acc_f[f.L.f_part_sum + at] = s;
    acc_i[f.L.i_part_pos + at] = n;
  }
}

// One thread per element of the upper triangle's tiles, then one per unit, then one for the counters.
__global__ __launch_bounds__(256) void feature_reduce_kernel(const FeatFold f, double* __restrict__ acc_f, int64_t* __restrict__ acc_i) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_gram = (int64_t)f.L.tiles * 1024;
  if (id < n_gram) {
    const int tile = (int)(id >> 10), rem = (int)(id & 1023), v = rem >> 6, lane = rem & 63;
    int bi = 0, left = tile;
    while (left >= f.L.n32 - bi) {
      left -= f.L.n32 - bi;
      ++bi;
    }
    const int bj = bi + left;
    // accumulator v of lane `lane` (v_mfma_f32_32x32x2_f32): row 8 * (v / 4) + 4 * (lane / 32) + v % 4, column lane % 32
    const int m = 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3), n = lane & 31;
    if (bi == bj && m > n) return;
    const double* part = acc_f + f.L.f_part_gram + id;
    double s = 0.0;
    for (int g = 0; g < f.groups; ++g) s += part[(size_t)g * n_gram];
    const int gi = bi * 32 + m, gj = bj * 32 + n;
    double* G = acc_f + f.L.f_gram;
    G[(size_t)gi * f.L.H + gj] += s;
    if (gi != gj) G[(size_t)gj * f.L.H + gi] += s;
    return;
  }
  const int64_t u = id - n_gram;
  if (u < f.L.U) {
    int l = 3;
    while (u < f.L.unit_off[l]) --l;
    if (!f.act[l]) return;
    double s = 0.0;
    int64_t n = 0;
    for (int b = 0; b < f.wgs[l]; ++b) {
      s += acc_f[f.L.f_part_sum + (size_t)b * f.L.U + u];
      n += acc_i[f.L.i_part_pos + (size_t)b * f.L.U + u];
    }
    acc_f[f.L.f_sum + u] += s;
    acc_i[f.L.i_pos + u] += n;
  } else if (u == f.L.U) {
    acc_i[f.L.i_cycles] += 1;
    acc_i[f.L.i_rows] += f.rows;
    for (int l = 0; l < 4; ++l)
      if (f.act[l]) acc_i[f.L.i_samples + l] += (int64_t)f.rows * f.positions[l];
  }
}

// window_stats' order for one sum: thread i adds terms i, i + 256, ..., then the 256 partials are added in index order.
__device__ __forceinline__ double feat_ordered_sum(double mine, double* lds) {
  __syncthreads();
  lds[threadIdx.x] = mine;
  __syncthreads();
  double total = 0.0;
  for (int i = 0; i < 256; ++i) total = total + lds[i];
  return total;
}

__global__ __launch_bounds__(256) void feature_finish_kernel(const FeatLayout L, const double* __restrict__ acc_f,
                                                             const int64_t* __restrict__ acc_i, double tau,
                                                             double* __restrict__ out) {
  // (plain operators under contract(off): the twin rounds every square before it adds it; the rounding intrinsics' inlined
  // bodies would keep the contraction setting of where they are defined)
#pragma clang fp contract(off)
  __shared__ double lds[256];
  const int t = threadIdx.x;
  const double* G = acc_f + L.f_gram;
  double tr = 0.0, fro = 0.0;
  for (int i = t; i < L.H; i += 256) tr = tr + G[(size_t)i * L.H + i];
  const int64_t n = (int64_t)L.H * L.H;
  for (int64_t i = t; i < n; i += 256) fro = fro + G[i] * G[i];
  tr = feat_ordered_sum(tr, lds);
  fro = feat_ordered_sum(fro, lds);
  if (t == 0) {
    out[0] = tr;
    out[1] = fro;
    out[14] = (double)acc_i[L.i_rows];
    out[15] = (double)acc_i[L.i_cycles];
    for (int l = 0; l < 4; ++l) out[16 + l] = (double)acc_i[L.i_samples + l];
  }
  // one thread per layer slot: the layer's total in index order, then the counts
  if (t < 4) {
    const int units = L.units[t];
    const double* sum = acc_f + L.f_sum + L.unit_off[t];
    const int64_t* pos = acc_i + L.i_pos + L.unit_off[t];
    double total = 0.0;
    for (int u = 0; u < units; ++u) total = total + sum[u];
    const double bar = tau * total;
    int64_t dormant = 0, dead = 0, positive = 0;
    for (int u = 0; u < units; ++u) {
      dormant += sum[u] * (double)units <= bar ? 1 : 0;
      dead += pos[u] == 0 ? 1 : 0;
      positive += pos[u];
    }
    out[2 + 3 * t] = (double)dormant;
    out[3 + 3 * t] = (double)dead;
    out[4 + 3 * t] = (double)positive;
  }
}

}  // namespace paac
