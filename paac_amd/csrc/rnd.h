// --explore_kind rnd (spec and float64 numpy twin: paac_amd/rnd.py): Random Network Distillation (Burda et al., arXiv
// 1810.12894) -- a fixed random target net and a predictor trained online to match it, both u[196] -> 256 -> 64 on a 14 x 14
// thumbnail of the newest frame; the predictor's error is the bonus.  Forward of both nets, error, normaliser, bonus, the
// predictor's exact gradient and its Adam step in THREE launches, fp32 matrix instructions (v_mfma_f32_16x16x4_f32: products
// exact in fp32), no floating-point atomics, every sum in a fixed order.  Instantiated in misc.hip alone.
//
// A net is flat: W1 [196, 256] | b1 [256] | W2 [256, 64] | b2 [64].  A bias directly follows its weights, so W1 | b1 IS a
// row-major [197, 256] matrix and W2 | b2 a [257, 64] one: the backward treats the bias as the weight row of a feature that is
// always 1, and the scratch rows of u and h_p carry that 1 behind their last column.
//
// Scratch (fp32 words; Rp = rows rounded up to 16): [0] the ticket, [4..] U [Rp, 208] (u, the 1, zeros up to 13 tiles of 16),
// HT [Rp, 256] (the target's hidden layer), HP [Rp, 272] (the predictor's, the 1, zeros up to 17 tiles), DO [Rp, 64]
// (dL/do_p), DH [Rp, 256] (dL/d pre-activation).  Every call writes every word it later reads -- rows at or beyond `rows`
// as zeros -- so nothing but the ticket is state, and the ticket goes back to 0.
//
// rnd_hidden_kernel -- pooling and layer 1 of both nets.  Grid: (row tile of 16) x (4 slabs of 128 of the 2 x 256 hidden columns):
//   40 workgroups at 160 rows, 672 at 2688.
//   * Pooling: a thread owns a PAIR of cells of one row (12 pixels x 6 lines): per line 48 contiguous bytes = three 16-byte
//     loads, neighbouring threads neighbouring pairs; byte 3 of every dword is the newest plane.  18 loads in flight per thread,
//     7 rounds for 16 rows.  Every slab pools its 16 rows again (4 x the reads, out of L2 after the first) rather than
//     spending a launch on it.  u goes to LDS as fp32 (stride 197) and, from slab 0, to U.
//   * Layer 1: wave w owns two column tiles; 49 k-steps of 4; A = u from LDS, B = 16 consecutive floats of a row of W1 out of L2.
// rnd_error_kernel -- layer 2 of both nets, e, raw, do, dh; the normaliser and the bonus by a ticket.  Grid: one row tile each.
//   * HT and HP of the tile are staged in LDS by 16-byte loads; wave w owns output column tile w of both nets (64 k-steps, 2
//     MFMAs each); e = o_p - o_t in registers; do = e * 2 / (64 rows) to DO and LDS; e * e to LDS, and thread r adds row r's 64
//     squares in column order: raw.
//   * dh = (do W2p^T) * (h_p > 0): wave w owns hidden columns [64 w, 64 w + 64); the B operand W2p[n][k] is read as one 16-byte
//     load of four consecutive k per lane, and the A operand follows the same k order (the instruction pairs A and B by lane
//     group, so any order that both operands share is a valid K order, and it is a fixed one).
//   * explore_last_arrival: the last tile to arrive has every raw in memory.  Its wave 0 takes mean(raw ** 2) in float64 -- lane
//     l adds rows l, l + 64, ... ascending, lane 0 adds the 64 partials in lane order -- updates m and the call count, and all
//     256 threads write bonus and reward.  Nothing depends on which tile is last.
// rnd_step_kernel -- weight gradient and Adam fused by ownership.  Grid: 13 x 16 tiles of [197, 256] + 17 x 4 tiles of [257, 64] =
//   276 workgroups.  A workgroup contracts its 16 x 16 tile over all Rp rows (dW1 = U^T DH, dW2 = HP^T DO): wave w takes the
//   w-th contiguous quarter of the rows in ascending order, the four partials are added as (0 + 1) + (2 + 3) out of LDS, and
//   thread e applies Adam to element e of the tile in place (in float64, rounded once into the fp32 weight and slots).  No
//   gradient buffer, no cross-workgroup sum.  The bias rides as row 196 / 256 of the last row tile.  grad_out (nullable)
//   receives the raw gradient.
#pragma once
#include "common.h"
#include "explore.h"
#include "feature_stats.h"

namespace paac {

constexpr int kRndD = 196, kRndH = 256, kRndO = 64;
constexpr int kRndW1 = 0, kRndB1 = kRndD * kRndH, kRndW2 = kRndB1 + kRndH, kRndB2 = kRndW2 + kRndH * kRndO;
constexpr int kRndNet = kRndB2 + kRndO;              // rnd.NET
constexpr int kRndUS = 208, kRndHS = 272;            // row strides of U and HP: 13 and 17 tiles of 16
constexpr int kRndRowWords = kRndUS + kRndH + kRndHS + kRndO + kRndH;
constexpr int kRndHead = 4;                          // the ticket, and 16-byte alignment of what follows
constexpr int kRndTiles1 = (kRndUS / 16) * (kRndH / 16), kRndTiles2 = (kRndHS / 16) * (kRndO / 16);
constexpr int kRndULds = 197;
static_assert(kRndNet == 66880 && kRndTiles1 == 208 && kRndTiles2 == 68, "rnd.py's layout");

inline int rnd_padded_rows(int rows) { return (rows + 15) / 16 * 16; }
inline int64_t rnd_scratch_words(int rows) { return kRndHead + (int64_t)rnd_padded_rows(rows) * kRndRowWords; }

struct RndArgs {
  const uint8_t* states;
  const float* target;
  float* predictor;
  float* mom;
  float* var;
  double* norm;            // m, the call count
  int32_t* ticket;
  float *U, *HT, *HP, *DO, *DH;
  float* rewards;
  float* bonus_out;
  float* raw_out;
  float* grad_out;         // nullable
  int rows, rows_padded;
  float do_scale;          // 2 / (64 rows)
  double beta, lr, beta1, beta2, eps;
};

__device__ __forceinline__ int rnd_b3(uint32_t w) { return (int)(w >> 24); }

__global__ __launch_bounds__(256) void rnd_hidden_kernel(const RndArgs a) {
  __shared__ float u_s[16 * kRndULds];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = blockIdx.x >> 2, slab = blockIdx.x & 3, row0 = tile * 16;

  // ---- pooling: 16 rows x 98 cell pairs -------------------------------------------------------------------------------------
  for (int task = tid; task < 16 * 98; task += 256) {
    const int rr = task / 98, cp = task - rr * 98, cy = cp / 7, p = cp - cy * 7;
    const bool valid = row0 + rr < a.rows;
    const uint8_t* base = a.states + (size_t)min(row0 + rr, a.rows - 1) * kExpK + (size_t)(6 * cy) * 336 + p * 48;
    uint4 q[6][3];
#pragma unroll
    for (int dy = 0; dy < 6; ++dy)
#pragma unroll
      for (int k = 0; k < 3; ++k) q[dy][k] = *reinterpret_cast<const uint4*>(base + dy * 336 + k * 16);
    int s0 = 0, s1 = 0;
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
      s0 += rnd_b3(q[dy][0].x) + rnd_b3(q[dy][0].y) + rnd_b3(q[dy][0].z) + rnd_b3(q[dy][0].w) + rnd_b3(q[dy][1].x) + rnd_b3(q[dy][1].y);
      s1 += rnd_b3(q[dy][1].z) + rnd_b3(q[dy][1].w) + rnd_b3(q[dy][2].x) + rnd_b3(q[dy][2].y) + rnd_b3(q[dy][2].z) + rnd_b3(q[dy][2].w);
    }
    const float u0 = valid ? (float)s0 / 9180.f : 0.f, u1 = valid ? (float)s1 / 9180.f : 0.f;
    const int d = 14 * cy + 2 * p;
    u_s[rr * kRndULds + d] = u0;
    u_s[rr * kRndULds + d + 1] = u1;
    if (slab == 0) {
      a.U[(size_t)(row0 + rr) * kRndUS + d] = u0;
      a.U[(size_t)(row0 + rr) * kRndUS + d + 1] = u1;
    }
  }
  // the 1 of the bias row and the zeros behind it: U from slab 0, HP from slab 2
  if (slab == 0 && tid < 16 * (kRndUS - kRndD)) {
    const int rr = tid / (kRndUS - kRndD), c = tid - rr * (kRndUS - kRndD);
    a.U[(size_t)(row0 + rr) * kRndUS + kRndD + c] = (c == 0 && row0 + rr < a.rows) ? 1.f : 0.f;
  }
  if (slab == 2) {
    const int rr = tid >> 4, c = tid & 15;
    a.HP[(size_t)(row0 + rr) * kRndHS + kRndH + c] = (c == 0 && row0 + rr < a.rows) ? 1.f : 0.f;
  }
  __syncthreads();

  // ---- layer 1: this wave's 32 hidden columns of its net ---------------------------------------------------------------------
  const bool pred = slab >= 2;
  const float* __restrict__ net = pred ? a.predictor : a.target;
  const int i = lane & 15, g = lane >> 4, col0 = (slab & 1) * 128 + wave * 32;
  const float* __restrict__ w = net + kRndW1 + (size_t)g * kRndH + col0 + i;
  const float* us = u_s + i * kRndULds + g;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 7
  for (int s = 0; s < kRndD / 4; ++s) {
    const float av = us[4 * s];
    const float b0 = w[(size_t)(4 * s) * kRndH], b1 = w[(size_t)(4 * s) * kRndH + 16];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
  }
  // D layout: accumulator v of lane (j = lane % 16, q = lane / 16) is row 4 q + v, column j of the tile
  const float bias0 = net[kRndB1 + col0 + i], bias1 = net[kRndB1 + col0 + 16 + i];
  float* out = pred ? a.HP : a.HT;
  const int stride = pred ? kRndHS : kRndH;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int row = row0 + 4 * g + v;
    const bool valid = row < a.rows;
    out[(size_t)row * stride + col0 + i] = valid ? fmaxf(acc0[v] + bias0, 0.f) : 0.f;
    out[(size_t)row * stride + col0 + 16 + i] = valid ? fmaxf(acc1[v] + bias1, 0.f) : 0.f;
  }
}

__global__ __launch_bounds__(256) void rnd_error_kernel(const RndArgs a, int tiles) {
  constexpr int HL = kRndH + 4, DL = kRndO + 4;
  __shared__ __attribute__((aligned(16))) float h_s[2][16 * HL];
  __shared__ __attribute__((aligned(16))) float do_s[16 * DL];
  __shared__ float sq_s[16 * DL];
  __shared__ double part_s[64];
  __shared__ double denom_s;
  __shared__ int last_s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int row0 = blockIdx.x * 16, i = lane & 15, g = lane >> 4;

  // ---- the tile's two hidden layers into LDS ---------------------------------------------------------------------------------
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int x = k * 256 + tid, net = x >> 10, rr = (x >> 6) & 15, c4 = x & 63;
    const float* src = net ? a.HP + (size_t)(row0 + rr) * kRndHS : a.HT + (size_t)(row0 + rr) * kRndH;
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * c4);
    *reinterpret_cast<f32x4*>(&h_s[net][rr * HL + 4 * c4]) = v;
  }
  __syncthreads();

  // ---- layer 2: output column tile `wave` of both nets, error, do --------------------------------------------------------------
  {
    const float* __restrict__ wt = a.target + kRndW2 + (size_t)g * kRndO + 16 * wave + i;
    const float* __restrict__ wp = a.predictor + kRndW2 + (size_t)g * kRndO + 16 * wave + i;
    const float *ht = &h_s[0][i * HL + g], *hp = &h_s[1][i * HL + g];
    f32x4 acct = {0.f, 0.f, 0.f, 0.f}, accp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int s = 0; s < kRndH / 4; ++s) {
      acct = __builtin_amdgcn_mfma_f32_16x16x4f32(ht[4 * s], wt[(size_t)(4 * s) * kRndO], acct, 0, 0, 0);
      accp = __builtin_amdgcn_mfma_f32_16x16x4f32(hp[4 * s], wp[(size_t)(4 * s) * kRndO], accp, 0, 0, 0);
    }
    const int col = 16 * wave + i;
    const float bt = a.target[kRndB2 + col], bp = a.predictor[kRndB2 + col];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int rr = 4 * g + v;
      const float e = row0 + rr < a.rows ? (accp[v] + bp) - (acct[v] + bt) : 0.f;
      const float d = e * a.do_scale;
      sq_s[rr * DL + col] = e * e;
      do_s[rr * DL + col] = d;
      a.DO[(size_t)(row0 + rr) * kRndO + col] = d;
    }
  }
  __syncthreads();
  if (tid < 16 && row0 + tid < a.rows) {
    float sum = 0.f;
    for (int j = 0; j < kRndO; ++j) sum += sq_s[tid * DL + j];
    a.raw_out[row0 + tid] = sum * (1.f / kRndO);
  }

  // ---- dh = (do W2p^T) * (h_p > 0): hidden columns [64 wave, 64 wave + 64) ------------------------------------------------------
  {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      f32x4 b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        b[t] = *reinterpret_cast<const f32x4*>(a.predictor + kRndW2 + (size_t)(64 * wave + 16 * t + i) * kRndO + 16 * kb + 4 * g);
      const f32x4 av = *reinterpret_cast<const f32x4*>(&do_s[i * DL + 16 * kb + 4 * g]);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], b[t][c], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int rr = 4 * g + v, col = 64 * wave + 16 * t + i;
        a.DH[(size_t)(row0 + rr) * kRndH + col] = h_s[1][rr * HL + col] > 0.f ? acc[t][v] : 0.f;
      }
  }
  if (!explore_last_arrival(a.ticket, tiles, &last_s)) return;

  // ---- every raw of the call is in memory: normaliser, bonus, reward add -------------------------------------------------------
  if (wave == 0) {
    double sum = 0.0;
    for (int r = lane; r < a.rows; r += 64) {
      const double x = (double)__hip_atomic_load(&a.raw_out[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sum += x * x;
    }
    part_s[lane] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total += part_s[l];
    const double mean = total / (double)a.rows, calls = a.norm[1];
    const double m = calls == 0.0 ? mean : 0.99 * a.norm[0] + 0.01 * mean;
    a.norm[0] = m;
    a.norm[1] = calls + 1.0;
    denom_s = sqrt(m) + 1e-8;
  }
  __syncthreads();
  const double denom = denom_s;
  for (int r = tid; r < a.rows; r += 256) {
    const double x = (double)__hip_atomic_load(&a.raw_out[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float bonus = (float)(a.beta * x / denom);
    a.bonus_out[r] = bonus;
    a.rewards[r] += bonus;
  }
}

__global__ __launch_bounds__(256) void rnd_step_kernel(const RndArgs a) {
  __shared__ float red[4][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const bool second = blockIdx.x >= kRndTiles1;
  const int b = second ? blockIdx.x - kRndTiles1 : blockIdx.x;
  const int width = second ? kRndO : kRndH, m_rows = second ? kRndH + 1 : kRndD + 1, flat0 = second ? kRndW2 : kRndW1;
  const int rt = b / (width / 16), ct = b - rt * (width / 16);
  const int sa = second ? kRndHS : kRndUS, sb = width;
  const float* __restrict__ A = (second ? a.HP : a.U) + 16 * rt + i;
  const float* __restrict__ B = (second ? a.DO : a.DH) + 16 * ct + i;

  // ---- this wave's quarter of the rows, ascending ------------------------------------------------------------------------------
  const int steps = a.rows_padded / 4, per = (steps + 3) / 4;
  const int s_end = min((wave + 1) * per, steps);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int s = wave * per;
  for (; s + 4 <= s_end; s += 4) {          // four k-steps of loads requested before the first MFMA
    float av[4], bv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t r = (size_t)(4 * (s + k) + g);
      av[k] = A[r * sa];
      bv[k] = B[r * sb];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], bv[k], acc, 0, 0, 0);
  }
  for (; s < s_end; ++s) {
    const size_t r = (size_t)(4 * s + g);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[r * sa], B[r * sb], acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) red[wave][v * 64 + lane] = acc[v];
  __syncthreads();

  // ---- element tid of the tile: gradient, Adam in place ------------------------------------------------------------------------
  const int v = tid >> 6, ln = tid & 63, row = 16 * rt + 4 * (ln >> 4) + v, col = 16 * ct + (ln & 15);
  if (row >= m_rows) return;
  const float grad = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  const int at = flat0 + row * width + col;
  if (a.grad_out) a.grad_out[at] = grad;
  const double t = a.norm[1];          // (the call count, this call included: rnd_error_kernel has advanced it)
  const double gd = (double)grad;
  const float mom = (float)(a.beta1 * (double)a.mom[at] + (1.0 - a.beta1) * gd);
  const float var = (float)(a.beta2 * (double)a.var[at] + (1.0 - a.beta2) * gd * gd);
  const double mhat = (double)mom / (1.0 - pow(a.beta1, t)), vhat = (double)var / (1.0 - pow(a.beta2, t));
  a.mom[at] = mom;
  a.var[at] = var;
  a.predictor[at] = (float)((double)a.predictor[at] - a.lr * mhat / (sqrt(vhat) + a.eps));
}

}  // namespace paac
