// Input gradients (paac_input_grad): the data gradient of conv1 -- the one layer gradient training never needs -- and the
// seed kernel in front of the data-gradient chain.
//
//   dX[b, iy, ix, c] = sum over (oy, ox, co) with iy = oy S + ky, ix = ox S + kx of dY1[b, oy, ox, co] * W1[ky, kx, c, co]
//
// X = u8 * (1/255) is the scaled input (networks.py:115), dX float32 [B, 84, 84, 4]; dY1 is already masked by relu'(a1), the
// input side has no mask; a pixel no window covers gets 0.
//
// conv1_dgrad_cell_kernel: a CELL GEMM with no overlap-add, for S = 4 and K1 = 4 R.  The input is tiled into cells of 4 x 4
// pixels x 4 channels (21 x 21 of them); every output of cell (cy, cx) is
//   dX[4 cy + py, 4 cx + px, c] = sum_{dy, dx < R} sum_co dY1[cy - dy, cx - dx, co] * W1[py + 4 dy, px + 4 dx, c, co]
// (zeros outside [0, O1)), i.e. C[M = B * 441, N = 64] = A[M, K = R R C1] * Bw[K, N]:
//   * A is the R x R window gather of dY1, contiguous along co: one 16-byte load per lane and 16-wide K group, never
//     materialised.  K is permuted inside each group, identically for both operands, like dmm.h: lane (row, kq) holds
//     k = 16 g + 4 kq + e for the four MFMAs e of the group.
//   * Bw is W1 re-indexed, n = (py, px, c): staged by the workgroup into LDS in fragment order ([group][py][lane] float4:
//     conflict-free 16-byte reads), 8 groups (32 KB) at a time -- the stock layers (K = 128 / 64) stage it once.
//   * M is flat over (sample, cell): a ragged last tile spans samples.  A wave owns one 16-cell tile per pass, a workgroup
//     (4 waves) takes `run` passes of 64 consecutive cells.
//   * v_mfma_f32_16x16x4_f32: exact fp32 products.  Accumulator tile j IS pixel row py = j of the cells; a 4 x 4 transpose
//     inside each lane quad turns (4 cells x 1 channel) into (1 cell x 4 channels): every lane stores 16 bytes, a quad row of
//     lanes the 64-byte pixel-row segment of a cell.  Every dX element is written exactly once, by one lane.
// conv1_dgrad_direct_kernel: any other first layer (K1 % S1 != 0, S1 != 4) -- one thread per pixel, plain fp32 FMAs in a
// fixed order, like conv_dgrad_direct_kernel (net_bwd.hip) but unmasked; also the yardstick the cell kernel is timed against.
// Both share the epilogue: dX, and / or the fused FGSM step x' = clamp(x - E sgn(dX), 0, 255) on the u8 frame.
#pragma once
#include "dmm.h"

namespace paac {

// These kernels are compiled without packed fp32 arithmetic, as a per-function target feature.  A function of another feature
// set is not inlined into them, so they call none that is not always-inline: the barrier and the quad exchange are spelled
// with builtins here, the helpers below carry the same attribute.
#if defined(__HIP_DEVICE_COMPILE__)
#define PAAC_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PAAC_NO_PK_F32
#endif
__device__ __forceinline__ PAAC_NO_PK_F32 void ig_barrier() {      // __syncthreads()
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the value of lane (lane ^ R) of the same quad, R = 1..3 (DPP quad_perm)
template <int R>
__device__ __forceinline__ PAAC_NO_PK_F32 float ig_quad_xor(const float v) {
  constexpr int ctrl = (0 ^ R) | ((1 ^ R) << 2) | ((2 ^ R) << 4) | ((3 ^ R) << 6);
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true));
}

constexpr int IG_OUT_DX = 1, IG_OUT_FGSM = 2;      // epilogue flags (template argument OUT: 1, 2 or 3)
struct InputGradOut {
  float* dx;               // [B, 84, 84, 4]            (IG_OUT_DX)
  const uint8_t* x;        // the u8 frames             (IG_OUT_FGSM)
  uint8_t* x_adv;          // the perturbed frames
  int levels;              // E, pixel levels
};

// One pixel's four channels.  sgn(0) = sgn(NaN) = 0: both comparisons are false.
template <int OUT>
__device__ __forceinline__ PAAC_NO_PK_F32 void input_grad_store(const InputGradOut& o, size_t pixel, const f32x4 g) {
  if constexpr ((OUT & IG_OUT_DX) != 0) *reinterpret_cast<f32x4*>(o.dx + pixel * 4) = g;
  if constexpr ((OUT & IG_OUT_FGSM) != 0) {
    const unsigned x = *reinterpret_cast<const unsigned*>(o.x + pixel * 4);      // four channels, one byte each
    unsigned r = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int v = (int)((x >> (8 * c)) & 255u) - o.levels * ((g[c] > 0.f ? 1 : 0) - (g[c] < 0.f ? 1 : 0));
      r |= (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * c);
    }
    *reinterpret_cast<unsigned*>(o.x_adv + pixel * 4) = r;
  }
}

constexpr int kIgWaves = 4;            // waves of a cell workgroup: one 16-cell tile each per pass
constexpr int kIgChunkGroups = 8;      // 16-wide K groups of Bw resident in LDS at a time (32 KB)

template <class G, int C1>
constexpr bool conv1_dgrad_cell_ok() {
  return G::S == 4 && G::KH == G::KW && G::KH % 4 == 0 && G::KH >= 4 && G::KH <= 16 && G::C == 4 && C1 % 16 == 0 && G::IH == G::IW;
}

template <int K1, int C1, int NG, int GC>
__device__ __forceinline__ PAAC_NO_PK_F32 void ig_stage_bw(f32x4* bw, const float* __restrict__ W1, const int ch, const int tid) {
  constexpr int R = K1 / 4;
  const int ng = (NG - ch * GC) < GC ? (NG - ch * GC) : GC;
  for (int i = tid; i < ng * 256; i += 64 * kIgWaves) {
    const int l = i & 63, py = (i >> 6) & 3, g = ch * GC + (i >> 8);
    const int k0 = 16 * g + 4 * (l >> 4), tap = k0 / C1, co0 = k0 - tap * C1;
    const int dy = tap / R, dx = tap - dy * R, px = (l & 15) >> 2, c = l & 3;
    bw[i] = *reinterpret_cast<const f32x4*>(W1 + ((size_t)((py + 4 * dy) * K1 + px + 4 * dx) * 4 + c) * C1 + co0);
  }
}

template <class G, int C1, int OUT>
__global__ __launch_bounds__(64 * kIgWaves) PAAC_NO_PK_F32 void conv1_dgrad_cell_kernel(const float* __restrict__ dY,
                                                                                        const float* __restrict__ W1,
                                                                                        const InputGradOut o, const int batch,
                                                                                        const int run) {
  static_assert(conv1_dgrad_cell_ok<G, C1>(), "the cell form: stride 4, kernel size 4 R, 4 input channels");
  constexpr int K1 = G::KH, R = K1 / 4, O1 = G::OH;
  constexpr int NC = (G::IH + 3) / 4, NCELL = NC * NC;       // cells per side / per sample
  constexpr int NG = R * R * C1 / 16;                        // K groups
  constexpr int GC = NG < kIgChunkGroups ? NG : kIgChunkGroups, NCH = (NG + GC - 1) / GC;
  __shared__ f32x4 bw[GC * 4 * 64];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long M = (long)batch * NCELL;

  // Bw[k, n = 16 py + 4 px + c] = W1[py + 4 dy, px + 4 dx, c, co], k = (dy R + dx) C1 + co: a chunk in fragment order
  // (ig_stage_bw, below the kernel's constants)
  if constexpr (NCH == 1) {
    ig_stage_bw<K1, C1, NG, GC>(bw, W1, 0, tid);
    ig_barrier();
  }

  for (int pass = 0; pass < run; ++pass) {
    const long tile = ((long)blockIdx.x * run + pass) * kIgWaves + wave;
    // the lane's A row: cell m of the flat (sample, cell) order
    const long m = tile * 16 + li;
    const bool row_ok = m < M;
    const int b = row_ok ? (int)(m / NCELL) : 0;
    const int cell = row_ok ? (int)(m - (long)b * NCELL) : 0;
    const int cy = cell / NC, cx = cell - cy * NC;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
      if constexpr (NCH > 1) {        // (uniform: every wave runs every pass, rows past M are predicated)
        ig_barrier();
        ig_stage_bw<K1, C1, NG, GC>(bw, W1, ch, tid);
        ig_barrier();
      }
      f32x4 fa[GC];
#pragma unroll
      for (int gl = 0; gl < GC; ++gl) {
        const int g = ch * GC + gl, tap = (16 * g) / C1, dy = tap / R, dx = tap - dy * R;
        const int oy = cy - dy, ox = cx - dx;
        const bool ok = row_ok && g < NG && oy >= 0 && oy < O1 && ox >= 0 && ox < O1;
        fa[gl] = ok ? *reinterpret_cast<const f32x4*>(dY + ((size_t)(b * O1 + oy) * O1 + ox) * C1 + (16 * g - tap * C1) + 4 * kq)
                    : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int gl = 0; gl < GC; ++gl) {
        if (ch * GC + gl < NG) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const f32x4 fb = bw[(gl * 4 + j) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[gl][e], fb[e], acc[j], 0, 0, 0);
          }
        }
      }
    }
    // acc[py][e] = (cell 4 kq + e, pixel row py, pixel px = li / 4, channel li % 4).  Round r of the quad transpose: lane q
    // hands its cell q ^ r to lane q ^ r and receives channel q ^ r of its own cell q.
    const int q = li & 3, px = li >> 2;
    const long m2 = tile * 16 + 4 * kq + q;
    const bool out_ok = m2 < M;
    const int b2 = out_ok ? (int)(m2 / NCELL) : 0;
    const int cell2 = out_ok ? (int)(m2 - (long)b2 * NCELL) : 0;
    const int cy2 = cell2 / NC, cx2 = cell2 - cy2 * NC;
    const int ix = 4 * cx2 + px;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = q ^ r;
        const float send = s == 0 ? acc[j][0] : s == 1 ? acc[j][1] : s == 2 ? acc[j][2] : acc[j][3];
        const float got = r == 0 ? send : r == 1 ? ig_quad_xor<1>(send) : r == 2 ? ig_quad_xor<2>(send) : ig_quad_xor<3>(send);
        v[0] = s == 0 ? got : v[0];
        v[1] = s == 1 ? got : v[1];
        v[2] = s == 2 ? got : v[2];
        v[3] = s == 3 ? got : v[3];
      }
      const int iy = 4 * cy2 + j;
      if (out_ok && iy < G::IH && ix < G::IW)      // (cells beyond the last pixel are clipped)
        input_grad_store<OUT>(o, ((size_t)b2 * G::IH + iy) * G::IW + ix, v);
    }
  }
}

template <class G, int COUT, int OUT>
__global__ __launch_bounds__(256) PAAC_NO_PK_F32 void conv1_dgrad_direct_kernel(const float* __restrict__ dY,
                                                                                 const float* __restrict__ Wt,
                                                                                 const InputGradOut o, const int batch) {
  static_assert(G::C == 4 && COUT % 4 == 0, "four input channels per pixel; output channels are read four at a time");
  const long pixel = (long)blockIdx.x * 256 + threadIdx.x;
  if (pixel >= (long)batch * G::IH * G::IW) return;
  const int ix = (int)(pixel % G::IW);
  const int iy = (int)((pixel / G::IW) % G::IH);
  const int b = (int)(pixel / ((long)G::IW * G::IH));
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ky = iy % G::S; ky < G::KH && ky <= iy; ky += G::S) {
    const int oy = (iy - ky) / G::S;
    if (oy >= G::OH) continue;
    for (int kx = ix % G::S; kx < G::KW && kx <= ix; kx += G::S) {
      const int ox = (ix - kx) / G::S;
      if (ox >= G::OW) continue;
      const f32x4* dy = reinterpret_cast<const f32x4*>(dY + ((size_t)(b * G::OH + oy) * G::OW + ox) * COUT);
      const f32x4* w = reinterpret_cast<const f32x4*>(Wt + (size_t)(ky * G::KW + kx) * 4 * COUT);
#pragma unroll 2
      for (int qd = 0; qd < COUT / 4; ++qd) {
        const f32x4 a = dy[qd];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 v = w[c * (COUT / 4) + qd];
          acc[c] = fmaf(a[0], v[0], acc[c]);
          acc[c] = fmaf(a[1], v[1], acc[c]);
          acc[c] = fmaf(a[2], v[2], acc[c]);
          acc[c] = fmaf(a[3], v[3], acc[c]);
        }
      }
    }
  }
  input_grad_store<OUT>(o, (size_t)pixel, (f32x4){acc[0], acc[1], acc[2], acc[3]});
}

// Seeds of the chain, one workgroup per row: dH[b, j] = relu'(h[b, j]) * (sum_a sl[b, a] Wa[j, a] + sv[b] wc[j]).
//   PAAC_IG_SEEDS        sl / sv given (either nullable = 0)
//   PAAC_IG_VALUE        sv = 1, sl = 0
//   PAAC_IG_LOGP_ACTION  sl = onehot(actions[b]) - probs[b], sv = 0: the gradient of log pi(a | s) wrt the logits
//   PAAC_IG_LOGP_ARGMAX  the same with a = argmax probs[b], the lowest index on ties -- no host value involved
struct InputGradSeeds {
  int mode;
  const float* sl;             // [B, A]
  const float* sv;             // [B]
  const int32_t* actions;      // [B]
};
__global__ __launch_bounds__(256) PAAC_NO_PK_F32 void input_grad_seed_kernel(const float* __restrict__ h,
                                                                              const float* __restrict__ probs,
                                                                              const float* __restrict__ Wa,
                                                                              const float* __restrict__ Wc,
                                                                              const InputGradSeeds sd, const int A, const int H,
                                                                              float* __restrict__ dH) {
  __shared__ float sl[32];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) {
    float v = 0.f;
    if (tid < A) {
      const float* p = probs + (size_t)i * A;
      if (sd.mode == PAAC_IG_SEEDS) {
        v = sd.sl ? sd.sl[(size_t)i * A + tid] : 0.f;
      } else if (sd.mode == PAAC_IG_LOGP_ACTION || sd.mode == PAAC_IG_LOGP_ARGMAX) {
        int a = 0;
        if (sd.mode == PAAC_IG_LOGP_ACTION) {
          a = sd.actions[i];
        } else {
          float best = p[0];
          for (int k = 1; k < A; ++k) {
            const float pk = p[k];
            if (pk > best) {
              best = pk;
              a = k;
            }
          }
        }
        v = (tid == a ? 1.f : 0.f) - p[tid];
      }
    }
    sl[tid] = v;
  }
  const float sv = sd.mode == PAAC_IG_VALUE ? 1.f : (sd.mode == PAAC_IG_SEEDS && sd.sv) ? sd.sv[i] : 0.f;
  ig_barrier();
  for (int j = tid; j < H; j += 256) {
    float acc = sv * Wc[j];
    for (int a = 0; a < A; ++a) acc = fmaf(sl[a], Wa[(size_t)j * A + a], acc);
    dH[(size_t)i * H + j] = h[(size_t)i * H + j] > 0.f ? acc : 0.f;
  }
}

}  // namespace paac
