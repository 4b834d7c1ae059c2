// fc data gradient of the small update batches with every operand split ONCE (dX[rows, FLAT] = dH[rows, H] * Wf^T, masked by
// relu'(last conv output)).  Arithmetic = dmm.h's XB = 2 path: each fp32 value split exactly into hi + mid + lo bf16 terms,
// the six partial products down to 2^-16 of the leading one, smallest first, fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
// The generic dmm_kernel splits what it loads in every workgroup: at 160 rows each fc weight is split 5 times (once per row
// tile) and each dH element 49 times (once per column tile), and the launch is VALU-bound on that.  Here
//   * dH arrives pre-split: the kernels that produce dH (heads.h: heads_train_kernel, role 1 of heads_bwd_kernel) also leave
//     its three bf16 planes behind, in the order this kernel's waves load them (store_dh_planes below);
//   * a workgroup owns 16 * CT columns of dX for ALL rows, and is the only one on the GPU that touches that slice of Wf: it
//     splits the slice once, cooperatively, into bf16 planes in LDS (48 KB per 16 columns at H = 512);
//   * its waves divide the 16-row tiles among themselves (tile t -> wave t % NW) and run the "transposed" contraction
//     dX^T[16 features, 16 rows] = Wf[16 features, K] * dH^T[K, 16 rows]: both operands are 4 + 4 consecutive k per lane, and a D
//     tile leaves 4 consecutive features of one row in a lane -- one 16-byte mask load and one 16-byte store, no transpose.
// K loop: one 16-byte buffer load per lane, plane and row tile from the L2-resident planes (PF k-steps ahead, pinned with
// sched_barrier), three ds_read_b128 per column tile (one k-step ahead), MFMAs; no VALU splitting.  The first dH fragments
// are requested in front of the weight loads so that both round trips to memory travel together.
//
// Plane layout (16-byte vectors of 8 bf16): vec(rt, ks, p, lane) = ((rt * H/32 + ks) * 3 + p) * 64 + lane, with rt = row / 16,
// ks = k / 32, p = 0 hi / 1 mid / 2 lo, lane = 16 * kq + (row % 16) holding, as elements 0..3 and 4..7, k = 32 ks + 4 kq .. + 3
// and k = 32 ks + 16 + 4 kq .. + 3 -- the slots dmm.h's split path gives them, so that a 32-deep MFMA step sums the same
// products in the same places on both routes.  A wave's load of one (rt, ks, p) is one contiguous KB.  Rows are zero-padded to
// a multiple of 16 by the workgroup of the last row.
#pragma once
#include "dmm.h"

namespace paac {

constexpr int kFcOnceWaves = 4;          // waves per workgroup of the 16-column form
constexpr int kFcOnceTilesPerWave = 3;   // row tiles per wave: 3 x (PF + 1) x 3 planes x 4 registers of fragments in flight
constexpr int kFcOnceMaxRows = 16 * kFcOnceWaves * kFcOnceTilesPerWave;   // 192: bound of the new route (registers)
// K is summed in this many consecutive parts, each from zero, the parts then added in order -- what the four K waves of the
// generic route's tuned body (net_bwd.hip: OP_FC_DGRAD class 1, WK = 4) and their LDS reduction do.  With the same k in every
// slot of the 32-deep MFMA step (below) the two routes give the same bits there, and a run does not depend on the switch.
constexpr int kFcOnceKParts = 4;

// Called by all 256 threads of the workgroup that produced row i of dH, with the row's H values in row_lds (written by the
// same threads before the call; the call synchronises).  planes == nullptr: nothing.
template <int H>
__device__ __forceinline__ void store_dh_planes(const float* row_lds, const int i, const int B, bf16x8* __restrict__ planes) {
  if constexpr (dh_planes_supported(H)) {
    if (!planes) return;       // (workgroup-uniform)
    __syncthreads();
    constexpr int KS = H / 32;
    const int tid = threadIdx.x;
    for (int k8 = tid; k8 < H / 8; k8 += 256) {
      const int ks = k8 >> 2, kq = k8 & 3;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(row_lds + 32 * ks + 4 * kq);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(row_lds + 32 * ks + 16 + 4 * kq);
      const float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      bf16x8 ph, pm, pl;
      split3_bf16(x, ph, pm, pl);
      bf16x8* dst = planes + ((long)((i >> 4) * KS + ks) * 3) * 64 + kq * 16;
      dst[i & 15] = ph;
      dst[64 + (i & 15)] = pm;
      dst[128 + (i & 15)] = pl;
      if (i == B - 1) {        // the pad rows of the last tile read as zero
        const bf16x8 z = __builtin_bit_cast(bf16x8, (u32x4){0u, 0u, 0u, 0u});
        for (int r = (i & 15) + 1; r < 16; ++r) {
          dst[r] = z;
          dst[64 + r] = z;
          dst[128 + r] = z;
        }
      }
    }
  }
}

struct FcOnceArgs {
  const void* planes;      // dH planes (layout above)
  unsigned planes_bytes;   // extent covering the row tiles of M
  const float* wf;         // [FLAT][H] fc weights as stored
  const float* xf;         // [M][FLAT] last conv output: the ReLU mask
  float* dx;               // [M][FLAT]
  int M, FLAT;
#ifdef PAAC_DMM_STAMPS
  unsigned long long* stamps;   // diagnostic build only: 8 x u64 per wave, the slots of dmm.h (tools/probe_fc.py)
#endif
};

#ifdef PAAC_DMM_STAMPS
#define FCONCE_STAMP(i)                                                                                      \
  do {                                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    if (p.stamps && lane == 0)                                                                               \
      p.stamps[((long)blockIdx.x * NW + wave) * 8 + (i)] =                                                   \
          ((i) == 0 || (i) == 7) ? (unsigned long long)wall_clock64() : (unsigned long long)clock64();       \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
  } while (0)
#else
#define FCONCE_STAMP(i)
#endif

// CT: 16-column tiles per workgroup; NW waves; a wave owns up to TPW row tiles.
template <int H, int CT, int NW, int TPW, int PF>
struct FcOnce {
  static constexpr int KS = H / 32;
  static constexpr int THREADS = 64 * NW;
  static constexpr int ITEMS = CT * KS * 64;               // 8-float groups of the weight slice
  static constexpr int PASSES = ITEMS / THREADS;
  static constexpr int RING = PF + 1;
  static constexpr int GPP = (KS + kFcOnceKParts - 1) / kFcOnceKParts;   // k-steps per K part
  static constexpr int SMEM_BYTES = CT * 3 * KS * 64 * 16;
  static_assert(ITEMS % THREADS == 0, "the weight slice divides over the threads");
  static_assert(PF >= 1 && PF < KS, "prefetch depth");

  // the K loop of a wave that owns NT row tiles (rt0, rt0 + NW, ...)
  template <int NT>
  __device__ __forceinline__ static void tiles(const FcOnceArgs& p, const bf16x8* wl, const __amdgpu_buffer_rsrc_t rs,
                                               const bf16x8 (&pre)[PF][TPW][3], const int rt0, const int n0, const int lane) {
    const int li = lane & 15, q = lane >> 4;
    bf16x8 fb[RING][NT][3];
#pragma unroll
    for (int s = 0; s < PF; ++s)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) fb[s][t][pl] = pre[s][t][pl];
    // mask rows of this wave's outputs: requested now, consumed in the epilogue
    f32x4 mk[NT][CT];
    int off[NT];       // element offset of the lane's float4 in dx / xf, -1 = row out of range
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int row = (rt0 + t * NW) * 16 + li;
      off[t] = (row < p.M) ? row * p.FLAT + n0 + 4 * q : -1;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        mk[t][c] = (off[t] >= 0) ? *reinterpret_cast<const f32x4*>(p.xf + off[t] + 16 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc[NT][CT], tot[NT][CT];      // the running K part, and the sum of the finished parts
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[t][c] = tot[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 wa[2][CT][3];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) wa[0][c][pl] = wl[((c * 3 + pl) * KS + 0) * 64 + lane];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + PF < KS) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            fb[(ks + PF) % RING][t][pl] = __builtin_bit_cast(
                bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)lane * 16u,
                                                              (unsigned)((((rt0 + t * NW) * KS + ks + PF) * 3 + pl) * 1024), 0));
      }
      if (ks + 1 < KS) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) wa[(ks + 1) & 1][c][pl] = wl[((c * 3 + pl) * KS + ks + 1) * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);
      // smallest terms first (dmm.h); the MFMA's A operand is the weight tile, its B operand the dH tile
      constexpr int PW[6] = {0, 1, 2, 0, 1, 0};   // weight plane (0 hi, 1 mid, 2 lo) of product n
      constexpr int PD[6] = {2, 1, 0, 1, 0, 0};   // dH plane
#pragma unroll
      for (int n = 0; n < 6; ++n)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int c = 0; c < CT; ++c)
            acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks & 1][c][PW[n]], fb[ks % RING][t][PD[n]], acc[t][c], 0, 0, 0);
      if ((ks + 1) % GPP == 0 || ks + 1 == KS) {     // a K part ends: part 0 opens the sum, the others join it in order
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            tot[t][c] = (ks < GPP) ? acc[t][c] : tot[t][c] + acc[t][c];
            acc[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
          }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#ifdef PAAC_DMM_STAMPS
    const int wave = rt0;
#endif
    FCONCE_STAMP(4);
    FCONCE_STAMP(5);       // (no LDS reduce: every wave owns whole sums)
    // D: lane (li, q) holds features n0 + 16 c + 4 q .. + 3 of row 16 rt + li
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (off[t] < 0) continue;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        f32x4 v = tot[t][c];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = mk[t][c][e] > 0.f ? v[e] : 0.f;
        *reinterpret_cast<f32x4*>(p.dx + off[t] + 16 * c) = v;
      }
    }
  }

  __device__ __forceinline__ static void run(const FcOnceArgs& p, char* smem) {
    bf16x8* wl = reinterpret_cast<bf16x8*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = blockIdx.x * (16 * CT);
    const int ntiles = (p.M + 15) >> 4;
    const int nt = (wave < ntiles) ? (ntiles - wave + NW - 1) / NW : 0;      // row tiles wave, wave + NW, ... (<= TPW)
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.planes, p.planes_bytes);
    FCONCE_STAMP(0);
    FCONCE_STAMP(1);
    FCONCE_STAMP(2);
    // (1) the first PF k-steps of this wave's dH fragments (a tile the wave does not own: out of range, no access, zeros)
    bf16x8 pre[PF][TPW][3];
#pragma unroll
    for (int s = 0; s < PF; ++s)
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          pre[s][t][pl] = __builtin_bit_cast(
              bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (t < nt) ? (unsigned)lane * 16u : kOob,
                                                            (unsigned)((((wave + t * NW) * KS + s) * 3 + pl) * 1024), 0));
    // (2) the weight slice: item = (column tile, k-step, lane) in LDS order; lane (li, kq) of it holds feature li at
    // k = 32 ks + 4 kq .. + 3 and 32 ks + 16 + 4 kq .. + 3 (the four kq of a feature are 128 contiguous bytes)
    f32x4 w0[PASSES], w1[PASSES];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int id = ps * THREADS + tid;
      const int l = id & 63, ks = (id >> 6) % KS, c = id / (64 * KS);
      const float* src = p.wf + (long)(n0 + 16 * c + (l & 15)) * H + 32 * ks + 4 * (l >> 4);
      w0[ps] = *reinterpret_cast<const f32x4*>(src);
      w1[ps] = *reinterpret_cast<const f32x4*>(src + 16);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int id = ps * THREADS + tid;
      const int l = id & 63, ks = (id >> 6) % KS, c = id / (64 * KS);
      const float x[8] = {w0[ps][0], w0[ps][1], w0[ps][2], w0[ps][3], w1[ps][0], w1[ps][1], w1[ps][2], w1[ps][3]};
      bf16x8 ph, pm, pl;
      split3_bf16(x, ph, pm, pl);
      wl[((c * 3 + 0) * KS + ks) * 64 + l] = ph;
      wl[((c * 3 + 1) * KS + ks) * 64 + l] = pm;
      wl[((c * 3 + 2) * KS + ks) * 64 + l] = pl;
    }
    __syncthreads();
    FCONCE_STAMP(3);       // (2 -> 3: both operands requested, the weight slice split and parked in LDS)
    if (nt == 0) {         // fewer row tiles than waves: nothing to contract
      FCONCE_STAMP(4);
      FCONCE_STAMP(5);
      FCONCE_STAMP(6);
      FCONCE_STAMP(7);
      return;
    }
    static_assert(TPW >= 1 && TPW <= 3, "row tiles per wave");
    if (nt == 1) tiles<1>(p, wl, rs, pre, wave, n0, lane);
    if constexpr (TPW >= 2) { if (nt == 2) tiles<2>(p, wl, rs, pre, wave, n0, lane); }
    if constexpr (TPW >= 3) { if (nt >= 3) tiles<3>(p, wl, rs, pre, wave, n0, lane); }
    FCONCE_STAMP(6);
    FCONCE_STAMP(7);
  }
};

template <class D>
__global__ __launch_bounds__(D::THREADS) void fc_dgrad_once_kernel(const FcOnceArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[D::SMEM_BYTES];
  D::run(p, smem);
}

}  // namespace paac
