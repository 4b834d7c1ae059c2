// The optimizer step on gfx950: gradient clip (ignore / global norm / per-tensor norm), TF RMSProp / Adam over the flat
// parameter buffer with the packed weight copies kept current, the --ppo_target_kl gate, gradient statistics.
#include <type_traits>

#include "common.h"
#include "tower.h"

namespace paac {

__global__ void fill_f32_kernel(float* p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// =============================================================================================
// Gradient clip (ignore / global norm / per-tensor norm) + TF RMSProp over the flat parameter buffer
// (actor_learner.py:31-34,51-64,70).
constexpr int NORM_BLOCKS = 256;         // tail blocks of norm_kernel
constexpr int kNormPartialsMax = 1024;   // head blocks + tail blocks; unused slots stay 0 (the optimizer step sums all of them)
constexpr int NORM_LANES = 8;            // lanes that share one float4 of the head (the slab sums of net_bwd.hip's finalize)

// The flat gradient is [conv tensors | fc_w fc_b actor critic] (TF variable order).  The norm pass walks it as
//   head blocks: the conv tensors, 32 float4 per block, NORM_LANES adjacent lanes per float4.  After a backward that left
//                its slab reduction pending (paac_loss_backward phase 3) the lanes sum the split-K slabs -- lane r takes
//                slabs r, r + 8, ... (up to 8 loads in flight), then a fixed xor tree -- and lane 0 WRITES the gradient
//                value before using it; otherwise lane 0 reads the value grad_finalize_kernel wrote with the same
//                arithmetic.  Either way the same bits enter the same partial: the norm does not depend on the route.
//   tail blocks: NORM_BLOCKS blocks stride over the rest (fc / heads gradients, written by their kernels).
// partials layout (kNormPartialsMax floats each): [0] sum of squares (what the clip needs), then what the reference's
// gradient summaries need (logger_utils.py:23-33 over the flat gradient, actor_learner.py:85-87): [1] sum, [2] max and
// [3] min over the NONZERO elements, [4] number of exact zeros.  The flat buffer's alignment pads (all in the tail) are
// zeros the reference's flat gradient does not contain; the reader (grad_stats_kernel) knows how many pads there are, so
// zeros count for max / min only when more zeros were seen than there are pads.
struct NormSeg {
  const float* src;   // first slab (pending reduction) or nullptr
  long dst4;          // float4 offset of the tensor inside the flat gradient
  int count4;         // float4s
  int splits;
  long stride;        // floats between slabs
};
struct NormArgs {
  NormSeg seg[6];
  int nseg, head_blocks;
  long tail_begin4;
};

// Local mode (PAAC_CLIP_LOCAL: tf.clip_by_norm per variable).  Upstream clips every entry of grads_and_vars on its own,
// so weights and biases are separate tensors with a factor each.  The norm blocks are tensor-aligned: each run of head
// blocks and each run of tail blocks covers exactly one tensor, so tensor t's partials are the contiguous slots
// [blk[t], blk[t + 1]) -- no hand-off between workgroups.  The launch has as many blocks as the global mode's
// (blk[nt] == its block count), so either mode leaves every slot the other one reads in a defined state.
struct LocalSpec {
  int nt;                              // tensors of the layout
  int blk[PAAC_MAX_TENSORS + 1];       // first norm block (= partials slot) of tensor t
  long off4[PAAC_MAX_TENSORS + 1];     // first float4 of tensor t in the padded layout; off4[nt] = n4
  float pads[PAAC_MAX_TENSORS];        // alignment pads of tensor t (zeros its partials count that upstream has not)
  float* factors;                      // [nt]: the factors applied, written by the optimizer step's block 0
};
constexpr int kNormFactors = 5 * kNormPartialsMax;   // offset of LocalSpec::factors inside ctx->partials
constexpr int kAdamAlpha = kNormFactors + PAAC_MAX_TENSORS;   // offset of the Adam step size inside ctx->partials (8192 floats)

// Adam's bias-correction powers (TF 1.0.1 AdamOptimizer: fp32 variables beta1_power / beta2_power, advanced by one fp32
// product each in _finish, after the update that used them).  Every block of the update launch reads the step size they
// give, so they cannot be advanced inside it: block 0 of the norm pass (ADAM) reads them with *lr, writes TF ApplyAdam's
//   alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power)
// to a scratch float of the ctx and stores the advanced powers.  The launch boundary orders this before every reader.
struct AdamPowers {
  float* powers;          // device float[2] {beta1_power, beta2_power}, in/out
  const float* lr;
  float* alpha;           // ctx->partials + kAdamAlpha
  float beta1, beta2;
};

// --ppo_target_kl (include/paac_hip.h has the contract): the gate of a gated optimizer step.  Block 0 thread 0 of the norm
// pass (GATED) takes the decision -- the thread that turns lr and the powers into alpha under Adam -- and every block of the
// update launch (GATED) reads *stop before it touches anything: the launch boundary orders the decision before every
// reader, exactly as it orders alpha.  Plain stores, no atomics: one writer, and the readers are in the next launch.
struct KlGate {
  const float* kl;     // the step's approx_kl (data parallel: the ranks' sum, inside the exchanged gradient store)
  float scale;         // 1, or 1 / world size
  float thr;           // float32(1.5 * target_kl)
  int first;           // first gated step of the cycle: clears *stop before the comparison
  int32_t* stop;       // sticky inside a cycle
  int32_t* applied;    // nullable: !*stop after this step's decision
  float* checked;      // nullable: the value compared
};
struct NoKlGate {};    // the ungated instantiations take no gate: their code is what it was before the flag
template <bool GATED> using KlGateArg = std::conditional_t<GATED, KlGate, NoKlGate>;

template <bool LOCAL, bool ADAM, bool GATED>
__global__ __launch_bounds__(256) void norm_kernel(float* __restrict__ g, long n4, float scale, const NormArgs a,
                                                   const LocalSpec ls, float* __restrict__ partials, const AdamPowers ap,
                                                   const KlGateArg<GATED> kg) {
  if constexpr (GATED) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      int stop = kg.first ? 0 : *kg.stop;
      const float k = *kg.kl * kg.scale;
      if (!(k <= kg.thr)) stop = 1;          // (a NaN stops too)
      *kg.stop = stop;
      if (kg.checked) *kg.checked = k;
      if (kg.applied) *kg.applied = stop ? 0 : 1;
      if constexpr (ADAM) {
        if (!stop) {
          const float b1p = ap.powers[0], b2p = ap.powers[1];
          *ap.alpha = *ap.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
          ap.powers[0] = b1p * ap.beta1;
          ap.powers[1] = b2p * ap.beta2;
        }
      }
    }
  } else if constexpr (ADAM) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const float b1p = ap.powers[0], b2p = ap.powers[1];
      *ap.alpha = *ap.lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
      ap.powers[0] = b1p * ap.beta1;
      ap.powers[1] = b2p * ap.beta2;
    }
  }
  float acc = 0.f, sum = 0.f, mx = -INFINITY, mn = INFINITY, zeros = 0.f;
  auto take = [&](const float4 q) {
    const float x = q.x * scale, y = q.y * scale, z = q.z * scale, w = q.w * scale;
    acc += (x * x + y * y) + (z * z + w * w);
    sum += (x + y) + (z + w);
    const float e[4] = {x, y, z, w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool nz = e[c] != 0.f;
      mx = fmaxf(mx, nz ? e[c] : -INFINITY);
      mn = fminf(mn, nz ? e[c] : INFINITY);
      zeros += nz ? 0.f : 1.f;
    }
  };
  float4* g4 = reinterpret_cast<float4*>(g);
  const int bid = blockIdx.x;
  int t = 0;                                     // local mode: the one tensor this block covers
  if constexpr (LOCAL) {
#pragma unroll
    for (int j = 1; j < PAAC_MAX_TENSORS; ++j) t += (j < ls.nt && bid >= ls.blk[j]) ? 1 : 0;
  }
  if (LOCAL ? t < a.nseg : bid < a.head_blocks) {
    const int r = threadIdx.x % NORM_LANES;
    long h;
    NormSeg sg = a.seg[0];
    if constexpr (LOCAL) {
      h = (long)(bid - ls.blk[t]) * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;   // float4 inside conv tensor t
#pragma unroll
      for (int j = 1; j < 6; ++j)
        if (j == t) sg = a.seg[j];
    } else {
      h = (long)bid * (256 / NORM_LANES) + threadIdx.x / NORM_LANES;   // float4 inside the concatenated conv tensors
#pragma unroll
      for (int j = 1; j < 6; ++j) {
        if (j < a.nseg && h >= sg.count4) {
          h -= sg.count4;
          sg = a.seg[j];
        }
      }
    }
    const bool live = h < sg.count4;     // whole lane groups are live or not: the shuffles below stay inside a group
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (sg.src != nullptr) {
      for (int s0 = r; s0 < sg.splits; s0 += 8 * NORM_LANES) {
        f32x4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int sp = s0 + u * NORM_LANES;
          t[u] = (live && sp < sg.splits) ? *reinterpret_cast<const f32x4*>(sg.src + (long)sp * sg.stride + 4 * h)
                                          : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) v += t[u];
      }
#pragma unroll
      for (int off = 1; off < NORM_LANES; off <<= 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += __shfl_xor(v[c], off, 64);
      }
      if (live && r == 0) *reinterpret_cast<f32x4*>(g4 + sg.dst4 + h) = v;
    } else if (live && r == 0) {
      v = *reinterpret_cast<const f32x4*>(g4 + sg.dst4 + h);
    }
    if (live && r == 0) take(make_float4(v[0], v[1], v[2], v[3]));
  } else {
    // latency-bound (a few float4 per thread): every load of a pass is issued before the first one is consumed
    // (local mode: the blocks of tail tensor t stride over its padded range only)
    constexpr int U = 8;
    const long STRIDE = LOCAL ? (long)(ls.blk[t + 1] - ls.blk[t]) * 256 : (long)NORM_BLOCKS * 256;
    const long end = LOCAL ? ls.off4[t + 1] : n4;
    const long begin = LOCAL ? ls.off4[t] + (long)(bid - ls.blk[t]) * 256 : a.tail_begin4 + (long)(bid - a.head_blocks) * 256;
    for (long i0 = begin + threadIdx.x; i0 < end; i0 += U * STRIDE) {
      float4 v[U];
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long i = i0 + u * STRIDE;
        live[u] = i < end;
        v[u] = live[u] ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (live[u]) take(v[u]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off, 64);
    sum += __shfl_down(sum, off, 64);
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
    mn = fminf(mn, __shfl_down(mn, off, 64));
    zeros += __shfl_down(zeros, off, 64);
  }
  __shared__ float red[5][4];
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = acc; red[1][w] = sum; red[2][w] = mx; red[3][w] = mn; red[4][w] = zeros;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partials[kNormPartialsMax + blockIdx.x] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    partials[2 * kNormPartialsMax + blockIdx.x] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    partials[3 * kNormPartialsMax + blockIdx.x] = fminf(fminf(red[3][0], red[3][1]), fminf(red[3][2], red[3][3]));
    partials[4 * kNormPartialsMax + blockIdx.x] = (red[4][0] + red[4][1]) + (red[4][2] + red[4][3]);
  }
}

// One workgroup: the partials of the last norm_kernel in slots [lo, hi) -> out[8] = {sum, sum of squares, max, min, exact
// zeros among the real (unpadded) elements, 0, 0, 0}.  Ends on a barrier (a caller may fold again at once).
__device__ void fold_norm_partials(const float* __restrict__ partials, int lo, int hi, float pads, float* __restrict__ out) {
  const int t = threadIdx.x;
  float ss = 0.f, sum = 0.f, mx = -INFINITY, mn = INFINITY, zeros = 0.f;
  for (int i = lo + t; i < hi; i += 256) {
    ss += partials[i];
    sum += partials[kNormPartialsMax + i];
    mx = fmaxf(mx, partials[2 * kNormPartialsMax + i]);
    mn = fminf(mn, partials[3 * kNormPartialsMax + i]);
    zeros += partials[4 * kNormPartialsMax + i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ss += __shfl_down(ss, off, 64);
    sum += __shfl_down(sum, off, 64);
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
    mn = fminf(mn, __shfl_down(mn, off, 64));
    zeros += __shfl_down(zeros, off, 64);
  }
  __shared__ float red[5][4];
  if ((t & 63) == 0) {
    const int w = t >> 6;
    red[0][w] = ss; red[1][w] = sum; red[2][w] = mx; red[3][w] = mn; red[4][w] = zeros;
  }
  __syncthreads();
  if (t == 0) {
    float a = 0.f, b = 0.f, c = -INFINITY, d = INFINITY, z = 0.f;
    for (int w = 0; w < 4; ++w) {
      a += red[0][w]; b += red[1][w]; c = fmaxf(c, red[2][w]); d = fminf(d, red[3][w]); z += red[4][w];
    }
    const float real_zeros = z - pads;
    if (real_zeros > 0.f) { c = fmaxf(c, 0.f); d = fminf(d, 0.f); }
    out[0] = b; out[1] = a; out[2] = c; out[3] = d; out[4] = real_zeros; out[5] = 0.f; out[6] = 0.f; out[7] = 0.f;
  }
  __syncthreads();
}

// The whole flat gradient: all np partials.  Launched by the host at the progress-record cadence only.
__global__ __launch_bounds__(256) void grad_stats_kernel(const float* __restrict__ partials, int np, float pads,
                                                         float* __restrict__ out) {
  fold_norm_partials(partials, 0, np, pads, out);
}

// Per tensor, after a local-mode step (tensor-aligned partials): out[t][8] = the summaries above of tensor t's raw
// gradient, with out[t][5] = the factor the step applied to it; rows nt .. PAAC_MAX_TENSORS - 1 are zero.
__global__ __launch_bounds__(256) void grad_tensor_stats_kernel(const float* __restrict__ partials, const LocalSpec ls,
                                                                float* __restrict__ out) {
  for (int t = 0; t < ls.nt; ++t) {
    fold_norm_partials(partials, ls.blk[t], ls.blk[t + 1], ls.pads[t], out + 8 * t);
    if (threadIdx.x == 0) out[8 * t + 5] = ls.factors[t];
  }
  for (int i = 8 * ls.nt + threadIdx.x; i < 8 * PAAC_MAX_TENSORS; i += 256) out[i] = 0.f;
}

constexpr int RMS_U = 4;   // float4 per thread and array in update_kernel

// What the optimizer step also maintains (csrc/tower.h, csrc/fc_heads.h): the pre-split bf16 planes of the Nature conv
// weights and the fragment-ordered copy of the fc weights -- written by the workgroup that has just updated the values, so
// no separate pack launch (and no second pass over 6.7 MB) follows an update.
struct PackSpec {
  // conv tensors [K, cout] at float offset conv_begin: tile blocks of 32 rows (one k-step) x cout columns
  int nconv;
  long conv_begin[3];
  int conv_cout[3], conv_tiles[3];   // tiles = K / 32
  long conv_dst[3];                  // offset of the layer inside the pack buffer, in 16-byte vectors
  bf16x8* conv_pack;                 // nullptr: no conv pack (NIPS, PAAC_TOWER=0)
  bf16x8* dgrad3_pack;               // conv3 / conv2 data-gradient planes (dgrad_tower.h), with conv_pack
  bf16x8* dgrad2_pack;
  // fc weights [K, H] at float offset fc_begin: tile blocks of 16 rows x 256 columns
  long fc_begin;
  int fc_K, fc_H;
  float* fc_pack;                    // nullptr: no fc pack
  // everything the tile blocks do not own, as float4 ranges walked by the flat blocks
  int nflat;
  long flat_begin4[5], flat_count4[5];
};

// One optimizer element update (TF ApplyRMSProp, actor_learner.py:31-34).
template <bool MOM>
__device__ __forceinline__ void rms_update4(float4& gv, float4& m, float4& mo, float4& v, const float f, const float lr,
                                            const float omd, const float momentum, const float eps) {
#define PAAC_RMS(c)                                        \
  {                                                        \
    const float gg = gv.c * f;                             \
    m.c = m.c + (gg * gg - m.c) * omd;                     \
    const float step = lr * gg / sqrtf(m.c + eps);         \
    mo.c = MOM ? momentum * mo.c + step : step;            \
    v.c = v.c - mo.c;                                      \
  }
  PAAC_RMS(x) PAAC_RMS(y) PAAC_RMS(z) PAAC_RMS(w)
#undef PAAC_RMS
}

// One optimizer element update (TF ApplyAdam): m = first moment, s = second moment, alpha = the bias-corrected step size
// (norm_kernel<., true>).  eps lies outside the sqrt: an exact-zero gradient on zero moments gives 0 / eps = 0.
__device__ __forceinline__ void adam_update4(float4& gv, float4& m, float4& s, float4& v, const float f, const float alpha,
                                             const float omb1, const float omb2, const float eps) {
#define PAAC_ADAM(c)                                       \
  {                                                        \
    const float gg = gv.c * f;                             \
    m.c = m.c + (gg - m.c) * omb1;                         \
    s.c = s.c + (gg * gg - s.c) * omb2;                    \
    v.c = v.c - (m.c * alpha) / (sqrtf(s.c) + eps);        \
  }
  PAAC_ADAM(x) PAAC_ADAM(y) PAAC_ADAM(z) PAAC_ADAM(w)
#undef PAAC_ADAM
}

// The update rules of update_kernel.  RULE_RMSPROP: momentum == 0 (the reference's setting, actor_learner.py:31-34): the
// momentum slot is written (it is checkpointed as OptimizerVariables_1) but not read.  RULE_ADAM: ms / mom are Adam's m /
// v, lr_dev points at the alpha norm_kernel<., true> wrote in the same step, (decay, momentum) carry (beta1, beta2).
// Block classes by blockIdx: [0, fc_tiles) one 16 x 256 tile of the fc weights; then one 32 x cout tile of a conv weight
// tensor each; then flat blocks over everything else.  A tile block streams its rows coalesced like a flat block, then
// passes the updated values through LDS into the packed order (fragments of fc_heads.h / bf16 planes of tower.h).
// LOCAL: clip_mode is PAAC_CLIP_LOCAL -- every block folds the tensor-aligned partials into per-tensor sums of squares in
// the same fixed order (the same factors everywhere), and each float4 takes the factor of the tensor it lies in.
enum { RULE_RMSPROP = 0, RULE_RMSPROP_MOM = 1, RULE_ADAM = 2 };
// GATED (--ppo_target_kl): a block whose step the norm pass has stopped returns before it reads or writes anything -- weights,
// packed copies, slots, the local factors and gnorm_out stay what the last applied step left.
template <int RULE, bool LOCAL, bool GATED>
__global__ __launch_bounds__(256) void update_kernel(float* __restrict__ var, const float* __restrict__ g,
                                                     float* __restrict__ ms, float* __restrict__ mom, long n4,
                                                     const float* __restrict__ lr_dev, float decay, float momentum,
                                                     float eps, float clip_norm, int clip_mode, float scale,
                                                     const float* __restrict__ partials, float* __restrict__ gnorm_out,
                                                     const PackSpec pk, const int fc_tiles, const int conv_tiles,
                                                     const LocalSpec ls, const KlGateArg<GATED> kg) {
  if constexpr (GATED) {
    if (*kg.stop != 0) return;               // block-uniform, in front of the first barrier
  }
  constexpr bool MOM = RULE == RULE_RMSPROP_MOM;
  __shared__ float red[4];
  __shared__ float s_factor;
  __shared__ float tile[32 * 68 > 16 * 260 ? 32 * 68 : 16 * 260];
  const int bid = blockIdx.x, tid = threadIdx.x;
  const int cls = bid < fc_tiles ? 0 : (bid < fc_tiles + conv_tiles ? 1 : 2);
  // ---- which float4s does this thread own ----------------------------------------------------------------------------
  long idx[RMS_U];       // float4 index of each of this thread's elements, -1 = none
  int cl = 0, ct_i = 0, ccout = 64;          // conv tile: layer, tile (k-step), columns
  if (cls == 0) {
    const int cblocks = pk.fc_H / 256;
    const int gI = bid / cblocks, cb = bid - gI * cblocks;
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      const int f = tid + 256 * u;           // float4 inside the tile: row f / 64, column group f % 64
      idx[u] = (pk.fc_begin + (long)(16 * gI + (f >> 6)) * pk.fc_H + 256 * cb + 4 * (f & 63)) >> 2;
    }
  } else if (cls == 1) {
    int t = bid - fc_tiles;
    while (cl < pk.nconv - 1 && t >= pk.conv_tiles[cl]) t -= pk.conv_tiles[cl++];
    ct_i = t;
    ccout = pk.conv_cout[cl];
    const int f4_per_tile = 32 * ccout / 4;  // 512 (cout 64) or 256 (cout 32): rows are contiguous, so is the tile
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      const int f = tid + 256 * u;
      idx[u] = f < f4_per_tile ? ((pk.conv_begin[cl] + (long)ct_i * 32 * ccout) >> 2) + f : -1;
    }
  } else {
    const long i0 = (long)(bid - fc_tiles - conv_tiles) * (256 * RMS_U) + tid;
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      long i = i0 + u * 256;
      long at = -1;
#pragma unroll
      for (int sgm = 0; sgm < 5; ++sgm) {
        if (sgm < pk.nflat && at < 0) {
          if (i < pk.flat_count4[sgm]) at = pk.flat_begin4[sgm] + i;
          else i -= pk.flat_count4[sgm];
        }
      }
      idx[u] = at;
    }
  }
  // the streams do not depend on the norm: request them first (RMS_U float4 per thread and array), reduce the
  // partials while they are in flight
  float4 gv[RMS_U], m[RMS_U], mo[RMS_U], v[RMS_U];
#pragma unroll
  for (int u = 0; u < RMS_U; ++u) {
    const long il = idx[u] >= 0 ? idx[u] : 0;
    gv[u] = reinterpret_cast<const float4*>(g)[il];
    m[u] = reinterpret_cast<float4*>(ms)[il];
    mo[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (RULE != RULE_RMSPROP) mo[u] = reinterpret_cast<float4*>(mom)[il];
    v[u] = reinterpret_cast<float4*>(var)[il];
  }
  const float lr = *lr_dev;
  float fu[RMS_U];       // factor (times scale) of each of this thread's float4s
  static_assert(kNormPartialsMax == 1024, "four partials per thread");
  if constexpr (LOCAL) {
    // segmented fold of the partials: 16 lanes per tensor, each summing the slots j, j + 16, ... of its tensor's range,
    // then a fixed xor tree -- the same order in every block
    __shared__ float s_p[kNormPartialsMax];
    __shared__ float s_ss[PAAC_MAX_TENSORS], s_ft[PAAC_MAX_TENSORS];
#pragma unroll
    for (int k = 0; k < 4; ++k) s_p[tid + 256 * k] = partials[tid + 256 * k];
    __syncthreads();
    const int t = tid >> 4, j = tid & 15;
    int lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < PAAC_MAX_TENSORS; ++q)
      if (q == t && q < ls.nt) {
        lo = ls.blk[q];
        hi = ls.blk[q + 1];
      }
    float acc = 0.f;
    for (int i = lo + j; i < hi; i += 16) acc += s_p[i];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
    if (j == 0 && t < ls.nt) {
      // TF 1.0.1 clip_by_norm literally: clip_norm * min(rsqrt(ss), 1 / clip_norm); ss == 0 gives 1 (no inf, no NaN)
      s_ss[t] = acc;
      s_ft[t] = clip_norm * fminf(1.0f / sqrtf(acc), 1.0f / clip_norm);
    }
    __syncthreads();
    if (tid == 0 && bid == 0) {
      // tf.global_norm of the CLIPPED gradients (actor_learner.py:64), in a fixed order
      float c2 = 0.f;
      for (int q = 0; q < ls.nt; ++q) {
        c2 += s_ft[q] * s_ft[q] * s_ss[q];
        ls.factors[q] = s_ft[q];
      }
      if (gnorm_out) *gnorm_out = sqrtf(c2);
    }
    // a tile block lies inside one tensor; a flat block's float4s may lie in several
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      if (u > 0 && cls != 2) {
        fu[u] = fu[0];
        continue;
      }
      int tt = 0;
#pragma unroll
      for (int q = 1; q < PAAC_MAX_TENSORS; ++q) tt += (q < ls.nt && idx[u] >= ls.off4[q]) ? 1 : 0;
      fu[u] = s_ft[tt] * scale;
    }
  } else {
    // every block reduces the same partials in the same order -> identical norm everywhere (unused slots hold 0)
    float acc = (partials[tid] + partials[tid + 256]) + (partials[tid + 512] + partials[tid + 768]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      const float gn = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
      float f = 1.f;
      if (clip_mode == PAAC_CLIP_GLOBAL) f = clip_norm * fminf(1.0f / gn, 1.0f / clip_norm);
      s_factor = f;
      if (gnorm_out && bid == 0) *gnorm_out = gn;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) fu[u] = s_factor * scale;
  }
  const float omd = 1.0f - decay;
#pragma unroll
  for (int u = 0; u < RMS_U; ++u) {
    if (idx[u] < 0) continue;
    if constexpr (RULE == RULE_ADAM) adam_update4(gv[u], m[u], mo[u], v[u], fu[u], lr, omd, 1.0f - momentum, eps);
    else rms_update4<MOM>(gv[u], m[u], mo[u], v[u], fu[u], lr, omd, momentum, eps);
    reinterpret_cast<float4*>(ms)[idx[u]] = m[u];
    reinterpret_cast<float4*>(mom)[idx[u]] = mo[u];
    reinterpret_cast<float4*>(var)[idx[u]] = v[u];
  }
  if (cls == 0) {
    // fc tile -> fragments [tile nt][group g][lane = 16 kq + li][s] = W[16 g + 4 kq + s][16 nt + li]
    float (*tl)[260] = reinterpret_cast<float (*)[260]>(tile);
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      const int fidx = tid + 256 * u;
      *reinterpret_cast<float4*>(&tl[fidx >> 6][4 * (fidx & 63)]) = v[u];
    }
    __syncthreads();
    const int cblocks = pk.fc_H / 256, G = pk.fc_K / 16;
    const int gI = bid / cblocks, cb = bid - gI * cblocks;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = tid + 256 * j;           // fragment: local tile q / 64, lane q % 64
      const int ntl = q >> 6, lane = q & 63, li = lane & 15, kq = lane >> 4;
      float4 o;
      o.x = tl[4 * kq + 0][16 * ntl + li];
      o.y = tl[4 * kq + 1][16 * ntl + li];
      o.z = tl[4 * kq + 2][16 * ntl + li];
      o.w = tl[4 * kq + 3][16 * ntl + li];
      reinterpret_cast<float4*>(pk.fc_pack)[((long)(16 * cb + ntl) * G + gI) * 64 + lane] = o;
    }
  } else if (cls == 1) {
    // conv tile (k-step ct_i: 32 rows x cout) -> per 16-channel tile three planes of 64 lanes x 8 bf16 (tower.h):
    // lane (ch = l & 15, kq = l >> 4) holds W[32 s + 8 kq + j][16 ct + ch], j = 0..7
    float (*tl)[68] = reinterpret_cast<float (*)[68]>(tile);
    const int f4_per_row = ccout / 4;
#pragma unroll
    for (int u = 0; u < RMS_U; ++u) {
      if (idx[u] < 0) continue;
      const int fidx = tid + 256 * u;
      *reinterpret_cast<float4*>(&tl[fidx / f4_per_row][4 * (fidx % f4_per_row)]) = v[u];
    }
    __syncthreads();
    const int ctiles = ccout / 16;
    for (int q = tid; q < ctiles * 64; q += 256) {
      const int ct = q >> 6, lane = q & 63, ch = lane & 15, kq = lane >> 4;
      float x[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) x[jj] = tl[8 * kq + jj][16 * ct + ch];
      bf16x8 h, md, l;
      split3_bf16(x, h, md, l);
      bf16x8* dst = pk.conv_pack + pk.conv_dst[cl] + ((long)ct_i * ctiles + ct) * 192 + lane;
      dst[0] = h;
      dst[64] = md;
      dst[128] = l;
    }
    // the same tile in the data-gradient order (dgrad_tower.h): row r = input channel, 8 consecutive columns = 8
    // consecutive output channels = one vector of the transposed, tap-flipped weight matrix; 32 rows x 8 groups = one
    // vector per thread
    if (cl >= 1 && ccout == 64) {
      const int r = tid >> 3, q8 = tid & 7;
      float x[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) x[jj] = tl[r][8 * q8 + jj];
      bf16x8 h, md, l;
      split3_bf16(x, h, md, l);
      bf16x8* dst;
      if (cl == 2) {                       // conv3: tile = (tap kh*3+kw, input-channel half)
        const int tap_d = 8 - (ct_i >> 1), c2 = 32 * (ct_i & 1) + r;
        const int sI = 2 * tap_d + (q8 >> 2);
        dst = pk.dgrad3_pack + ((long)sI * 4 + (c2 >> 4)) * 192 + (q8 & 3) * 16 + (c2 & 15);
      } else {                             // conv2: tile = tap kh*4+kw, rows = its 32 input channels
        const int kh = ct_i >> 2, kw = ct_i & 3;
        const int clsI = (kh & 1) * 2 + (kw & 1), tap_d = (1 - (kh >> 1)) * 2 + (1 - (kw >> 1));
        const int sI = 2 * tap_d + (q8 >> 2);
        dst = pk.dgrad2_pack + ((long)(clsI * 8 + sI) * 2 + (r >> 4)) * 192 + (q8 & 3) * 16 + (r & 15);
      }
      dst[0] = h;
      dst[64] = md;
      dst[128] = l;
    }
  }
}

// The norm pass's view of the flat gradient: the conv tensors (head blocks; with their pending slab reduction when a
// phase-3 backward left one for `grad`) and where the tail starts.  Returns the number of blocks (= partials), 0 on a
// mismatch.  grad == nullptr: layout only (paac_grad_stats), nothing is consumed.
static int fill_norm_args(paac_ctx* ctx, const float* grad, NormArgs* na) {
  const paac_layout& L = ctx->layout;
  const int nconv_t = 2 * ctx->spec.nconv;            // conv weights and biases: the first tensors of the layout
  memset(na, 0, sizeof(*na));
  const bool pending = grad != nullptr && ctx->pending_fin_grad != nullptr;
  if (pending && ctx->pending_fin_grad != grad) return 0;
  long total4 = 0;
  for (int i = 0; i < nconv_t; ++i) {
    NormSeg& sg = na->seg[na->nseg++];
    sg.dst4 = L.offset[i] / 4;
    sg.count4 = (int)(L.size[i] / 4);
    if ((L.offset[i] % 4) != 0 || (L.size[i] % 4) != 0) return 0;
    if (pending) {
      for (int j = 0; j < ctx->pending_fin.nseg; ++j) {
        const FinalizeSeg& f = ctx->pending_fin.seg[j];
        if (f.dst == grad + L.offset[i]) {
          sg.src = f.src;
          sg.splits = f.splits;
          sg.stride = f.stride;
        }
      }
      if (sg.src == nullptr) return 0;
    }
    total4 += sg.count4;
  }
  na->head_blocks = (int)((total4 + 256 / NORM_LANES - 1) / (256 / NORM_LANES));
  na->tail_begin4 = L.offset[nconv_t] / 4;
  if (na->tail_begin4 != total4) return 0;            // the conv tensors are contiguous from 0 (no pads among them)
  if (na->head_blocks + NORM_BLOCKS > kNormPartialsMax) {
    // conv tensors larger than the head blocks cover (user architectures with large conv layers): no head, the tail blocks
    // stride over the whole gradient -- the backward has reduced the slabs itself (norm_head_fits), global mode only
    if (pending) return 0;
    na->nseg = 0;
    na->head_blocks = 0;
    na->tail_begin4 = 0;
    return NORM_BLOCKS;
  }
  if (pending) ctx->pending_fin_grad = nullptr;
  return na->head_blocks + NORM_BLOCKS;
}

bool norm_head_fits(const paac_ctx* ctx) {
  long total4 = 0;
  for (int i = 0; i < 2 * ctx->spec.nconv; ++i) total4 += ctx->layout.size[i] / 4;
  return (total4 + 256 / NORM_LANES - 1) / (256 / NORM_LANES) + NORM_BLOCKS <= kNormPartialsMax;
}

// Local mode's tensor-aligned blocks, inside the np blocks the global mode launches (fill_norm_args): each conv tensor
// its own run of head blocks (32 float4 each), each small tail tensor one block per 2048 float4, the fc weights the rest.
// Returns 0 when they do not fit.
static int fill_local_spec(const paac_ctx* ctx, const NormArgs& na, int np, LocalSpec* ls) {
  const paac_layout& L = ctx->layout;
  memset(ls, 0, sizeof(*ls));
  ls->nt = L.num_tensors;
  for (int t = 0; t < L.num_tensors; ++t) {
    const long end = t + 1 < L.num_tensors ? L.offset[t + 1] : L.total;
    ls->off4[t] = L.offset[t] / 4;
    ls->pads[t] = (float)(end - L.offset[t] - L.size[t]);
  }
  ls->off4[L.num_tensors] = L.total / 4;
  const int fc_t = na.nseg;                           // the fc weights: the first tensor after the conv tensors
  int nb[PAAC_MAX_TENSORS], b = 0;
  for (int t = 0; t < L.num_tensors; ++t) {
    const long c4 = ls->off4[t + 1] - ls->off4[t];
    nb[t] = t < na.nseg ? (int)((c4 + 256 / NORM_LANES - 1) / (256 / NORM_LANES)) : (int)((c4 + 2047) / 2048);
    if (t != fc_t) b += nb[t];
  }
  nb[fc_t] = np - b;
  if (nb[fc_t] < 1) return 0;
  b = 0;
  for (int t = 0; t < L.num_tensors; ++t) {
    ls->blk[t] = b;
    b += nb[t];
  }
  ls->blk[L.num_tensors] = b;
  ls->factors = ctx->partials + kNormFactors;
  return b == np;
}

// The packed copies the optimizer step maintains and the block classes that go with them (from the ctx's layout).
static void fill_pack_spec(const paac_ctx* ctx, PackSpec* pk, int* fc_tiles, int* conv_tiles, long* flat4) {
  const paac_layout& L = ctx->layout;
  const ArchSpec& sp = ctx->spec;
  memset(pk, 0, sizeof(*pk));
  *fc_tiles = 0;
  *conv_tiles = 0;
  long owned_begin[4], owned_end[4];   // float ranges the tile blocks own, ascending
  int nowned = 0;
  if ((ctx->tower_on || ctx->tower2_on) && ctx->tower_pack) {
    pk->nconv = sp.nconv;
    long dst = 0;
    for (int i = 0; i < sp.nconv; ++i) {
      const long K = (long)sp.conv[i].k * sp.conv[i].k * sp.conv[i].cin;
      pk->conv_begin[i] = L.offset[2 * i];
      pk->conv_cout[i] = sp.conv[i].cout;
      pk->conv_tiles[i] = (int)(K / 32);
      pk->conv_dst[i] = dst;
      dst += (K / 32) * (sp.conv[i].cout / 16) * 192;
      *conv_tiles += pk->conv_tiles[i];
      owned_begin[nowned] = L.offset[2 * i];
      owned_end[nowned++] = L.offset[2 * i] + K * sp.conv[i].cout;
    }
    pk->conv_pack = reinterpret_cast<bf16x8*>(ctx->tower_pack);
    pk->dgrad3_pack = pk->conv_pack + kTowerPackVecs;
    pk->dgrad2_pack = pk->dgrad3_pack + kDgradW3Vecs;
  }
  if (ctx->fc_pack && sp.fc % 256 == 0) {
    pk->fc_begin = L.offset[2 * sp.nconv];
    pk->fc_K = sp.flat;
    pk->fc_H = sp.fc;
    pk->fc_pack = reinterpret_cast<float*>(ctx->fc_pack);
    *fc_tiles = (sp.flat / 16) * (sp.fc / 256);
    owned_begin[nowned] = pk->fc_begin;
    owned_end[nowned++] = pk->fc_begin + (long)sp.flat * sp.fc;
  }
  long at = 0;
  *flat4 = 0;
  for (int i = 0; i <= nowned; ++i) {
    const long end = i < nowned ? owned_begin[i] : L.total;
    if (end > at) {
      pk->flat_begin4[pk->nflat] = at / 4;
      pk->flat_count4[pk->nflat] = (end - at) / 4;
      *flat4 += (end - at) / 4;
      ++pk->nflat;
    }
    if (i < nowned) at = owned_end[i];
  }
}

}  // namespace paac

using namespace paac;

// paac_clip_rmsprop / paac_clip_adam and their gated twins: one norm pass, one update launch.  ap == nullptr: RMSProp (s1 = ms,
// s2 = mom, h1 = decay, h2 = momentum, step_dev = lr); otherwise Adam (s1 = m, s2 = v, h1 = beta1, h2 = beta2; the norm pass
// turns *lr_dev and the powers into alpha, which the update reads).  gate != nullptr: the GATED instantiations of both kernels
// (--ppo_target_kl), the same grids.
static int clip_step(const char* fn, paac_ctx* ctx, float* params, const float* grad, float* s1, float* s2, int64_t n,
                     const float* lr_dev, float h1, float h2, float eps, float clip_norm, int clip_mode, float grad_scale,
                     float* gnorm_out, const AdamPowers* ap, const KlGate* gate, hipStream_t s) {
  PAAC_REQUIRE(n > 0 && (n % 4) == 0, "%s: n=%ld must be a positive multiple of 4 (padded layout)", fn, (long)n);
  PAAC_REQUIRE(clip_mode == PAAC_CLIP_IGNORE || clip_mode == PAAC_CLIP_GLOBAL || clip_mode == PAAC_CLIP_LOCAL,
               "%s: clip mode %d (0 ignore, 1 global, 2 local)", fn, clip_mode);
  ProfScope ps(ctx, F_CLIP_RMSPROP, (int)(n / 4), s);   // the optimizer step's family, either rule
  const long n4 = n / 4;
  const bool local = clip_mode == PAAC_CLIP_LOCAL;
  NormArgs na;
  LocalSpec ls;
  memset(&ls, 0, sizeof(ls));
  if (local) {                                        // layout first: a refusal must leave a pending slab reduction pending
    PAAC_REQUIRE(n == ctx->layout.total, "%s: local mode needs the whole layout (n=%ld, layout %ld floats)", fn, (long)n,
                 (long)ctx->layout.total);
    const int np_layout = fill_norm_args(ctx, nullptr, &na);
    PAAC_REQUIRE(np_layout > 0 && na.head_blocks > 0 && fill_local_spec(ctx, na, np_layout, &ls),
                 "%s: the layout's tensors do not fit the local mode's norm blocks", fn);
  }
  const int np = fill_norm_args(ctx, grad, &na);
  PAAC_REQUIRE(np > 0, "%s: a slab reduction is pending for another gradient buffer, or the conv tensors need more than %d "
                       "norm blocks", fn, kNormPartialsMax - NORM_BLOCKS);
  float* g = const_cast<float*>(grad);
  AdamPowers none;
  memset(&none, 0, sizeof(none));
  const AdamPowers& pw = ap != nullptr ? *ap : none;
  const NoKlGate ungated;
#define PAAC_NORM_LAUNCH(LOCAL, ADAM)                                                                                         \
  {                                                                                                                           \
    if (gate != nullptr)                                                                                                      \
      launch_k(norm_kernel<LOCAL, ADAM, true>, dim3((unsigned)np), dim3(256), s, PROF_FIRST, g, n4, grad_scale, na, ls,       \
               ctx->partials, pw, *gate);                                                                                     \
    else                                                                                                                      \
      launch_k(norm_kernel<LOCAL, ADAM, false>, dim3((unsigned)np), dim3(256), s, PROF_FIRST, g, n4, grad_scale, na, ls,      \
               ctx->partials, pw, ungated);                                                                                   \
  }
  if (ap != nullptr) {
    if (local) PAAC_NORM_LAUNCH(true, true)
    else PAAC_NORM_LAUNCH(false, true)
  } else {
    if (local) PAAC_NORM_LAUNCH(true, false)
    else PAAC_NORM_LAUNCH(false, false)
  }
#undef PAAC_NORM_LAUNCH
  ctx->last_clip_local = local ? 1 : 0;
  PackSpec pk;
  int fc_tiles, conv_tiles;
  long flat4;
  fill_pack_spec(ctx, &pk, &fc_tiles, &conv_tiles, &flat4);
  const dim3 grid((unsigned)(fc_tiles + conv_tiles + (flat4 + 256 * RMS_U - 1) / (256 * RMS_U)));
  const float* step_dev = ap != nullptr ? ap->alpha : lr_dev;
#define PAAC_UPDATE_LAUNCH(RULE, LOCAL)                                                                                       \
  {                                                                                                                           \
    if (gate != nullptr)                                                                                                      \
      launch_k(update_kernel<RULE, LOCAL, true>, grid, dim3(256), s, PROF_LAST, params, grad, s1, s2, n4, step_dev, h1, h2,   \
               eps, clip_norm, clip_mode, grad_scale, (const float*)ctx->partials, gnorm_out, pk, fc_tiles, conv_tiles, ls,   \
               *gate);                                                                                                        \
    else                                                                                                                      \
      launch_k(update_kernel<RULE, LOCAL, false>, grid, dim3(256), s, PROF_LAST, params, grad, s1, s2, n4, step_dev, h1, h2,  \
               eps, clip_norm, clip_mode, grad_scale, (const float*)ctx->partials, gnorm_out, pk, fc_tiles, conv_tiles, ls,   \
               ungated);                                                                                                      \
  }
  if (ap != nullptr) {
    if (local) PAAC_UPDATE_LAUNCH(RULE_ADAM, true)
    else PAAC_UPDATE_LAUNCH(RULE_ADAM, false)
  } else if (h2 != 0.f) {
    if (local) PAAC_UPDATE_LAUNCH(RULE_RMSPROP_MOM, true)
    else PAAC_UPDATE_LAUNCH(RULE_RMSPROP_MOM, false)
  } else {
    if (local) PAAC_UPDATE_LAUNCH(RULE_RMSPROP, true)
    else PAAC_UPDATE_LAUNCH(RULE_RMSPROP, false)
  }
#undef PAAC_UPDATE_LAUNCH
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// The public gate -> the kernels' (same fields, same order); the refusals of the gated entries.
static int kl_gate_of(const char* fn, const paac_kl_gate* gate, KlGate* out) {
  PAAC_REQUIRE(gate != nullptr, "%s: null gate", fn);
  PAAC_REQUIRE(gate->kl != nullptr && gate->stop != nullptr, "%s: the gate's kl and stop must not be null", fn);
  PAAC_REQUIRE(gate->thr >= 0.f, "%s: gate thr=%g must be a number >= 0", fn, (double)gate->thr);      // (NaN fails)
  PAAC_REQUIRE(gate->scale > 0.f && gate->scale < INFINITY, "%s: gate scale=%g must be finite and positive", fn,
               (double)gate->scale);
  *out = KlGate{gate->kl, gate->scale, gate->thr, gate->first ? 1 : 0, gate->stop, gate->applied, gate->checked};
  return 0;
}

extern "C" {

int paac_clip_rmsprop(paac_ctx* ctx, float* params, const float* grad, float* ms, float* mom, int64_t n,
                      const float* lr_dev, float decay, float momentum, float eps, float clip_norm, int clip_mode,
                      float grad_scale, float* gnorm_out, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && grad && ms && mom && lr_dev, "paac_clip_rmsprop: null argument");
  return clip_step("paac_clip_rmsprop", ctx, params, grad, ms, mom, n, lr_dev, decay, momentum, eps, clip_norm, clip_mode,
                   grad_scale, gnorm_out, nullptr, nullptr, (hipStream_t)stream);
}

int paac_clip_rmsprop_gated(paac_ctx* ctx, float* params, const float* grad, float* ms, float* mom, int64_t n,
                            const float* lr_dev, float decay, float momentum, float eps, float clip_norm, int clip_mode,
                            float grad_scale, float* gnorm_out, const paac_kl_gate* gate, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && grad && ms && mom && lr_dev, "paac_clip_rmsprop_gated: null argument");
  KlGate kg;
  if (const int rc = kl_gate_of("paac_clip_rmsprop_gated", gate, &kg)) return rc;
  return clip_step("paac_clip_rmsprop_gated", ctx, params, grad, ms, mom, n, lr_dev, decay, momentum, eps, clip_norm,
                   clip_mode, grad_scale, gnorm_out, nullptr, &kg, (hipStream_t)stream);
}

static int adam_args_ok(const char* fn, float beta1, float beta2, float eps) {
  PAAC_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: beta1=%g and beta2=%g must lie in [0, 1)", fn,
               (double)beta1, (double)beta2);
  PAAC_REQUIRE(eps > 0.f, "%s: eps=%g must be positive", fn, (double)eps);
  return 0;
}

int paac_clip_adam(paac_ctx* ctx, float* params, const float* grad, float* m, float* v, float* beta_powers, int64_t n,
                   const float* lr_dev, float beta1, float beta2, float eps, float clip_norm, int clip_mode,
                   float grad_scale, float* gnorm_out, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && grad && m && v && beta_powers && lr_dev, "paac_clip_adam: null argument");
  if (const int rc = adam_args_ok("paac_clip_adam", beta1, beta2, eps)) return rc;
  const AdamPowers ap{beta_powers, lr_dev, ctx->partials + kAdamAlpha, beta1, beta2};
  return clip_step("paac_clip_adam", ctx, params, grad, m, v, n, lr_dev, beta1, beta2, eps, clip_norm, clip_mode, grad_scale,
                   gnorm_out, &ap, nullptr, (hipStream_t)stream);
}

int paac_clip_adam_gated(paac_ctx* ctx, float* params, const float* grad, float* m, float* v, float* beta_powers, int64_t n,
                         const float* lr_dev, float beta1, float beta2, float eps, float clip_norm, int clip_mode,
                         float grad_scale, float* gnorm_out, const paac_kl_gate* gate, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && grad && m && v && beta_powers && lr_dev, "paac_clip_adam_gated: null argument");
  if (const int rc = adam_args_ok("paac_clip_adam_gated", beta1, beta2, eps)) return rc;
  KlGate kg;
  if (const int rc = kl_gate_of("paac_clip_adam_gated", gate, &kg)) return rc;
  const AdamPowers ap{beta_powers, lr_dev, ctx->partials + kAdamAlpha, beta1, beta2};
  return clip_step("paac_clip_adam_gated", ctx, params, grad, m, v, n, lr_dev, beta1, beta2, eps, clip_norm, clip_mode,
                   grad_scale, gnorm_out, &ap, &kg, (hipStream_t)stream);
}

int paac_grad_stats(paac_ctx* ctx, float* stats_out, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && stats_out, "paac_grad_stats: null argument");
  const float pads = (float)(ctx->layout.total - ctx->layout.total_unpadded);
  NormArgs na;
  const int np = fill_norm_args(ctx, nullptr, &na);
  PAAC_REQUIRE(np > 0, "paac_grad_stats: no norm layout");
  hipLaunchKernelGGL(grad_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ctx->partials, np, pads,
                     stats_out);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_grad_tensor_stats(paac_ctx* ctx, float* out, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && out, "paac_grad_tensor_stats: null argument");
  PAAC_REQUIRE(ctx->last_clip_local, "paac_grad_tensor_stats: the last paac_clip_rmsprop on this ctx was not a local-mode "
                                     "step (per-tensor partials exist only after PAAC_CLIP_LOCAL)");
  NormArgs na;
  LocalSpec ls;
  const int np = fill_norm_args(ctx, nullptr, &na);
  PAAC_REQUIRE(np > 0 && fill_local_spec(ctx, na, np, &ls), "paac_grad_tensor_stats: no local norm layout");
  hipLaunchKernelGGL(grad_tensor_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ctx->partials, ls,
                     out);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
