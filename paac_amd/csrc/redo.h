// --redo_every (spec and numpy twin: paac_amd/redo.py): dormant units recycled at a window boundary -- incoming weights drawn
// afresh, bias and outgoing weights zeroed, optimizer slots reset (ReDo, Sokar et al., arXiv 2302.12902).  Instantiated in
// optim.hip alone: the kernels write parameters and slots, as the optimizer step does.
//
// redo_mask_kernel -- one launch, one workgroup per layer slot present
//   * the layer's `sum` words (the head of the --feature_stats block) go through LDS once, coalesced; thread 0 adds them in
//     index order in fp64 -- feature_finish_kernel's order, so the mask is the dormant set the `features` record counted --
//     and every thread then decides its units: sum[u] * units <= tau * total.  A layer whose total is 0 is left alone (mask
//     all zero, skipped = 1).  Writes mask int32[U] and counts int32[4][3] = {recycled, units, skipped} per layer slot (zeros
//     for a slot the geometry does not have).  It only reads the block.
// redo_apply_kernel -- one launch over the flat parameter buffer, memory-bound by design: masks in, sparse quads out
//   * Tensor descriptors arrive by value (RedoArgs): a weight tensor is [rows, width] with the output unit along the
//     contiguous axis and the INPUT unit of row r being r % cin (conv HWIO: rows = kh * kw * cin; fc [in, H] behind the HWC
//     flatten: row = p * C + c; heads [H, A]: row = c), a bias is one row.  So one rule serves every role: element (r, o) is
//     outgoing when mask_in[r % cin], incoming when mask_out[o]; outgoing wins.
//   * A workgroup owns one span of kRedoSpan consecutive floats of ONE tensor and stages into LDS only the mask words the
//     span can touch: the tensor's `width` output words and the input words of its own rows (all cin of them once the span
//     holds that many rows, else just those rows').  Each lane then owns quads of four consecutive floats along the output
//     axis.  A quad with no touched element loads nothing and stores nothing; a partly touched quad loads params and both
//     slots with 16-byte loads, a fully touched one does not even load; touched quads store 16 bytes to each of the three
//     arrays.  Only a lane with an incoming element runs Philox.  One writer per element, no atomics, plain vector stores.
//   * The draw: philox4x32-10 on counter (flat index lo, flat index hi, event, 0x5245444F), key (seed lo, seed hi); from word 0,
//     u = (word0 >> 8) * 2^-24 and x = -d + (d + d) * u in fp32, product rounded before the sum (fp contract off): the twin's
//     bits.
#pragma once
#include <math.h>

#include "common.h"

namespace paac {

constexpr int kRedoQuads = 4;                        // quads per lane
constexpr int kRedoSpan = 256 * kRedoQuads * 4;      // floats of one workgroup's span
constexpr int kRedoMaxUnits = 1024;                  // widest unit axis (feature_stats.Layout's bound)
constexpr int kRedoMaxTensors = 10;                  // conv / fc weights and biases, the two head weights
constexpr uint32_t kRedoStream = 0x5245444Fu;        // "REDO": the fourth counter word
enum { REDO_CONV_W = 0, REDO_FC_W = 1, REDO_HEAD_W = 2, REDO_BIAS = 3 };

struct RedoTensor {
  int64_t offset;     // first float in the flat buffer (a multiple of 4)
  int extent;         // elements
  int padded;         // floats up to the next tensor (a multiple of 4); the pads keep their bits
  int width;          // inner (output-unit) width
  int role;
  int cin;            // the input unit of row r is r % cin (1 where there is none)
  int out_off;        // mask offset of the unit axis; -1: the tensor has no incoming rule (head weights)
  int in_off;         // mask offset of the input-unit axis; -1: none (conv1, biases)
  float d;            // 1 / sqrt(fan-in) of the tensor's layer
  int block0;         // first workgroup of the tensor
};
struct RedoArgs {
  RedoTensor t[kRedoMaxTensors];
  int nt, nblocks;
};
struct RedoLayers {
  int n;
  int slot[4], units[4], unit_off[4];
  int absent[4];      // 1: the geometry has no such slot (its counts are written as zeros)
};

__global__ __launch_bounds__(256) void redo_mask_kernel(const RedoLayers L, const double* __restrict__ sum_all, double tau,
                                                        int32_t* __restrict__ mask, int32_t* __restrict__ counts) {
#pragma clang fp contract(off)
  __shared__ double s_sum[kRedoMaxUnits];
  __shared__ double s_total;
  __shared__ int s_cnt[4];
  const int t = threadIdx.x, b = blockIdx.x;
  const int slot = L.slot[b], units = L.units[b], off = L.unit_off[b];
  if (b == 0 && t < 4 && L.absent[t]) {
    counts[3 * t + 0] = 0;
    counts[3 * t + 1] = 0;
    counts[3 * t + 2] = 0;
  }
  for (int u = t; u < units; u += 256) s_sum[u] = sum_all[off + u];
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int u = 0; u < units; ++u) total = total + s_sum[u];
    s_total = total;
  }
  __syncthreads();
  const double total = s_total, bar = tau * total;
  const bool skipped = total == 0.0;
  int mine = 0;
  for (int u = t; u < units; u += 256) {
    const int m = (!skipped && s_sum[u] * (double)units <= bar) ? 1 : 0;
    mask[off + u] = m;
    mine += m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((t & 63) == 0) s_cnt[t >> 6] = mine;
  __syncthreads();
  if (t == 0) {
    counts[3 * slot + 0] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    counts[3 * slot + 1] = units;
    counts[3 * slot + 2] = skipped ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void redo_apply_kernel(const RedoArgs a, float* __restrict__ params, float* __restrict__ slot0,
                                                         float* __restrict__ slot1, const int32_t* __restrict__ mask,
                                                         const float slot0_fresh, const uint32_t k0, const uint32_t k1,
                                                         const uint32_t event) {
#pragma clang fp contract(off)
  __shared__ int s_out[kRedoMaxUnits];
  __shared__ int s_in[kRedoMaxUnits];
  const int tid = threadIdx.x, bid = blockIdx.x;
  int ti = 0;
#pragma unroll
  for (int j = 1; j < kRedoMaxTensors; ++j) ti += (j < a.nt && bid >= a.t[j].block0) ? 1 : 0;
  const RedoTensor T = a.t[ti];
  const int begin = (bid - T.block0) * kRedoSpan;          // < T.padded: the host sizes the grid
  const int end = min(begin + kRedoSpan, T.padded);
  const int W = T.width;
  if (T.out_off >= 0)
    for (int o = tid; o < W; o += 256) s_out[o] = mask[T.out_off + o];
  if (T.in_off >= 0 && begin < T.extent) {
    const int row_first = begin / W, row_last = (min(end, T.extent) - 1) / W;
    const int n = min(row_last - row_first + 1, T.cin);
    for (int i = tid; i < n; i += 256) {
      const int c = (row_first + i) % T.cin;
      s_in[c] = mask[T.in_off + c];
    }
  }
  __syncthreads();
  const bool aligned = (W & 3) == 0;                       // a quad lies inside one row
#pragma unroll
  for (int j = 0; j < kRedoQuads; ++j) {
    const int e0 = begin + 4 * (tid + 256 * j);
    if (e0 >= end) continue;
    bool zero[4], draw[4];
    int row = 0, col = 0;
    if (aligned) {
      row = e0 / W;
      col = e0 - row * W;
    }
    bool any = false, all = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = e0 + k;
      if (!aligned) {
        row = e / W;
        col = e - row * W - k;
      }
      const bool valid = e < T.extent;
      const bool outgoing = valid && T.in_off >= 0 && s_in[row % T.cin] != 0;
      const bool incoming = valid && T.out_off >= 0 && s_out[col + k] != 0;
      zero[k] = outgoing || (incoming && T.role == REDO_BIAS);
      draw[k] = incoming && !zero[k];
      any = any || zero[k] || draw[k];
      all = all && (zero[k] || draw[k]);
    }
    if (!any) continue;
    f32x4* p4 = reinterpret_cast<f32x4*>(params + T.offset + e0);
    f32x4* a4 = reinterpret_cast<f32x4*>(slot0 + T.offset + e0);
    f32x4* b4 = reinterpret_cast<f32x4*>(slot1 + T.offset + e0);
    f32x4 p = (f32x4){0.f, 0.f, 0.f, 0.f}, s0 = p, s1 = p;
    if (!all) {
      p = *p4;
      s0 = *a4;
      s1 = *b4;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(zero[k] || draw[k])) continue;
      float x = 0.f;
      if (draw[k]) {
        const uint64_t idx = (uint64_t)T.offset + (uint64_t)(e0 + k);
        uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), event, kRedoStream};
        philox4x32_10(c, k0, k1);
        const float u = (float)(c[0] >> 8) * 0x1p-24f;       // exact: 24 bits
        const float prod = (T.d + T.d) * u;
        x = -T.d + prod;
      }
      p[k] = x;
      s0[k] = slot0_fresh;
      s1[k] = 0.f;
    }
    *p4 = p;
    *a4 = s0;
    *b4 = s1;
  }
}

// The unit counts of the four layer slots of a geometry (feature_stats.Layout.of_geometry) and where each starts in the mask.
inline void redo_units_of(const ArchSpec& spec, int units[4], int unit_off[4]) {
  int at = 0;
  for (int l = 0; l < 4; ++l) {
    units[l] = l == 3 ? spec.fc : (l < spec.nconv ? spec.conv[l].cout : 0);
    unit_off[l] = at;
    at += units[l];
  }
}

// The descriptor table of ctx's layout (paac_param_layout order: conv weights and biases, fc weights and bias, actor weights
// and bias, critic weights and bias).  The head biases have no rule and no descriptor.  false: a width the kernels do not take.
inline bool redo_fill_args(const paac_ctx* ctx, RedoArgs* a, RedoLayers* layers) {
  const paac_layout& L = ctx->layout;
  const ArchSpec& sp = ctx->spec;
  memset(a, 0, sizeof(*a));
  memset(layers, 0, sizeof(*layers));
  int units[4], unit_off[4];
  redo_units_of(sp, units, unit_off);
  for (int l = 0; l < 4; ++l) {
    if (units[l] > kRedoMaxUnits) return false;
    if (units[l] == 0) {
      layers->absent[l] = 1;
      continue;
    }
    layers->slot[layers->n] = l;
    layers->units[layers->n] = units[l];
    layers->unit_off[layers->n] = unit_off[l];
    ++layers->n;
  }
  const int nc = sp.nconv;
  int block = 0;
  auto add = [&](int tensor, int role, int width, int cin, int out_off, int in_off, double fan_in) {
    RedoTensor& T = a->t[a->nt++];
    const int64_t next = tensor + 1 < L.num_tensors ? L.offset[tensor + 1] : L.total;
    T.offset = L.offset[tensor];
    T.extent = (int)L.size[tensor];
    T.padded = (int)(next - L.offset[tensor]);
    T.width = width;
    T.role = role;
    T.cin = cin;
    T.out_off = out_off;
    T.in_off = in_off;
    T.d = (float)(1.0 / sqrt(fan_in));
    T.block0 = block;
    block += (T.padded + kRedoSpan - 1) / kRedoSpan;
  };
  for (int i = 0; i < nc; ++i) {
    const ConvSpec& c = sp.conv[i];
    const double fan_in = (double)c.k * c.k * c.cin;
    add(2 * i, REDO_CONV_W, c.cout, i ? c.cin : 1, unit_off[i], i ? unit_off[i - 1] : -1, fan_in);
    add(2 * i + 1, REDO_BIAS, c.cout, 1, unit_off[i], -1, fan_in);
  }
  const int last_c = sp.conv[nc - 1].cout;
  add(2 * nc, REDO_FC_W, sp.fc, last_c, unit_off[3], unit_off[nc - 1], (double)sp.flat);
  add(2 * nc + 1, REDO_BIAS, sp.fc, 1, unit_off[3], -1, (double)sp.flat);
  add(2 * nc + 2, REDO_HEAD_W, ctx->cfg.num_actions, sp.fc, -1, unit_off[3], (double)sp.fc);
  add(2 * nc + 4, REDO_HEAD_W, 1, sp.fc, -1, unit_off[3], (double)sp.fc);
  a->nblocks = block;
  for (int i = 0; i < a->nt; ++i)
    if ((a->t[i].offset & 3) || (a->t[i].padded & 3) || a->t[i].width < 1 || a->t[i].width > kRedoMaxUnits ||
        a->t[i].cin < 1 || a->t[i].cin > kRedoMaxUnits)
      return false;
  return true;
}

}  // namespace paac
