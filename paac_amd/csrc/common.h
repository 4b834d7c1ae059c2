// Internal definitions shared by the kernel translation units of libpaac_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/paac_hip.h"

namespace paac {

void set_error(const char* fmt, ...);

// A paac_returns as its caller meant it: the estimator without the flag, and the truncation plane of the paac_returns_truncs
// the block is the head of (nullptr without the flag).
inline int returns_estimator(const paac_returns* ret) { return ret->estimator & ~PAAC_RETURNS_TRUNCS; }
inline const float* returns_truncs(const paac_returns* ret) {
  return (ret->estimator & PAAC_RETURNS_TRUNCS) ? reinterpret_cast<const paac_returns_truncs*>(ret)->truncs : nullptr;
}

#define PAAC_CHECK_HIP(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      paac::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return -2;                                                                          \
    }                                                                                     \
  } while (0)

#define PAAC_REQUIRE(cond, ...)          \
  do {                                   \
    if (!(cond)) {                       \
      paac::set_error(__VA_ARGS__);      \
      return -1;                         \
    }                                    \
  } while (0)

constexpr int OBS_H = 84, OBS_W = 84, OBS_C = 4;
constexpr int OBS_PIX = OBS_H * OBS_W;  // 7056

// Architecture description (networks.py:138-169).
struct ConvSpec {
  int ih, iw, cin, oh, ow, cout, k, stride;
};
struct ArchSpec {
  int nconv;
  ConvSpec conv[3];
  int flat;  // fc input features
  int fc;    // fc width H
};
ArchSpec arch_spec(int arch);

// Kernel families for the timing hooks (paac_prof_*).
enum Family {
  F_CONV1_FWD = 0, F_CONV2_FWD, F_CONV3_FWD, F_FC_FWD, F_HEADS_FWD,
  F_HEADS_BWD, F_FC_WGRAD, F_FC_DGRAD, F_CONV3_WGRAD, F_CONV3_DGRAD, F_CONV2_WGRAD, F_CONV2_DGRAD, F_CONV1_WGRAD,
  F_GRAD_FINALIZE, F_CLIP_RMSPROP, F_MISC,
  // the kernels around the network (entry points without a ctx: timed through the ctx profiling was enabled on)
  F_ENV_STEP, F_SAMPLE_ENV_STEP, F_SAMPLE_MT, F_SAMPLE_PHILOX, F_NSTEP_RETURNS, F_PREPROCESS_STACK, F_CONV_TOWER,
  // two contractions in one launch (dmm_pair_kernel) and the conv3 + conv2 data-gradient tower: named for what ran
  F_FC_CONV3_WGRAD, F_CONV2_CONV1_WGRAD, F_DGRAD_TOWER
};
static_assert(F_DGRAD_TOWER + 1 == PAAC_PROF_FAMILIES, "family count");

}  // namespace paac

namespace paac {
// Forward activations of one batch.  Two sets per ctx: [0] acting / bootstrap (paac_forward*), [1] training
// (paac_train_forward + paac_loss_backward) -- so the bootstrap inference of a cycle can run concurrently with
// the training forward on another stream without clobbering the activations the backward pass needs.
struct Workspace {
  float* act[3];   // conv outputs a1..a3 (fp32 NHWC)
  float* fc_slab;  // [FC_SPLITS_MAX][max_batch][H] split-K partials of the fc layer
  float* h;        // [max_batch][H] fc activations
  float* probs;    // [max_batch][A]
  float* values;   // [max_batch]
  float* logits;   // [max_batch][A]
};
}  // namespace paac

namespace paac {
// GEMM ops of the network (tuning table index) and their launch tuning record.
enum Op { OP_CONV1_FWD = 0, OP_CONV2_FWD, OP_CONV3_FWD, OP_FC_FWD, OP_FC_WGRAD, OP_FC_DGRAD, OP_CONV3_WGRAD,
          OP_CONV3_DGRAD, OP_CONV2_WGRAD, OP_CONV2_DGRAD, OP_CONV1_WGRAD, OP_CONV_TOWER, OP_COUNT };
struct Tune {
  int cfg;     // index into the family's configuration table, -1 = size heuristic
  int ksplit;  // blockIdx.z K split (slab epilogues), 0 = heuristic
  int xcd;     // grid dimension tied to the XCD (0 M tiles, 1 N tiles, 2 z), -1 none
};
inline int batch_class(int batch) { return batch > 512 ? 2 : batch > 64 ? 1 : 0; }

constexpr int kDlStride = 36;   // floats per row of paac_ctx::dl_buf (heads.h)

// dH as bf16 planes (csrc/fc_dgrad_once.h): the fc widths whose producers can stage a dH row in the LDS they already own
// (>= 1536 floats in either heads kernel), and the bytes of the plane buffer (rows padded to a multiple of 16, 3 x 2 B)
constexpr bool dh_planes_supported(int H) { return (H % 32) == 0 && H <= 1024; }
inline size_t dh_planes_bytes(int max_batch, int H) { return (size_t)((max_batch + 15) / 16 * 16) * H * 6; }

// Split-K slab reduction of the conv weight gradients into the flat gradient (net_bwd.hip): segments of one backward.
struct FinalizeSeg {
  const float* src;  // first slab
  float* dst;
  int count;         // floats
  int splits;
  long stride;       // floats between slabs
};
struct FinalizeArgs {
  FinalizeSeg seg[8];
  int nseg;
};

}  // namespace paac

namespace paac {
struct ActSample;      // csrc/synth_dev.h: what an acting step's sampler still owes; the riders of an acting fc launch
struct ActRider;
struct TowerRider;     // ... and those of the conv tower launch in front of it
struct ActFinishRecord;
}  // namespace paac

struct paac_ctx {
  paac_cfg cfg;
  paac::Tune tune[paac::OP_COUNT][3];   // [op][batch class: 0 = batch <= 64, 1 = batch <= 512, 2 = larger]
  paac::ArchSpec spec;
  paac_layout layout;
  int max_batch;
  paac::Workspace ws[2];
  int last_ws;
  float* dact[3];  // gradients wrt conv outputs (post ReLU mask)
  float* dh;       // [max_batch][H]
  // dH once more as three bf16 planes (hi, mid, lo of the exact split) in the fragment order of fc_dgrad_once_kernel
  // (csrc/fc_dgrad_once.h), rows padded to a multiple of 16; written by the heads-gradient kernels next to dh
  void* dh_planes;         // nullptr: the fc width has no plane form
  int dh_planes_rows;      // rows of the update whose planes are current (0: none -- the generic fc data gradient runs)
  int fc_dgrad_once;       // PAAC_FC_DGRAD_ONCE (default 1; read at paac_create): 0 = always the generic fc data gradient
  float* wslab;    // wgrad split-K slabs (all layers)
  int64_t wslab_floats;
  float* partials; // norm / gradient-summary partials of the last paac_clip_rmsprop / paac_clip_adam (5 x kNormPartialsMax
                   // floats), then the per-tensor factors of a local-mode step, then Adam's step size (optim.hip: kAdamAlpha)
  int last_clip_local;             // 1: the last optimizer step ran in PAAC_CLIP_LOCAL (tensor-aligned partials)
  // paac_loss_backward(phase = 3) leaves the slab reduction of the conv weight gradients to the next paac_clip_rmsprop on
  // the same gradient buffer (its norm pass does it): the segments, and the buffer they belong to
  paac::FinalizeArgs pending_fin;
  const float* pending_fin_grad;   // nullptr: nothing pending
  // paac_train_forward_trunk stopped the training forward (ws[1]) after the fc layer's split-K slabs: rows covered and
  // slab count; the next backward finishes the heads (fused into its first launch where it can)
  int heads_pending_rows, heads_pending_splits;
  // paac_keep_next_forward: the next acting forward (ws[0] routes of the conv tower + fc_heads_kernel) also leaves its rows'
  // activations -- conv1 / conv2 / conv3 outputs and the fc activations -- at rows [keep_row, keep_row + batch) of the
  // TRAINING activation set, so that an update over rows the acting steps have already computed needs no training forward
  // (weights are frozen inside a cycle).  -1 = off.  One shot, and the only thing a forward takes from the context instead
  // of from its ForwardCall (below): launch_forward alone reads it, into the call's keep_row, and resets it.
  int keep_row;
  int heads_pending_h;             // 1: the pending "slab" holds finished fc activations (bias + ReLU applied), one split
  float* zeros;                    // max(H) zero floats (the bias of heads that read finished activations)
  // csrc/mt_ahead.h: the record a spare workgroup of the acting forward's fc launch leaves for the sampling step behind it
  void* mt_ahead;                  // MtAhead, owned by the ctx
  // paac_act_step_pipe: the sample of the last pipelined step, owed until the next acting fc launch (or the flush) pays it --
  // host-side state that lives from one entry to the next: under graph capture it is resolved at capture time
  paac::ActSample* act_owed;       // owned by the ctx; ->partial == nullptr: nothing pending
  int act_region;                  // the half of ws[0].fc_slab the next ridden fc launch writes its head partials to (they
                                   // alternate: the rider beside it is still reading the other half)
  // PAAC_ACT_TOWER_RIDER (default 1; read at paac_create): what the conv tower launch of a pipelined acting step carries on its
  // helper waves -- 1: the heads finish of the owed sample, 2: also the step's frame shift (measured level with 1:
  // profiles/r10_bench.txt), 0: nothing
  int act_tower_rider;
  int act_tower_rode;              // what the tower of the last forward with riders did carry: 1 heads finish | 2 frame shift
  paac::ActFinishRecord* act_fin_rec;      // what that heads finish leaves for the sampler riding the next fc launch; owned
  float* dl_buf;                   // [max_batch][kDlStride] per-row head gradients + loss terms (heads.h)
  float* ppo_rows;                 // [max_batch][2] per-row clip / KL terms of paac_loss_backward_ppo (heads.h: ppo_stats_kernel)
  float* vclip_rows;               // [max_batch] per-row vclipped of paac_loss_backward_ppo_vclip
  int fc_splits_max;
  // conv tower (csrc/tower.h, Nature only): conv weights pre-split into bf16 planes in MFMA operand order
  void* tower_pack;      // kTowerPackVecs x 16 bytes, nullptr when the tower is off
  void* fc_pack;         // fc weights in fc_heads_kernel's fragment order (flat * H floats)
  int tower_on;          // PAAC_TOWER (default 1)
  int no_quarter_tiles;  // PAAC_FC_QUARTER=0: always whole 16 x 16 tiles (A/B measurements)
  int tower2_on;         // the two-conv tower of the stock NIPS geometry (csrc/tower2.h), same knob
  int managed_weights;   // paac_set_managed_weights: 1 = the caller keeps tower_pack current (paac_clip_rmsprop / paac_pack_weights
                         // re-pack) and acting forwards keep no conv1 / conv2 activations; 0 = every forward re-packs first
  // profiling hooks
  int prof_on;
  static constexpr int PROF_MAX_EVENTS = 8192;
  hipEvent_t* ev_start;
  hipEvent_t* ev_stop;
  int* ev_family;
  int* ev_batch;
  int* ev_mix;     // bf16 products per fp32 multiply of the launch's contraction bodies, one byte each (prof_mix)
  int ev_count;
};

namespace paac {

// Timing hooks: while a ProfScope is alive, launch_k() attaches its start/stop events to the kernel dispatch itself
// (hipExtLaunchKernelGGL: the events carry the dispatch's own begin/end timestamps, like rocprofv3's kernel trace),
// so the elapsed time is the kernel's GPU duration without marker-packet overhead.  A scope with several launches
// (first_only / last_only) puts the start on the first and the stop on the last.
struct ProfEvents {
  hipEvent_t start, stop;
  int mix, nmix;
};
extern thread_local ProfEvents g_prof;
extern paac_ctx* g_prof_ctx;   // the ctx paac_prof_enable(ctx, 1) was last called on (nullptr: none)

struct ProfScope {
  paac_ctx* ctx;
  int idx;
  ProfScope(paac_ctx* c, int family, int batch, hipStream_t) : ctx(c), idx(-1) {
    if (c && c->prof_on && c->ev_count < paac_ctx::PROF_MAX_EVENTS) {
      idx = c->ev_count++;
      c->ev_family[idx] = family;
      c->ev_batch[idx] = batch;
      g_prof.start = c->ev_start[idx];
      g_prof.stop = c->ev_stop[idx];
    }
  }
  ~ProfScope() {
    if (idx >= 0) ctx->ev_mix[idx] = g_prof.mix;
    g_prof.start = nullptr;
    g_prof.stop = nullptr;
    g_prof.mix = 0;
    g_prof.nmix = 0;
  }
};

// Instruction mix of a contraction body launched inside the current ProfScope: MFMA products issued per fp32 multiply --
// 1 = fp32 MFMA, 3 = exact-bf16 path (u8 operand x fp32 split into 3 bf16 terms), 6 = split-bf16 path.  bench.py prices
// the family against the ceiling of what it actually ran.  Up to four bodies per launch, in launch order.
inline void prof_mix(int products) {
  if (g_prof.start && g_prof.nmix < 4) g_prof.mix |= (products & 255) << (8 * g_prof.nmix++);
}

enum { PROF_WHOLE = 0, PROF_FIRST = 1, PROF_LAST = 2, PROF_NONE = 3 };
template <class K, class... Args>
inline void launch_k(K kernel, dim3 grid, dim3 block, hipStream_t s, int part, Args... args) {
  hipEvent_t st = (part == PROF_WHOLE || part == PROF_FIRST) ? g_prof.start : nullptr;
  hipEvent_t sp = (part == PROF_WHOLE || part == PROF_LAST) ? g_prof.stop : nullptr;
  if (st || sp)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, st, sp, 0, args...);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
}

// launchers implemented in the kernel translation units
int launch_deferred_heads(paac_ctx* ctx, const float* params, hipStream_t s);
// --adv_norm: the heads of the N bootstrap rows [batch, batch + N) of a pending trunk-only training forward alone (the
// rollout rows stay pending for the backward's first launch); the returns + normalisation launch (csrc/misc.hip)
int launch_bootstrap_heads(paac_ctx* ctx, const float* params, int batch, int N, hipStream_t s);
int launch_returns_norm(const paac_returns* ret, const float* v_boot, float* adv_n, double* stats, hipStream_t s);
// --ppo_minibatches' record pass: p_old / values out of the finished training-side heads (csrc/misc.hip)
int launch_record_policy(paac_ctx* ctx, const int32_t* actions, int batch, int vrows, float* p_old, float* v_out, hipStream_t s);
struct SynthStep;      // one environment step's arguments (synth_dev.h); step == nullptr / an inactive one: no environment step
// the acting forward with the counter-based sampler (and the step) inside its heads launch: fills a ForwardCall (below)
int launch_forward_sample(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* probs,
                          float* values, uint64_t seed, const uint64_t* step_base, uint64_t step_off,
                          uint32_t env_offset, int32_t* actions, const SynthStep* step, hipStream_t s);
int launch_pack_weights(paac_ctx* ctx, const float* params, hipStream_t s);
int launch_pack_dgrad(paac_ctx* ctx, const float* params, hipStream_t s);
// the fc kernel's per-tile head partials of an acting forward whose heads a later launch finishes (csrc/fc_heads.h)
struct HeadsPartials {
  const float* partial;
  int ntiles;
  const float *ba, *bc;
  float* values_out;
};
// floats of one of the two head-partial regions ridden fc launches alternate between: half of ws[0].fc_slab
inline size_t act_region_floats(const paac_ctx* c) { return (size_t)c->fc_splits_max * c->max_batch * c->spec.fc / 2; }
// the acting fc launch with riders and the flush launch of an owed sample (csrc/misc.hip, where the sampler lives)
struct FcHeadsArgs;    // fc_heads.h
int launch_fc_heads_rider(bool nature, const FcHeadsArgs& a, const ActRider& r, hipStream_t s);
int launch_act_sample_flush(const ActSample& owed, hipStream_t s);
size_t mt_ahead_bytes();
bool sampler_folds_heads(int N, int A, const void* walk_scratch);
bool tower2_available();
int synth_step_of(const char* fn, const char* what, bool in_place_ok, SynthStep* st, uint64_t seed, uint32_t env_offset, int N,
                  uint32_t thresh, const uint64_t* step_base, uint64_t step_off, const uint8_t* stack_in, uint8_t* stack_out,
                  uint8_t* stack_out2, float* rewards, float* masks, float* ep_reward, int32_t* ep_len, void* finished,
                  uint8_t* raw_scratch);
int launch_sample_mt_synth_step(const float* probs, int A, uint32_t* mt_state, int32_t* actions, const SynthStep& st,
                                void* walk_scratch, int64_t walk_scratch_bytes, const void* mt_ahead, hipStream_t stream,
                                const HeadsPartials* heads = nullptr);
// sampler only, from finished probabilities (no environment step): N <= 64 environments, N * (A - 1) <= 1024 draws
int launch_sample_mt_probs(const float* probs, int A, uint32_t* mt_state, int32_t* actions, int N, hipStream_t stream);
// false: the geometry of ctx's arch has no fc + head partials kernel (fc_heads.h: fc_heads_waves == 0), so no acting
// forward leaves head partials for a later launch (kHeadsDefer)
bool forward_has_fc_heads(const paac_ctx* ctx);
// the conv weight gradients fit the head blocks of paac_clip_rmsprop's norm pass, which can then finish their slab
// reduction (paac_loss_backward phase 3); false for user architectures with large conv layers
// One step of the generalized-advantage scan (heads.h has the contract): V = V_t, Vn = V_{t+1}, A = A_{t+1} -> A_t.  Separate
// round-to-nearest fp64 operations: no FMA contraction, so the scan equals its IEEE restatement bit for bit.
__device__ __forceinline__ void gae_step(const double gamma, const double gl, const float rw, const float mk, const double V,
                                         const double Vn, double& A) {
  const double delta = __dsub_rn(__dadd_rn((double)rw, __dmul_rn(__dmul_rn(gamma, Vn), (double)mk)), V);
  A = __dadd_rn(delta, __dmul_rn(__dmul_rn(gl, A), (double)mk));
}
// One step of the n-step return (paac.py:146-147) as numpy evaluates it: estimated_return starts as the FLOAT32 network
// output vb, so the first `gamma * estimated_return` is a float32 product (python float x float32 array -> float32, in
// numpy 1.x and 2.x alike); it is promoted to float64 by `* masks[t]` and stays float64 afterwards.  Separate
// round-to-nearest operations (no FMA contraction) keep the scan bit-identical to numpy's.  first: the step at t = T - 1.
__device__ __forceinline__ void nstep_step(const double gamma, const bool first, const float vb, const float rw, const float mk,
                                           double& R) {
  const double prod = first ? (double)__fmul_rn((float)gamma, vb) : __dmul_rn(gamma, R);
  R = __dadd_rn((double)rw, __dmul_rn(prod, (double)mk));
}
// --bootstrap_truncated (include/paac_hip.h: paac_returns.truncs has the contract): one step of either scan for the
// truncation-aware instantiations.  tr != 0: the step ended its episode at the step cap alone (its mask is 0), and the return
// bootstraps from V = V_t, the acting value of the state the step left -- an fp64 product at every t, t = T - 1 included (the
// fp32 first product belongs to the v_boot term, which a masked step does not read).  tr == 0: nstep_step / gae_step.
__device__ __forceinline__ void nstep_step_tr(const double gamma, const bool first, const float vb, const float rw, const float mk,
                                              const float tr, const double V, double& R) {
  if (tr != 0.f) R = __dadd_rn((double)rw, __dmul_rn(gamma, V));
  else nstep_step(gamma, first, vb, rw, mk, R);
}
__device__ __forceinline__ void gae_step_tr(const double gamma, const double gl, const float rw, const float mk, const float tr,
                                            const double V, const double Vn, double& A) {
  if (tr != 0.f) A = __dsub_rn(__dadd_rn((double)rw, __dmul_rn(gamma, V)), V);      // the recursion is cut as at any terminal
  else gae_step(gamma, gl, rw, mk, V, Vn, A);
}

// The per-cycle bookkeeping (paac.py:127,156; actor_learner.py:119-123), done by one thread of whichever launch computes
// the cycle's returns -- the standalone scan, the heads gradient kernels, returns_norm_kernel -- or by paac_lr_step alone.
struct CycleTick {
  int64_t* global_step;     // += step_inc, then *lr_out = f32(lr0 - step*lr0/anneal), 0 past anneal; nullable: no schedule
  int64_t step_inc;
  double lr0;
  int64_t anneal;
  float* lr_out;
  uint64_t* tick;           // += tick_inc (sampler / synthetic-env frame counter); nullable
  uint64_t tick_inc;
};
__device__ __forceinline__ void cycle_tick(const CycleTick& ct) {
  if (ct.global_step) {
    const int64_t step = *ct.global_step + ct.step_inc;
    *ct.global_step = step;
    double lr = 0.0;
    if (step <= ct.anneal) lr = ct.lr0 - ((double)step * ct.lr0 / (double)ct.anneal);
    *ct.lr_out = (float)lr;
  }
  if (ct.tick) *ct.tick += ct.tick_inc;
}

// Philox4x32-10 (oracle/sampler.py:sample_philox): the counter-based generator of the throughput sampler and the minibatch
// shuffles (csrc/misc.hip) and of the evaluation / match / ghost action streams (csrc/games.hip).
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

bool norm_head_fits(const paac_ctx* ctx);
// What one call of the forward varies in, and what the forward reports back -- everything but paac_keep_next_forward's pending
// row arrives here, nothing through the context.  The fields a call does not name are null / zero / off.
enum HeadsMode {
  kHeadsFinish = 0,        // logits, probabilities and values come out of this call
  kHeadsDefer,             // the caller's next launch finishes the heads from the fc kernel's per-tile partials (fc_heads.h):
                           // acting batches of the fc + head partials routes only
  kHeadsTrunkOnly          // training set: up to the fc layer's split-K slabs (batches above the small-batch tail only; smaller
                           // ones run the whole forward); the backward's first launch or launch_deferred_heads finishes the heads
};
struct PhiloxArgs;         // heads.h
struct ForwardCall {
  int ws;                          // activation set: 0 acting, 1 training
  float *logits, *probs, *values;  // outputs beside the set's own copies; nullable
  const PhiloxArgs* philox;        // the counter-based sampler inside the heads launch; nullable
  const SynthStep* step;           // ... and an environment step inside it too; nullable
  HeadsMode heads;
  int keep_row = -1;               // the rows are also kept at [keep_row, keep_row + batch) of the training set; -1: the pending
                                   // row of paac_keep_next_forward, if any (set 0)
  bool keep_h_only;                // with keep_row: only the fc activations are kept (bootstrap rows: the update reads nothing else)
  const uint32_t* ahead_state;     // MT19937 state a spare workgroup of the fc launch works ahead from (mt_ahead.h); nullptr: off
  int ahead_D;                     // doubles the sampling step can consume at most: N * (A - 1)
  const ActRider* rider;           // riders of the fc launch (fc_heads.h: RIDER); the caller's stack object
  const TowerRider* tower_rider;   // with rider: what the conv tower launch in front may carry instead (tower.h: RIDER)
  // results
  float* partial;                  // where the fc + head partials launch left the partials: ws[0].fc_slab, or the half of it a
  int ntiles;                      // ridden launch took; in how many column groups (16- or 8-wide tiles)
  bool rode;                       // the fc launch that carries the riders was issued
};
int launch_forward(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, ForwardCall& call, hipStream_t s);
int launch_sample_env_step_heads(const HeadsPartials& hp, float* probs_out, int A, uint32_t* mt_state, int32_t* actions,
                                 const SynthStep& st, const void* mt_ahead, hipStream_t s);
// What the heads of one backward compute (heads.h has the arithmetic of each loss): the arrays a loss reads or writes, the
// others null / zero.  ret: the returns are computed inside the heads launch and land in ret->y_out / adv_out (y / adv unused).
constexpr int kLossA3c = 0, kLossA3cRecord = 1, kLossPpo = 2, kLossPpoVclip = 3;
struct BackwardCall {
  const float* y;
  const float* adv;
  const paac_returns* ret;
  int loss;
  float* p_old_out;        // kLossA3cRecord
  const float* p_old;      // kLossPpo, kLossPpoVclip
  float clip_eps;
  float* ppo_stats_out;    // kLossPpo: [2], kLossPpoVclip: [3]; nullable
  const float* v_old;      // kLossPpoVclip
  float vclip_eps;
};
int launch_backward(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions, int batch, float beta,
                    float* grad, float* loss_out, int phase, const BackwardCall& call, hipStream_t s);

}  // namespace paac
