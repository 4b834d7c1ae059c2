/*
 * paac_hip.h -- C-ABI of libpaac_hip.so: the MI355X (gfx950) hot path of PAAC.
 *
 * The reference (arjunchandra/paac) is pure Python/TensorFlow-1 and has no FFI; the entry points
 * below are what a binding for its hot path would call, one per kernel family.  Each entry cites
 * the reference code it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; paac_last_error() gives the message
 *     (thread-local).  No exceptions cross the ABI.
 *   - the CALLER owns every tensor (device pointers + explicit dims); the library owns only the
 *     opaque paac_ctx (activation/slab workspace) and paac_graph handles.
 *   - every launch goes to the caller-supplied hipStream_t (passed as void*); no hidden host
 *     synchronisation, no allocation after paac_create -> every entry is hipGraph-capturable.
 *   - a ctx is not thread-safe; use one per process/GPU.
 *   - all floating point is fp32 (the reference graph is fp32); the n-step return scan is fp64
 *     like the reference's numpy buffers.
 */
#ifndef PAAC_HIP_H
#define PAAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct paac_ctx paac_ctx;
typedef struct paac_graph paac_graph;
typedef void* paac_stream_t; /* hipStream_t */

enum { PAAC_ARCH_NIPS = 0, PAAC_ARCH_NATURE = 1,     /* networks.py:138-151 / :154-169 */
       /* a user architecture (networks.py:117-120, README.md:80-83: "subclass the trunk"): the same trunk family -- conv
        * 8x8 / 4, conv 4x4 / 2 [, conv 3x3 / 1], fc -- with the user's filter counts (multiples of 16) and fc width (a
        * multiple of 256).  An architecture here is a compiled geometry: paac_amd/build.py builds a library for it on
        * demand (-DPAAC_USER_ARCH ...), which then serves PAAC_ARCH_NATURE and PAAC_ARCH_USER (not PAAC_ARCH_NIPS). */
       PAAC_ARCH_USER = 2 };
/* --clip_norm_type (train.py, actor_learner.py:51-64): IGNORE = no clipping; GLOBAL = tf.clip_by_global_norm over all
 * gradients; LOCAL = tf.clip_by_norm of every variable's gradient on its own (weights and biases are separate variables).
 * Upstream's 'local' branch cannot run: actor_learner.py:62-63 hands each (grad, var) tuple to tf.clip_by_norm instead
 * of the gradient.  LOCAL implements the branch's evident intent (its comment "Clip layer grads by layer norm", the help
 * text, and the tf.global_norm of the clipped gradients after it). */
enum { PAAC_CLIP_IGNORE = 0, PAAC_CLIP_GLOBAL = 1, PAAC_CLIP_LOCAL = 2 };

#define PAAC_MAX_TENSORS 12
#define PAAC_OBS_BYTES 28224 /* 84*84*4 */
#define PAAC_RAW_H 210
#define PAAC_RAW_W 160

/* Flat parameter layout, TF variable-creation order (actor_learner.py:44 grads_and_vars order;
 * pretrained checkpoints .index): conv1_w [8,8,4,C1], conv1_b, conv2_w, conv2_b, (conv3_w, conv3_b,)
 * fcN_w [K,H], fcN_b, actor_w [H,A], actor_b, critic_w [H,1], critic_b.  Every tensor starts on a
 * 4-float boundary; pad floats are zero and stay zero. */
typedef struct {
  int32_t num_tensors;
  int64_t total;          /* floats, padded */
  int64_t total_unpadded; /* the reference's parameter count P */
  int64_t offset[PAAC_MAX_TENSORS];
  int64_t size[PAAC_MAX_TENSORS];
  int32_t rank[PAAC_MAX_TENSORS];
  int32_t shape[PAAC_MAX_TENSORS][4];
  char name[PAAC_MAX_TENSORS][32];
} paac_layout;

typedef struct {
  int32_t device;      /* HIP device ordinal */
  int32_t arch;        /* PAAC_ARCH_* */
  int32_t num_actions; /* A, 2..32 */
  int32_t max_batch;   /* largest batch any forward/backward will see (N*T for training) */
} paac_cfg;

const char* paac_last_error(void);
int paac_version(void);

int paac_param_layout(int arch, int num_actions, paac_layout* out);

int paac_create(const paac_cfg* cfg, paac_ctx** out);
int paac_destroy(paac_ctx* ctx);

/* Policy/value inference: networks.py:100-169 + policy_v_network.py:24-37 (what
 * paac.py:20-23 and :140-142 fetch).  states u8 [batch,84,84,4] NHWC.  Any of logits/probs/values
 * may be NULL.  Activations stay in the ctx for a following paac_backward on the same batch. */
int paac_forward(paac_ctx* ctx, const float* params, const uint8_t* states, int batch,
                 float* logits, float* probs, float* values, paac_stream_t stream);

/* paac_forward fused with the counter-based categorical sampler (paac_sample_philox semantics) in the heads
 * kernel: what one PAACLearner.choose_next_actions call (paac.py:18-29) costs on the device-resident loop.
 * probs/values nullable; actions int32[batch]. */
int paac_forward_sample(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* probs,
                        float* values, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                        uint32_t env_offset, int32_t* actions, paac_stream_t stream);

/* paac_forward_sample with the step of the device-resident synthetic environments (paac_synth_step, path A) inside
 * the heads launch: row i's workgroup samples action i and does environment i's bookkeeping, extra workgroups shift
 * the observation stacks `states` -> `stack_out`.  One launch less per rollout step; same results as
 * paac_forward_sample followed by paac_synth_step(env_seed, ...). */
int paac_forward_sample_synth_step(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* probs,
                                   float* values, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                                   uint32_t env_offset, int32_t* actions, uint64_t env_seed, uint32_t terminal_threshold,
                                   uint8_t* stack_out, float* rewards_out, float* masks_out, float* ep_reward,
                                   int32_t* ep_len, void* finished, paac_stream_t stream);

/* Training forward alone (into the ctx's TRAINING activation set, separate from the one paac_forward* use).
 * Follow with paac_loss_backward(forward_done=1) on the same states with the same OR A SMALLER batch: activations
 * are row-major per sample, so a caller may append the bootstrap observations (paac.py:140-142) as extra rows,
 * read their values here, compute the returns, and run the backward over the first N*T rows only.
 * values: nullable f32[batch]. */
int paac_train_forward(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* values,
                       paac_stream_t stream);
/* The same without the heads (it stops after the fc layer): the next paac_loss_backward[_returns](forward_done=1) on this
 * ctx finishes them -- inside its first launch when it is a whole backward (phase 0 / 3) of the three-conv network (one
 * launch less per update; every value bit-identical), as a launch of their own otherwise.  Batches of up to 64 rows run
 * the whole forward.  With paac_loss_backward_returns and ret->v_boot == NULL the bootstrap values are taken from rows
 * [batch, batch + N) of this forward (paac.py:140-142: the bootstrap observations appended to the rollout rows). */
int paac_train_forward_trunk(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, paac_stream_t stream);

/* An update without a training forward.  Weights are frozen inside a cycle (paac.py:99-165), so the T acting forwards of a
 * rollout have already computed the activations the update's forward (paac.py:163-165) would recompute.
 * paac_keep_next_forward(ctx, r): the NEXT acting forward on this ctx (paac_forward / paac_act_step_mt of at most 256 rows,
 * three-conv network, managed weights) also leaves its rows' conv1 / conv2 / conv3 outputs and fc activations at rows
 * [r, r + batch) of the ctx's training activation set (one shot; r = -1 cancels).
 * paac_bootstrap_forward_trunk: an acting-shaped forward (conv tower + fc, no heads) of the N bootstrap observations
 * (paac.py:140-142), kept at rows [train_row, train_row + batch) -- after the T acting steps were kept at rows t*N and
 * this call at T*N, paac_loss_backward[_returns](forward_done = 1) runs on the kept rows exactly as after
 * paac_train_forward_trunk (v_boot == NULL: bootstrap values from rows [batch, batch + N)).  Same mathematics as the
 * reference's second session.run over the same observations; the values differ from a recomputed forward only by the
 * summation order of the kernels involved. */
int paac_keep_next_forward(paac_ctx* ctx, int train_row);
int paac_bootstrap_forward_trunk(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, int train_row,
                                 paac_stream_t stream);

/* One whole acting step of the device-resident loop in three launches (paac.py:104-127 for N <= 64 environments with
 * the reference's numpy sampler): policy forward on `states` (conv tower, fc with the head contractions in its epilogue),
 * then ONE launch that finishes the heads (bias, softmax; probabilities and values also written to probs_out [N,A] /
 * values_out [N]), samples the actions exactly like paac_sample_mt (np.random.multinomial(1, p - epsneg) per
 * environment on the MT19937 state, advanced in place) and steps the synthetic environments like paac_synth_step
 * (stack_out = shifted stacks with the new frame, stack_out2 (nullable) = a second copy of them; rewards / masks /
 * episode bookkeeping).
 * raw_scratch (nullable, [N,2,210,160] u8): path B like paac_synth_step's -- the step launch writes the step's raw screen
 * pairs there instead of shifting the stacks, and one more launch (paac_preprocess_stack's kernel: max of the two screens,
 * PIL-nearest resize, history push, reset on terminal) builds stack_out / stack_out2 from them: four launches.
 * stack_out == NULL (with it stack_out2, raw_scratch and the four record pointers): no environment step -- forward + heads
 * finish + sampler only, for environments that live on the host (paac.py:104-110; up to PAAC_ACT_STEP_MAX_ENVS of them).
 * A geometry without the fc + head partials kernel (a user architecture whose flattened conv output the kernel's waves do
 * not divide) runs paac_forward (heads finished into probs_out / values_out) and then the sampler [+ environment step]
 * launch of paac_sample_mt_synth_step instead: same stream, same outputs.
 * Up to PAAC_ACT_STEP_MAX_ENVS environments and N*(A-1) <= 1024 draws: the three launches above.  Beyond, up to
 * PAAC_ACT_STEP_MAX_ENVS_LARGE environments and PAAC_FUSED_SAMPLE_MAX_DRAWS draws (the 128 x 18 and 256 x 4 shards):
 * paac_forward + paac_sample_mt_synth_step in one call (four launches; lend walk_scratch as there), with the sampler's
 * MT19937 doubles made one launch ahead by a spare workgroup of the fc launch (they depend on nothing but the stream
 * position), so that the sampler workgroups load them instead of each rebuilding the state blocks. */
#define PAAC_ACT_STEP_MAX_ENVS 64
#define PAAC_ACT_STEP_MAX_ENVS_LARGE 256
int paac_act_step_mt(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, uint32_t* mt_state,
                     int32_t* actions, float* probs_out, float* values_out, uint64_t env_seed, uint32_t env_offset,
                     uint32_t terminal_threshold, const uint64_t* step_base_dev, uint64_t step_offset, uint8_t* stack_out,
                     uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                     void* finished, uint8_t* raw_scratch, void* walk_scratch, int64_t walk_scratch_bytes,
                     paac_stream_t stream);

/* paac_act_step_mt's small route with the sampler OFF the dependent chain: two launches per step, the same bits.
 * In the path-A synthetic environments the new frame and the terminal flag are functions of (seed, environment, step id)
 * alone -- only the reward bookkeeping reads the action; the fused step launch of paac_act_step_mt already shifts the stacks
 * beside the sampler on that ground.  So the shift of step t needs nothing step t computes, the conv tower of step t + 1 needs
 * only that shift, and nobody reads step t's sample before the update.  (Device games, whose frame depends on the action, have
 * no such entry.)
 * paac_act_step_pipe (paac_act_step_mt's arguments): launches the conv tower of step t, then its fc + head-partials launch,
 * which also carries (a) the frame shift of step t, states -> stack_out [/ stack_out2], dealt over the fc workgroups, and (b)
 * one extra workgroup, first in the grid, that finishes the heads, samples and does the bookkeeping of the PREVIOUS pipelined
 * step, if one is owed.  No workgroup waits for another: every rider reads only what an earlier launch wrote (the head
 * partials alternate between two regions of the acting fc slab buffer).  On return step t's stacks are enqueued, and its
 * actions, probs_out, values_out, mt_state advance, rewards, masks, episode totals and finished ring are OWED: the ctx
 * remembers the step's arguments (host-side state, like paac_keep_next_forward's; under graph capture it is resolved at
 * capture time, so a captured sequence must pay what it owes inside the capture).  The debt is paid by
 *   - the next paac_act_step_pipe (its fc launch),
 *   - paac_bootstrap_forward_trunk on the same ctx (its fc launch carries the owed sample, nothing else changes), or
 *   - paac_act_step_flush: a one-workgroup launch of the same routine (nothing owed: nothing launched).
 * All three give the bits of paac_act_step_mt.  *step_base_dev is read when the debt is paid: it must not change in between
 * (the rollout advances it once per cycle, behind the bootstrap forward).
 * Refused (nothing launched, no state changed): stack_out == NULL or stacks shifted in place; raw_scratch (path B: its
 * preprocess launch follows the step, it keeps paac_act_step_mt); shapes outside paac_act_step_mt's three-launch route
 * (batch <= PAAC_ACT_STEP_MAX_ENVS, N*(A-1) <= 1024, a geometry with the fc + head-partials kernel, and two regions of partials
 * that fit: A <= 31 at batch == max_batch).  While a sample is owed, every other acting forward on the ctx (paac_act_step_mt,
 * paac_forward*) and every entry that reads what the sample writes (paac_loss_backward*, paac_returns_norm_tick,
 * paac_record_policy) is refused with a message that names the flush.  walk_scratch is accepted and unused.
 * paac_act_step_pending: 1 while a sample is owed. */
int paac_act_step_pipe(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, uint32_t* mt_state,
                       int32_t* actions, float* probs_out, float* values_out, uint64_t env_seed, uint32_t env_offset,
                       uint32_t terminal_threshold, const uint64_t* step_base_dev, uint64_t step_offset, uint8_t* stack_out,
                       uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                       void* finished, uint8_t* raw_scratch, void* walk_scratch, int64_t walk_scratch_bytes,
                       paac_stream_t stream);
int paac_act_step_flush(paac_ctx* ctx, paac_stream_t stream);
int paac_act_step_pending(const paac_ctx* ctx);
/* PAAC_ACT_TOWER_RIDER (read at paac_create; default 1): on the Nature network, at up to 32 environments, the conv tower launch
 * of a pipelined step has four idle waves per workgroup, and carries on them -- 1: the heads finish of the owed sample (up to 7
 * actions), which leaves the sampler's inputs in a record owned by the ctx, so that the workgroup riding the next fc launch
 * only parks them; 2: also the frame shift of its own step, so that the first fc launch of a run carries nothing (measured
 * 0.6 % ahead of 1 in two sessions, beyond three times the run-to-run spread in one of them only: not the default); 0: neither
 * (the route described above).  The same bits every way.  paac_act_finish_layout: that record's size, the byte offsets of its
 * conditional probabilities / packed thresholds / probabilities / exact-zero words and the limits it is sized for (environments,
 * actions, column groups of head partials) -- eight words.  paac_act_tower_rode: what the conv tower of the last
 * paac_act_step_pipe / paac_bootstrap_forward_trunk whose fc launch was issued with riders did carry -- 1: a heads finish,
 * 2: the frame shift (host-side state, for tests and probes). */
int paac_act_finish_layout(int64_t* out, int n);
int paac_act_tower_rode(const paac_ctx* ctx);
/* paac_tower_kept_layout (host only): the eight-region conv tower (up to 32 rows) stores every kept conv1 / conv2 pixel from ONE
 * of the regions that compute it.  out[0] = the number of regions of a sample; then per region, for conv1 (20 x 20) and then
 * conv2 (9 x 9), eight words: the rectangle it computes (y, x, height, width) and the rectangle it owns, in image
 * coordinates -- 1 + 16 * regions words.  regions: 8 (the other region counts store from their GEMM epilogues: refused). */
int paac_tower_kept_layout(int regions, int64_t* out, int n);

/* Conv-weight packing.  The Nature conv layers run as one fused launch that reads the conv weights pre-split into bf16
 * planes (an internal copy owned by the ctx).  By default every paac_forward* / paac_train_forward / paac_loss_backward
 * call refreshes that copy from `params` first (one small extra launch), so a caller may change `params` at any time.
 * A caller that owns every write to `params` can switch to managed mode: paac_set_managed_weights(ctx, 1) -- then the
 * copy is refreshed only by paac_clip_rmsprop / paac_clip_adam (right behind the optimizer step) and by an explicit
 * paac_pack_weights (call it after initialising, restoring or broadcasting `params`); in managed mode the acting
 * forwards also stop keeping the conv1 / conv2 activations (only the training forward keeps them, for the backward pass). */
int paac_pack_weights(paac_ctx* ctx, const float* params, paac_stream_t stream);
int paac_set_managed_weights(paac_ctx* ctx, int on);

/* Loss + gradients of policy_v_network.py:29-57 through the whole network (what
 * optimizer.compute_gradients(loss), actor_learner.py:44, evaluates): runs the training forward
 * on `states` (unless forward_done != 0: paac_train_forward already ran on the same batch), then backward.
 * phase: 0 = everything; 1 = forward (unless done) + heads + fc layer -> the gradients of fc_w .. critic_b, i.e. the
 * contiguous tail [offset(fc_w), total) of the flat buffer (95 % of its bytes); 2 = conv layers -> the head
 * [0, offset(fc_w)).  A data-parallel caller all-reduces the tail while phase 2 still runs.  3 = everything, except that
 * the split-K slabs of the conv weight gradients are summed into `grad` by the NEXT paac_clip_rmsprop or paac_clip_adam
 * on this ctx and this `grad` (its norm pass does it, in the same order, so norm and update are bit-identical to phase 0; one launch
 * less): until then the conv part of `grad` is not valid -- for a caller that goes straight to the optimizer step.
 * actions = sampled action index per row (the one-hot's argmax,
 * paac.py:27), y = critic target, adv = advantage, batch rows t-major (paac.py:151-154).
 * grad: flat, padded layout.  loss_out (nullable, device float[4]) = {loss, actor, critic, mean entropy}. */
int paac_loss_backward(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                       const float* y, const float* adv, int batch, float entropy_beta,
                       float* grad, float* loss_out, int forward_done, int phase, paac_stream_t stream);

/* Advantage estimator of paac_loss_backward_returns.  NSTEP: paac_nstep_returns.  GAE: paac_gae_returns with gae_lambda. */
enum { PAAC_RETURNS_NSTEP = 0, PAAC_RETURNS_GAE = 1 };

/* paac_nstep_returns_tick + paac_loss_backward with the returns computed inside the backward's first launch (the heads
 * gradient kernel derives y / adv of every row from the rollout records; its last workgroup writes y_out / adv_out and
 * does the global_step / lr / frame-counter bookkeeping): one launch less per update, same values bit for bit.
 * batch must equal T*N (rows t-major, paac.py:151-154).  With phase == 2 (conv part only) `ret` is not used.
 * estimator = PAAC_RETURNS_GAE: == paac_gae_returns_tick + paac_loss_backward instead, bit for bit again. */
typedef struct {
  const float* v_boot;        /* [N] bootstrap values (float32 network output, paac.py:140-142) */
  const float* rewards;       /* [T,N] clipped rewards */
  const float* masks;         /* [T,N] 1 - terminal */
  const float* values;        /* [T,N] values of the acting forwards */
  int32_t T, N;
  double gamma;
  float* y_out;               /* [T*N] */
  float* adv_out;             /* [T*N] */
  int64_t* global_step_dev;   /* nullable: no schedule bookkeeping */
  int64_t increment;
  double initial_lr;
  int64_t lr_annealing_steps;
  float* lr_out_dev;
  uint64_t* tick_dev;         /* nullable */
  uint64_t tick_inc;
  int32_t estimator;          /* PAAC_RETURNS_NSTEP (0: the n-step return above) or PAAC_RETURNS_GAE */
  double gae_lambda;          /* in [0, 1]; read by PAAC_RETURNS_GAE only.  Both zero = a struct from before these fields */
} paac_returns;
/* --bootstrap_truncated: partial-episode bootstrapping (Pardo et al., arXiv 1712.00378) of the return at a step that was
 * terminal only because the game's step cap was reached.  The reference has no counterpart; this is the contract.
 *   The plane travels behind the block: paac_returns keeps its layout (callers compiled against it are served as before), and
 *   a caller that has a plane passes the `ret` member of a paac_returns_truncs with PAAC_RETURNS_TRUNCS or'ed into
 *   ret.estimator -- the flag says that `truncs` follows.  Every entry that takes a paac_returns reads it that way.
 *   No flag, or truncs == NULL: the entry launches the kernels it always launched, with the arguments it always passed;
 *   nothing below applies.  With a plane, tr = truncs[t, e] (such a step has mask 0), V_t = values[t, e] (the
 *   acting value of the state the step left -- the observation the cap cut off is overwritten by the reset, so this is the
 *   value of the last state seen), fp32 inputs promoted to fp64, every operation a separate round-to-nearest operation:
 *     n-step, tr = 1:  R_t = r_t + gamma*V_t            (an fp64 product at every t, t = T-1 included: the fp32 first product
 *                                                         belongs to the v_boot term, which a masked step does not read)
 *     GAE,    tr = 1:  delta_t = (r_t + gamma*V_t) - V_t;  A_t = delta_t  (the recursion is cut as at any terminal);
 *                      y_t = f32(A_t + V_t)
 *   and every step with tr = 0 is the step of paac_nstep_returns / paac_gae_returns.  An all-zero plane gives their bits.
 *   The plane is read by the truncation-aware instantiations of the kernels that compute returns (chosen at compile time,
 *   like the estimator): the backward's first launch, paac_returns_norm_tick, paac_returns_scan. */
#define PAAC_RETURNS_TRUNCS 0x100
typedef struct {
  paac_returns ret;
  const float* truncs;        /* [T,N] nullable: 1 = the step ended its episode at the step cap alone, else 0 */
} paac_returns_truncs;
int paac_loss_backward_returns(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                               const paac_returns* ret, int batch, float entropy_beta, float* grad, float* loss_out,
                               int forward_done, int phase, paac_stream_t stream);

/* --ppo_epochs K / --ppo_clip EPS: PPO's clipped-surrogate epochs (Schulman et al., arXiv 1707.06347) on one rollout.  The
 * reference has no counterpart; this is the contract.
 *   K = 1 (the default) is the update above, through the same kernels, whatever EPS says.  K > 1 (up to PAAC_PPO_EPOCHS_MAX)
 *   is K optimizer steps per rollout; EPS in (0, 1) is read only then.
 *   Epoch 1 is the update above (either estimator; global_step / lr / frame counter advance once per cycle, here) and also
 *   records p_old[i] = pi(a_i | s_i): the fp32 probability its own training-side heads computed, the value they write to the
 *   ctx's probabilities at [i, a_i] -- paac_loss_backward_returns_record, or paac_loss_backward_record.  The
 *   ratio of epoch 1 is therefore identically 1 on every route, it needs no ratio arithmetic, and its gradient is
 *   paac_loss_backward's bit for bit.  y, adv and p_old are frozen for the rest of the cycle.
 *   Epochs 2..K: paac_train_forward_trunk over the T*N rollout rows (no bootstrap rows) on the current weights, then
 *   paac_loss_backward_ppo(forward_done = 1), then the same exchange, clip and optimizer step with the same lr (Adam's powers
 *   advance per step).  Per row, fp32, no contraction, with eps = 1e-30f and s = 5/B:
 *     p = pi[act]; invq = 1/(p_old + eps); r = p*invq
 *     active = !((adv > 0 && r > 1 + EPS) || (adv < 0 && r < 1 - EPS))
 *     g_a = -(adv*(active ? 1 : 0)*1[a = act]*invq - beta*(log(pi_a + eps) + pi_a/(pi_a + eps)))
 *     dlogit_a = s*pi_a*(g_a - sum_j g_j pi_j); dv = s*0.5*(v - y)
 *     actor term = -(min(r*adv, clamp(r, 1 - EPS, 1 + EPS)*adv) + beta*entropy); entropy and critic terms unchanged
 *   (the gradient of the reference loss at the effective advantage adv*active*(p + eps)/(p_old + eps)).
 * paac_loss_backward_ppo: y / adv / p_old device float[batch]; loss_out as paac_loss_backward's (its actor entry = the mean
 * actor term above); ppo_stats_out (nullable): device float[2] = {clip_fraction = mean of !active, approx_kl = mean of
 * log(p_old + eps) - log(p + eps)}, reduced in a fixed order (one small launch), written unless phase == 2.  forward_done
 * and every phase as paac_loss_backward.  clip_eps outside (0, 1) (NaN included) and a NULL p_old are refused.
 * paac_loss_backward_record: paac_loss_backward that also writes p_old_out[batch] (not in phase 2): the recording epoch of a
 * caller that computes y / adv itself.  Gradient and loss equal paac_loss_backward's bit for bit.
 * paac_loss_backward_returns_record: the same for paac_loss_backward_returns (either estimator; paac_returns is unchanged). */
#define PAAC_PPO_EPOCHS_MAX 16
int paac_loss_backward_record(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                              const float* y, const float* adv, float* p_old_out, int batch, float entropy_beta,
                              float* grad, float* loss_out, int forward_done, int phase, paac_stream_t stream);
int paac_loss_backward_returns_record(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                                      const paac_returns* ret, float* p_old_out, int batch, float entropy_beta,
                                      float* grad, float* loss_out, int forward_done, int phase, paac_stream_t stream);
int paac_loss_backward_ppo(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                           const float* y, const float* adv, const float* p_old, float clip_eps, int batch,
                           float entropy_beta, float* grad, float* loss_out, float* ppo_stats_out, int forward_done,
                           int phase, paac_stream_t stream);

/* --ppo_vclip EPSV: the PPO2 critic term (value clipping) for epochs 2..K of a --ppo_epochs cycle.  The reference has no
 * counterpart; this is the contract.  EPSV = 0 (the default) is off: paac_loss_backward_ppo, unchanged.  Read only when K > 1.
 *   Epoch 1 is the update above; it also records v_old[i], the fp32 value its own training-side heads computed: a copy out of
 *   the ctx's value buffer right behind epoch 1's backward (paac_debug_activation(25) into the caller's array: one captured
 *   device-to-device copy; a record instantiation per estimator, action bucket and heads kernel would store the same bits at the
 *   price of sixteen more kernels).  In epoch 1 v == v_old, the term is inert and needs no arithmetic.
 *   Epochs 2..K: paac_loss_backward_ppo_vclip in place of paac_loss_backward_ppo.  Per row, fp32, no contraction:
 *     vc = v_old + fminf(fmaxf(v - v_old, -EPSV), EPSV)
 *     l1 = (y - v)^2;  l2 = (y - vc)^2;  vclipped = l2 > l1
 *     critic term = 0.25 * fmaxf(l1, l2)
 *     dv = vclipped ? 0 : s*0.5*(v - y)
 *   The actor and entropy parts are paac_loss_backward_ppo's exactly; with v_old = v the row is its row bit for bit.
 * ppo_stats_out (nullable): device float[3] = {clip_fraction, approx_kl, value_clip_fraction = mean of vclipped}, through the
 * same fixed-order reduction launch.  vclip_eps <= 0 (NaN included) and a NULL v_old are refused; everything else as
 * paac_loss_backward_ppo. */
int paac_loss_backward_ppo_vclip(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                                 const float* y, const float* adv, const float* p_old, const float* v_old, float clip_eps,
                                 float vclip_eps, int batch, float entropy_beta, float* grad, float* loss_out,
                                 float* ppo_stats_out, int forward_done, int phase, paac_stream_t stream);

/* --ppo_minibatches M: K epochs of M shuffled minibatches (arXiv 1707.06347, Algorithm 1; the PPO2 loop) in place of K full-batch
 * steps.  The reference has no counterpart; this is the contract.  M = 1 (the default) is the --ppo_epochs cycle above through
 * the same launches, bit for bit.  M is read only when K > 1.  With K > 1 and M > 1, B = T*N rows and b = B/M, one cycle is:
 *   1. Rollout and bootstrap forward, as always.
 *   2. Record pass (nothing is recorded after a weight update): paac_record_policy finishes the training-side heads of the
 *      rollout rows on the pre-update weights and writes p_old[i] = pi(a_i | s_i) (and v_old[i] under --ppo_vclip); y and adv
 *      come from the returns launches above (paac_nstep_returns_tick / paac_gae_returns_tick / paac_returns_norm_tick: the same
 *      bits as the M = 1 cycle's for the same rollout and weights; the schedule bookkeeping happens here, once per cycle); adv_n
 *      is normalised over the whole rollout, not per minibatch.  y, adv, adv_n, p_old, v_old are frozen from here on.
 *   3. Permutations, ONE launch for all K epochs (paac_minibatch_perms): for epoch e and row i, key_i = word 0 of
 *      philox4x32-10(ctr = {i, step lo, step hi, 0x504D0000 + e}; key = seed), step = *step_base_dev + step_offset (base in
 *      memory + immediate offset like paac_sample_philox: a replayed graph draws a fresh shuffle every cycle; the learner passes
 *      --sampler_seed and the cycle's frame counter).  perm_e = the row indices in ascending (key_i, i) order
 *      (np.argsort(keys, kind="stable")).  Minibatch j of epoch e is perm_e[j*b : (j+1)*b].  Nothing rank-specific enters the
 *      counter: every data-parallel rank applies the same permutation to its own shard.
 *   4. Per epoch ONE gather launch (paac_gather_minibatch): states_p[r] = states[perm_e[r]] into a staging block allocated once
 *      (fixed addresses under replay), the same index map on actions, y, the array the actor term reads (adv or adv_n), p_old
 *      and v_old.
 *   5. Per minibatch j: paac_train_forward_trunk on rows [j*b, (j+1)*b) of the staging block, paac_loss_backward_ppo[_vclip]
 *      with batch = b (every mean is over the minibatch), the exchange under data parallelism (one all-reduce per step), the
 *      same clip and optimizer step with the cycle's one lr (Adam's powers advance per step).  All K epochs run this way, the
 *      first included: an M > 1 cycle has no full-batch update, K*M optimizer steps.  (The first step runs on the weights
 *      p_old was recorded on: nothing is clipped there, and its ratio is 1 -- exactly when the record pass and the step's
 *      forward run the same kernels, up to the summation order of kept acting rows against a recomputed trunk otherwise.)
 *   Refused: M outside [1, PAAC_PPO_MINIBATCHES_MAX], M that does not divide T*N, K*M > PAAC_PPO_STEPS_MAX (a captured cycle
 *   grows by about ten launches per step), T*N > PAAC_MINIBATCH_MAX_ROWS with M > 1.
 * paac_minibatch_perms: perms_out = device int32[epochs][B], epoch e's permutation of 0..B-1 at row e.  One workgroup per epoch
 * sorts 64-bit (key << 32 | row) composites in LDS (64 KB at PAAC_MINIBATCH_MAX_ROWS rows); a B that is no power of two is padded
 * with composites (0xFFFFFFFF << 32 | row >= B), larger than every real pair even when a real key is 0xFFFFFFFF.
 * step_base_dev may be NULL (base 0).
 * paac_gather_minibatch: out[r] = in[perm[r]] for r < B.  states / states_out: u8 [B,84,84,4], 16-byte aligned, moved as 16-byte
 * vectors (1764 per row); actions (int32), y, adv, p_old, v_old (float), each [B].  Every array comes with its output or both
 * are NULL (any of them, the states included); an output that overlaps its input is refused.  perm entries outside [0, B) are
 * skipped (nothing is read through them).
 * paac_record_policy: the heads of a pending trunk-only training forward (paac_train_forward_trunk, or kept acting rows +
 * paac_bootstrap_forward_trunk) are finished by the launch a backward that cannot fuse them would run (all pending rows, on
 * `params`); after a whole training forward nothing is pending and nothing is recomputed.  Then one small launch writes
 * p_old_out[i] = probabilities[i, actions[i]] for i < batch and v_out[i] = value[i] for i < value_rows, straight out of the ctx's
 * training-side head outputs (what paac_debug_activation(26) / (25) copy).  value_rows may exceed batch: with the bootstrap
 * observations appended as rows [batch, batch + N), v_out[batch ...] are the bootstrap values the returns launch needs.
 * p_old_out or v_out may be NULL (not both).  No gradient; a following paac_loss_backward*(forward_done = 1) finds the heads
 * finished and computes the gradient it computes without this call, bit for bit. */
#define PAAC_PPO_MINIBATCHES_MAX 16
#define PAAC_PPO_STEPS_MAX 64
#define PAAC_MINIBATCH_MAX_ROWS 8192
int paac_minibatch_perms(int B, int epochs, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                         int32_t* perms_out, paac_stream_t stream);
int paac_gather_minibatch(const int32_t* perm, int B, const uint8_t* states, uint8_t* states_out, const int32_t* actions,
                          int32_t* actions_out, const float* y, float* y_out, const float* adv, float* adv_out,
                          const float* p_old, float* p_old_out, const float* v_old, float* v_old_out, paac_stream_t stream);
int paac_record_policy(paac_ctx* ctx, const float* params, const int32_t* actions, int batch, float* p_old_out, float* v_out,
                       int value_rows, paac_stream_t stream);

/* Gradient clipping + RMSPropOptimizer.apply_gradients (actor_learner.py:31-34,51-64,70):
 *   g <- grad * grad_scale           (grad_scale = 1/world_size after the sum all-reduce)
 *   mode IGNORE: f = 1
 *   mode GLOBAL: gn = sqrt(sum g^2); g <- g * f, f = clip_norm*min(1/gn, 1/clip_norm)   (tf.clip_by_global_norm)
 *   mode LOCAL:  per tensor i of the layout (weights and biases separately): ss_i = sum g_i^2 over its elements;
 *                g_i <- g_i * f_i, f_i = clip_norm*min(rsqrt(ss_i), 1/clip_norm)        (tf.clip_by_norm, TF 1.0.1);
 *                ss_i == 0 gives f_i = 1
 *   ms += (g^2 - ms)(1-decay); mom = momentum*mom + lr*g/sqrt(ms+eps); var -= mom
 * lr is read from device memory (*lr_dev) so the call can sit in a replayed graph.
 * gnorm_out (nullable): device float receiving the global norm the reference's global_norm tensor holds: of the RAW
 * gradient g in modes IGNORE and GLOBAL, of the CLIPPED gradient, sqrt(sum_i f_i^2 ss_i), in mode LOCAL.  LOCAL needs
 * n = the layout's total.  Every mode is two launches (norm pass, update), deterministic (no float atomics).
 * After paac_loss_backward(phase = 3) on the same `grad` the norm pass first completes the conv part of `grad` (which is
 * therefore written although the parameter is const). */
int paac_clip_rmsprop(paac_ctx* ctx, float* params, const float* grad, float* ms, float* mom, int64_t n,
                      const float* lr_dev, float decay, float momentum, float eps, float clip_norm,
                      int clip_mode, float grad_scale, float* gnorm_out, paac_stream_t stream);

/* Gradient clipping + tf.train.AdamOptimizer(lr, beta1, beta2, epsilon=eps).apply_gradients (TF 1.0.1 ApplyAdam), the
 * alternative update rule to paac_clip_rmsprop's on the same clipped gradient g (grad_scale and the modes IGNORE /
 * GLOBAL / LOCAL exactly as there):
 *   alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power)
 *   m += (g - m)(1-beta1); v += (g^2 - v)(1-beta2); var -= m*alpha / (sqrt(v) + eps)
 *   beta1_power *= beta1; beta2_power *= beta2      (fp32 products, after the update: Adam's _finish)
 * beta_powers: device float[2] = {beta1_power, beta2_power}, read and advanced on the device (start them at {beta1, beta2}
 * and the zeros for m and v).  lr is read from device memory (*lr_dev) like paac_clip_rmsprop's, so the call can sit
 * in a replayed graph.  Two launches: the norm pass's first workgroup also turns lr and the powers into alpha (a ctx scratch
 * float) and advances the powers; the update reads alpha.  beta1 and beta2 must lie in [0, 1), eps must be positive.
 * Everything else is paac_clip_rmsprop's contract: n % 4 == 0, LOCAL needs the whole layout, a pending phase-3 slab
 * reduction of `grad` is completed, the packed weights are refreshed in managed mode, gnorm_out, paac_grad_stats and
 * paac_grad_tensor_stats report this step. */
int paac_clip_adam(paac_ctx* ctx, float* params, const float* grad, float* m, float* v, float* beta_powers, int64_t n,
                   const float* lr_dev, float beta1, float beta2, float eps, float clip_norm, int clip_mode,
                   float grad_scale, float* gnorm_out, paac_stream_t stream);

/* --ppo_target_kl D: KL early stopping of a cycle's optimizer steps (Spinning Up's PPO rule, on the approx_kl this library
 * already computes).  The reference has no counterpart; this is the contract.  D = 0 (the default) is off: every step goes
 * through the ungated entries above, bit for bit.  D is read only when --ppo_epochs K > 1.  With D > 0:
 *   Gated steps: the optimizer steps whose backward writes a ppo_stats row.  M = 1: steps s = 1 .. K-1 (step 0 is the plain
 *     update, its ratio is identically 1, it is never gated).  M > 1: every step s = 0 .. K*M-1.
 *   The statistic: before a gated step is applied, kl_s = ppo_stats[s][1], the approx_kl of that step's own batch, the mean
 *     of log(p_old + eps) - log(p + eps).
 *   The stop rule: if !(kl_s <= thr), thr = float32(1.5 * D), this step and every remaining step of the cycle are skipped.
 *     A NaN stops too.
 *   A skipped step writes nothing to the weights, the packed weight copies, the optimizer slots or Adam's beta_powers, and
 *     leaves gnorm_out (and the local mode's factors) as the last applied step left them.  The norm pass's other work still
 *     happens -- a pending phase-3 slab reduction of `grad` is completed, the gradient-statistics partials are those of this
 *     step's gradient -- so the ctx is in the state an applied step leaves.
 *   The stop flag is sticky: the first gated step of each cycle clears it (first != 0) and nothing else does.
 *   global_step, the learning rate and the frame counter are per cycle and unaffected.
 *   No launch is added or removed: a skipped step's forward, backward and both optimizer launches still run (a captured cycle
 *     keeps its shape); the update launch's workgroups return at once.
 *   Data parallelism: the value compared is the mean of the ranks' kl_s (equal shards).  It travels inside the step's one
 *     all-reduce -- the learner keeps the gradient in a store of n + 4 floats, copies ppo_stats[s][1] to element n behind the
 *     backward, exchanges the whole store and passes kl = store + n, scale = grad_scale -- so every rank takes the same
 *     decision from the same bits.  One process: kl = ppo_stats[s] + 1, scale = 1.
 * paac_kl_gate, all pointers in device memory: the norm pass's first thread clears *stop if first, computes k = *kl * scale,
 * writes *checked = k, sets *stop = 1 if !(k <= thr), writes *applied = !*stop, and under Adam advances the powers (and writes
 * alpha) only when not stopped; every workgroup of the update launch reads *stop first and returns if it is set.  Plain
 * stores; the launch boundary orders the decision before its readers.  The gate is an argument of the call: the ctx keeps
 * nothing of it.
 * paac_clip_rmsprop_gated / paac_clip_adam_gated: their ungated twin's arguments and contract, plus the gate.  Refused: a NULL
 * gate, a NULL kl or stop, thr NaN or negative, scale not finite and positive.  applied and checked may be NULL. */
typedef struct {
  const float* kl;
  float scale;
  float thr;
  int first;
  int32_t* stop;
  int32_t* applied;
  float* checked;
} paac_kl_gate;
int paac_clip_rmsprop_gated(paac_ctx* ctx, float* params, const float* grad, float* ms, float* mom, int64_t n,
                            const float* lr_dev, float decay, float momentum, float eps, float clip_norm, int clip_mode,
                            float grad_scale, float* gnorm_out, const paac_kl_gate* gate, paac_stream_t stream);
int paac_clip_adam_gated(paac_ctx* ctx, float* params, const float* grad, float* m, float* v, float* beta_powers, int64_t n,
                         const float* lr_dev, float beta1, float beta2, float eps, float clip_norm, int clip_mode,
                         float grad_scale, float* gnorm_out, const paac_kl_gate* gate, paac_stream_t stream);

/* The reference's gradient summaries (actor_learner.py:85-87 -> logger_utils.py:23-33: mean, stddev, max, min of the
 * flat raw gradient and of the flat clipped gradient, plus global_norm): the reductions ride along the norm pass of
 * the LAST paac_clip_rmsprop / paac_clip_adam on this ctx (no extra pass over the gradient); this call only folds its
 * per-block partials.  stats_out: device float[8] = {sum, sum of squares, max, min, number of exact zeros, 0, 0, 0} of the raw
 * flat gradient (g * grad_scale) over the reference's P elements (alignment pads excluded), in every mode.  In modes
 * IGNORE and GLOBAL the clipped gradient is the raw one times one factor, so its statistics follow; in mode LOCAL they
 * follow from paac_grad_tensor_stats.  Call at the logging cadence.
 * After a gated step that was skipped (--ppo_target_kl) the partials are those of the skipped step's gradient, the last one
 * computed and not applied, while gnorm_out and the local mode's factors are still the last applied step's: the summaries then
 * describe a gradient no update used. */
int paac_grad_stats(paac_ctx* ctx, float* stats_out, paac_stream_t stream);

/* Per-tensor summaries of the last paac_clip_rmsprop / paac_clip_adam, which must have run in mode LOCAL (fails
 * otherwise): out: device float[PAAC_MAX_TENSORS][8], row i = {sum, sum of squares, max, min, exact zeros, factor f_i applied, 0, 0} of tensor
 * i's raw gradient (g * grad_scale, its alignment pads excluded); rows past the layout's tensors are zero.  The clipped
 * tensor is the raw one times f_i.  Call at the logging cadence. */
int paac_grad_tensor_stats(paac_ctx* ctx, float* out, paac_stream_t stream);

/* actor_learner.py:119-123 + paac.py:127: *global_step += increment; *lr_out = f32(lr0 - step*lr0/anneal)
 * (0 beyond anneal); evaluated in fp64 like the reference's Python float. */
int paac_lr_step(int64_t* global_step_dev, int64_t increment, double initial_lr, int64_t lr_annealing_steps,
                 float* lr_out_dev, paac_stream_t stream);

/* paac.py:140-149: R = v_boot; for t = T-1..0: R = r_t + gamma*R*m_t; y_t = R; adv_t = R - V_t.
 * fp64 scan, fp32 in/out.  rewards/masks/values/y/adv are [T,N] (t-major). */
int paac_nstep_returns(const float* v_boot, const float* rewards, const float* masks, const float* values,
                       int T, int N, double gamma, float* y, float* adv, paac_stream_t stream);

/* paac_nstep_returns + paac_lr_step (+ an optional counter bump) in ONE launch: the end-of-rollout bookkeeping of
 * paac.py:127,140-156.  tick_dev may be NULL. */
int paac_nstep_returns_tick(const float* v_boot, const float* rewards, const float* masks, const float* values,
                            int T, int N, double gamma, float* y, float* adv, int64_t* global_step_dev,
                            int64_t increment, double initial_lr, int64_t lr_annealing_steps, float* lr_out_dev,
                            uint64_t* tick_dev, uint64_t tick_inc, paac_stream_t stream);

/* Generalized advantage estimation (Schulman et al., arXiv 1506.02438) on the same records, beside the reference's n-step
 * return.  With V_T = v_boot, the fp32 inputs promoted to fp64 and every operation a separate round-to-nearest fp64
 * operation (gl = gamma * gae_lambda, one fp64 product):
 *   A = 0; for t = T-1..0: delta = (r_t + (gamma*V_{t+1})*m_t) - V_t; A = delta + (gl*A)*m_t;
 *                          adv_t = f32(A); y_t = f32(A + V_t)
 * gae_lambda in [0, 1]: 0 = the one-step TD error; 1 = the n-step return up to the last place (use paac_nstep_returns
 * for the reference's values bit for bit). */
int paac_gae_returns(const float* v_boot, const float* rewards, const float* masks, const float* values,
                     int T, int N, double gamma, double gae_lambda, float* y, float* adv, paac_stream_t stream);

/* paac_gae_returns + the bookkeeping of paac_nstep_returns_tick in ONE launch. */
int paac_gae_returns_tick(const float* v_boot, const float* rewards, const float* masks, const float* values,
                          int T, int N, double gamma, double gae_lambda, float* y, float* adv, int64_t* global_step_dev,
                          int64_t increment, double initial_lr, int64_t lr_annealing_steps, float* lr_out_dev,
                          uint64_t* tick_dev, uint64_t tick_inc, paac_stream_t stream);

/* --adv_norm: advantage normalisation.  The reference has no counterpart; this is the contract.
 *   The statistics are taken per rank and per rollout, over the B = T*N advantages the estimator (n-step or GAE) produced:
 *     mean = sum(adv) / B;  std = sqrt(sum((adv - mean)^2) / B)      (fp32 adv promoted to fp64; population form, two passes)
 *     adv_n[i] = f32((adv[i] - mean) / (std + 1e-8))
 *   One workgroup, a fixed summation order, no float atomics: the same inputs give the same bits on every launch, replayed
 *   from a graph or not.  std == 0 (B = 1, a rollout of identical advantages) gives all zeros; non-finite inputs propagate.
 *   Only the actor term reads adv_n (pass it as `adv` of paac_loss_backward* / paac_loss_backward_ppo*), in every epoch; y, the
 *   critic term and the recorded adv array are unchanged.  Under data parallelism every rank normalises its own shard: no
 *   collective is added, and G ranks x N environments is not the same update as one rank with G*N environments.
 * paac_adv_normalize: standalone.  adv / adv_n_out: device float[B] (may be the same array); stats_out (nullable): device
 * double[2] = {mean, std}.
 * paac_returns_norm_tick: paac_nstep_returns_tick or paac_gae_returns_tick (by ret->estimator; y_out / adv_out equal theirs bit
 * for bit, and so does the global_step / lr / frame-counter bookkeeping, which is optional here as in paac_returns) + the
 * normalisation of adv_out into adv_n_out (== paac_adv_normalize's bits), in ONE launch.  The returns cannot ride inside the
 * backward's first launch when the flag is on -- a row's workgroup cannot know the batch-wide mean -- so the cycle becomes:
 * training forward (trunk), this call, paac_loss_backward[_record](y_out, adv_n_out, forward_done = 1).
 * ret->v_boot == NULL: the bootstrap values are rows [T*N, T*N + N) of the training forward that has already run on `ctx`
 * (paac_train_forward[_trunk] over T*N + N rows, or kept acting rows + paac_bootstrap_forward_trunk): a pending trunk-only
 * forward gets the heads of those N rows finished here (one launch; the rollout rows stay pending, kept rows stay kept, and
 * the backward's first launch finishes them as usual).  With ret->v_boot set, ctx and params may be NULL. */
int paac_adv_normalize(const float* adv, int B, float* adv_n_out, double* stats_out, paac_stream_t stream);
/* paac_nstep_returns[_tick] / paac_gae_returns[_tick] from the argument block: the estimator by ret->estimator, the
 * bookkeeping of the _tick entries when ret->global_step_dev is set (tick_dev optional as there), y_out / adv_out written,
 * v_boot required -- and the truncation plane read (contract: paac_returns_truncs above).  No plane launches the kernel of the entry
 * named first with its arguments; an all-zero plane gives the same bits through the truncation-aware kernel. */
int paac_returns_scan(const paac_returns* ret, paac_stream_t stream);
int paac_returns_norm_tick(paac_ctx* ctx, const float* params, const paac_returns* ret, float* adv_n_out, double* stats_out,
                           paac_stream_t stream);

/* --window_stats (spec and numpy twin: paac_amd/window_stats.py): one finished cycle folded into the running accumulators of
 * the log window, acc_f device double[n_f] and acc_i device int64[n_i] (paac_window_fields reports the two lengths; the field
 * offsets are window_stats.FIELDS_F / FIELDS_I; all zero bytes = an empty window).  ONE launch of one workgroup of 256 threads,
 * no atomics, capturable; it only reads its inputs and reads and writes the block.
 *   planes    values, rewards, masks, y, adv float[T*N] and actions int32[T*N], row t * N + n; truncs float[T*N], nullable (the
 *             plane of --bootstrap_truncated): sums of v, v^2, y, y^2, y - v, (y - v)^2, adv, adv^2 and the clipped reward, max
 *             |adv|, counts of masks == 0, truncs != 0, rewards != 0 and of every action in [0, A).  Thread i takes rows i,
 *             i + 256, ... in order, in fp64, every product and sum a separate round-to-nearest operation; the 256 partials are
 *             added in index order
 *   update    loss float[steps, 4], one row per optimizer step of the cycle (loss0, nullable float[4]: read in place of row 0);
 *             ppo_stats, nullable float[steps, stats_cols], stats_cols 2 or 3 (column 2, value_clip_fraction, is live only with
 *             3), summed over the steps >= stats_first; applied, nullable int32[steps] (--ppo_target_kl: steps with a non-zero
 *             entry count as applied; NULL: all do); gnorm float[1], summed and maximised once per cycle
 *   finished  nullable: the finished-episode ring (paac_synth_step).  Entries [acc_i[ring_cursor], count) are new; at most the
 *             newest 4096 of them survive in the ring and are folded (sum and sum of squares of return and length, min and max,
 *             which the fold that sees the window's first episode sets), the rest are counted as dropped; ring_cursor = count
 * Refused with a message naming the argument, without a launch: a null pointer among in, acc_f, acc_i, the six planes, loss and
 * gnorm; T * N < 1; A outside [2, 32]; steps outside [1, PAAC_PPO_STEPS_MAX]; with ppo_stats, stats_cols other than 2 or 3 and
 * stats_first outside [0, steps]. */
typedef struct {
  int32_t T, N, A;
  const float* values;
  const float* rewards;
  const float* masks;
  const int32_t* actions;
  const float* y;
  const float* adv;
  const float* truncs;
  const float* loss;
  const float* loss0;
  int32_t steps;
  const float* ppo_stats;
  int32_t stats_cols;
  int32_t stats_first;
  const int32_t* applied;
  const float* gnorm;
  const void* finished;
} paac_window_inputs;
int paac_window_fields(int* n_f, int* n_i);
int paac_window_fold(const paac_window_inputs* in, double* acc_f, int64_t* acc_i, paac_stream_t stream);

/* paac.py:34-45 bit-exact: probs - float32.epsneg, then numpy legacy multinomial(1, p) per env in
 * index order on ONE MT19937 stream.  mt_state: device uint32[625] = numpy key[624] + pos, advanced
 * in place (import/export with np.random.get_state()/set_state()).  scratch: device, >=
 * paac_sample_mt_scratch_bytes(N, A). */
int64_t paac_sample_mt_scratch_bytes(int N, int A);
int paac_sample_mt(const float* probs, int N, int A, uint32_t* mt_state, void* scratch, int32_t* actions,
                   paac_stream_t stream);

/* Throughput sampler (build's own spec, oracle/sampler.py:sample_philox): u = philox4x32-10
 * (ctr = {env_offset+e, step lo, step hi, 0}; key = seed) with step = *step_base_dev + step_offset,
 * action = inverse CDF on fp32 running sums.  The base lives in device memory and the offset is an
 * immediate so a captured graph of T steps replays with a fresh base (paac_counter_add, once per cycle). */
int paac_sample_philox(const float* probs, int N, int A, uint64_t seed, const uint64_t* step_base_dev,
                       uint64_t step_offset, uint32_t env_offset, int32_t* actions, paac_stream_t stream);
int paac_counter_add(uint64_t* counter_dev, uint64_t inc, paac_stream_t stream);

/* emulator_runner.py:18-33 frame path on device: FramePool max over 2 raw frames
 * (atari_emulator.py:72), PIL-nearest resize 210x160 -> 84x84 (:73), ObservationPool push + rotated
 * read-out (environment.py:66-71).  raw: u8 [N,2,210,160] (gray) or [N,2,210,160,3] (rgb, converted with
 * the ITU-R 601 fixed-point luma).  stack_in/stack_out: u8 [N,84,84,4] oldest..newest (may alias).
 * push_mask (nullable): u8[N], 0 = copy the env's stack through unchanged.
 * reset_mask (nullable): u8[N], !=0 = the three older channels are cleared before the push. */
int paac_preprocess_stack(const uint8_t* raw, int is_rgb, int N, const uint8_t* stack_in, uint8_t* stack_out,
                          const uint8_t* push_mask, const uint8_t* reset_mask, paac_stream_t stream);

/* Device-resident synthetic environments (the metric's "synthetic 84x84x4 uint8 frames"; spec in
 * paac_amd/synthetic.py, a BaseEnvironment plugin producing the same numbers on the host).
 * One call replaces one Runners.update_environments()/wait_updated() round (runners.py:44-50) plus the
 * per-env bookkeeping of paac.py:119-138 for N envs.  The frame id of the step is
 * *step_base_dev + step_offset + 1 (id 0 is the reset frame):
 *   stack_in -> stack_out (and stack_out2 if non-NULL); auto-reset on terminal like
 *   emulator_runner.py:26-27; rewards_out f32[N] = clipped reward (actor_learner.py:95-101);
 *   masks_out f32[N] = 1 - terminal; ep_reward f32[N] / ep_len i32[N] running episode totals;
 *   finished: {i32 count; i32 pad; f32 reward[4096]; i32 len[4096]} ring of finished episodes.
 * raw_scratch: NULL = path A (one new 84x84 plane per step); else u8 [N,2,210,160] = path B (two raw
 * frames are generated there, then max + resize + stack via the preprocess kernel). */
int paac_synth_reset(uint64_t seed, uint32_t env_offset, int N, uint8_t* stack_out, uint8_t* raw_scratch,
                     paac_stream_t stream);
int paac_synth_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, uint32_t terminal_threshold,
                    const uint64_t* step_base_dev, uint64_t step_offset, const uint8_t* stack_in, uint8_t* stack_out,
                    uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                    void* finished, uint8_t* raw_scratch, paac_stream_t stream);

/* Device-resident catch environments: a learnable game (a ball falls, a paddle moves, +1 for a catch, -1 for a miss) on a
 * 14 x 14 board of 6 x 6 pixel cells, rendered into the same [N,84,84,4] u8 observations; spec in paac_amd/catch.py, a
 * BaseEnvironment plugin producing the same numbers on the host.  3 actions: 0 stay, 1 left, 2 right.
 *   state: i32 [N,8] per environment {bx, by, dx, px, k, 0, 0, 0}; the episode-start hashes are keyed by (seed,
 *          env_offset + e, k).
 * paac_catch_reset: episode 0's start states into state_out, their observations ([0, 0, 0, plane]) into stack_out.
 * paac_catch_step: one step of N environments on actions [N] -- state_in -> state_out, stack_in -> stack_out (history shifted,
 *   the new state's plane pushed; after a terminal step the next episode's start state and an empty history), the records of
 *   paac_synth_step (rewards_out / masks_out [N], ep_reward / ep_len [N] in place, the finished ring, nullable).  One launch.
 *   The step does not run in place: state_in / stack_in must not be state_out / stack_out (refused).  state_out2 / stack_out2
 *   (nullable): second copies of the outputs, like paac_synth_step's stack_out2 (a ring's wrap-around slot). */
int paac_catch_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                     paac_stream_t stream);
int paac_catch_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                    int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                    float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                    paac_stream_t stream);

/* Device-resident bricks environments: a brick-wall game with lives (a ball bounces between a two-cell paddle and three rows
 * of 14 bricks, +1 per brick struck, three lives, at most 500 steps per episode) on the same 14 x 14 board, rendered into the
 * same [N,84,84,4] u8 observations; spec in paac_amd/bricks.py, a BaseEnvironment plugin producing the same numbers on the
 * host.  3 actions: 0 stay, 1 left, 2 right.
 *   state: i32 [N,12] per environment {bx, by, dx, dy, px, lives, steps, k, rows0, rows1, rows2, 0}; the episode-start and
 *          serve hashes are keyed by (seed, env_offset + e, k).  The step trusts its records: they come from
 *          paac_bricks_reset, from an earlier step, or from a caller that writes valid states.
 * paac_bricks_reset / paac_bricks_step: the argument lists, outputs, records and refusals of paac_catch_reset /
 *   paac_catch_step; single_life != 0 makes every lost life end the episode (--single_life_episodes).  One launch. */
int paac_bricks_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                      paac_stream_t stream);
int paac_bricks_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                     int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                     float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished, int single_life,
                     paac_stream_t stream);

/* Device-resident rally environments: a two-paddle game with an opponent (a ball flies between the agent's two-cell paddle in
 * the bottom row and a scripted opponent's in the top row; +1 when the opponent misses, -1 when the agent does, first to five
 * points, at most 1000 steps per episode) on the same 14 x 14 board, rendered into the same [N,84,84,4] u8 observations; spec
 * in paac_amd/rally.py, a BaseEnvironment plugin producing the same numbers on the host.  6 actions, ALE Pong's minimal set:
 * 0 noop, 1 fire (= noop), 2 right, 3 left, 4 rightfire (= right), 5 leftfire (= left).
 *   state: i32 [N,12] per environment {bx, by, dx, dy, px, ox, mine, theirs, steps, k, 0, 0}; the episode-start, serve and
 *          opponent-laziness hashes are keyed by (seed, env_offset + e, k).  The step trusts its records, as bricks' does.
 * paac_rally_reset / paac_rally_step: the argument lists, outputs, records and refusals of paac_catch_reset /
 *   paac_catch_step.  One launch. */
int paac_rally_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                     paac_stream_t stream);
int paac_rally_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                    int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                    float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                    paac_stream_t stream);

/* GPU-resident evaluation of the stateful games (spec: paac_amd/evaluation.py): one evaluation step of N environments in one
 * launch, behind the acting forward that wrote probs [N, A].  With t = *step_base_dev + step_offset (base NULL = 0; a captured
 * block of steps replays with a fresh base, paac_counter_add) and g = env_offset + e:
 *   no-ops   noops_e = word 0 of philox4x32-10(ctr = {g, 0, 0, 0x45560002}; key = eval_seed) % (noops + 1); noops = 0: none
 *   action   t < noops_e: 0 (every game's no-op); else greedy != 0: argmax of probs[e] (lowest index on ties; NaN rows are not
 *            supported), greedy == 0: paac_sample_philox's inverse CDF on u = philox(ctr = {g, t lo, t hi, 0x45560001};
 *            key = eval_seed) -- streams of their own (the rollout sampler's is 0, the minibatch shuffles' 0x504D0000 + epoch);
 *            written to actions_out[e]
 *   game     state_in -> state_out, stack_in -> stack_out exactly as the game's step entry does on that action (seed
 *            env_seed, single_life off); not in place: state_in == state_out or stack_in == stack_out is refused
 *   accounts from t = noops_e on and while done[e] == 0: score[e] += reward, length[e] += 1, and on a terminal step (its
 *            reward included) done[e] = 1 and *alive -= 1 (one atomic per finishing environment).  Rewards and terminals of
 *            the no-op steps are ignored; after done nothing of e changes again (the game itself keeps being stepped).
 *            The caller zeroes score / length / done and sets *alive = N before step 0.
 * The rollout bookkeeping (ep_reward / ep_len / finished ring) is not touched.  Refused with a message, without a launch:
 * the in-place buffers above, N <= 0, A outside [2, 32], noops < 0, a game id that is none of the three. */
/* What one step of the device games records, as one block (paac_game_step): the five records of paac_catch_step, then
 * truncs f32[N] (nullable: nothing is written) = 1 where the step was terminal ONLY because the game's step cap was reached
 * (bricks: steps == 500 and the step did not also lose the last life, or any life under single_life; rally: steps == 1000 and
 * neither side reached five points on the step), else 0.  A step that is both a real ending and at the cap is not truncated;
 * catch never is (13 steps is its rule, not a limit).  rewards / masks keep their meaning: a truncated step is terminal. */
typedef struct {
  float* rewards;
  float* masks;
  float* ep_reward;
  int32_t* ep_len;
  void* finished;
  float* truncs;
} paac_env_records;
/* paac_catch_step / paac_bricks_step / paac_rally_step by the game's id (PAAC_EVAL_CATCH / _BRICKS / _RALLY below), the
 * records as a block; option = bricks' single_life (ignored by the other games).  Same launch, outputs and refusals; with
 * rec->truncs == NULL the same stores. */
int paac_game_step(int game, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                   int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                   const paac_env_records* rec, int option, paac_stream_t stream);
/* Device-resident duel environments: rally played against the learner itself (spec in paac_amd/duel.py).  N rows = N / 2
 * boards of the rally board; row e < N / 2 is the bottom player of board e, row e + N / 2 the top player of the same board,
 * and each row sees the board from its own side: own paddle (128) in the bottom row, the other's (64) in the top row.
 *   state: i32 [N,12], rally's record.  A bottom row holds the board {bx, by, dx, dy, px, ox, mine, theirs, steps, k, 0, 0};
 *          a top row holds its mirror {bx, 13 - by, dx, -dy, ox, px, theirs, mine, steps, k, 0, 0}.  The hashes are keyed by
 *          (seed, env_offset + board, k); the first serve goes towards the bottom player in even episodes, the top player
 *          in odd ones.
 *   step:  row e reads actions[e] AND actions[(e + N / 2) % N]: the board advances by rally's rules with the scripted opponent
 *          replaced by the top player's paddle move (2, 4 = right; 3, 5 = left).  Both rows of a board compute the same board
 *          step; no row writes what another reads.  rewards: the bottom row's is rally's, the top row's 0 - that (+0.0 for
 *          0); masks and rec->truncs (nullable) are the same for both.  Records, outputs and the second outputs as
 *          paac_game_step's.  One launch.
 * Refused with a message, without a launch: N odd or below 2, null actions / state / stack / records pointers, in-place
 * buffers.  There is no evaluation id: a duel policy is scored as a rally agent (PAAC_EVAL_RALLY), or against another policy
 * on the duel board itself by paac_match_step below. */
int paac_duel_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                    paac_stream_t stream);
int paac_duel_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                   int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                   const paac_env_records* rec, paac_stream_t stream);
/* A user's device game (--emulator user --device_game; plugin contract in paac_amd/user_game.py and csrc/game_dev.h): one
 * non-paired game trait from a header outside the package, compiled into a library of its own (-DPAAC_USER_GAME,
 * -DPAAC_USER_GAME_HEADER, -DPAAC_USER_GAME_TRAIT) and run by the same step and evaluation kernels as the built-in games.
 * paac_user_game_info: returns 1 and fills the trait's kWords, kActions and kMaxSteps where a user game is compiled in;
 *   returns 0 (and zeros) in the stock library.
 * paac_user_game_reset: paac_catch_reset's argument list, outputs and refusals, state i32 [N, kWords].
 * paac_user_game_step: paac_duel_step's argument list (the records as one block, rec->truncs nullable) with the game's one
 *   integer option before the stream (0 where the game has none); outputs and refusals as paac_game_step's.  One launch.
 * The game's id for paac_game_step / paac_eval_step is PAAC_EVAL_USER.  In the stock library reset and step fail with a
 * message, without a launch, and PAAC_EVAL_USER is refused as any unknown id is. */
int paac_user_game_info(int* words, int* actions, int* max_steps);
int paac_user_game_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                         paac_stream_t stream);
int paac_user_game_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                        int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                        uint8_t* stack_out2, const paac_env_records* rec, int option, paac_stream_t stream);
#define PAAC_EVAL_CATCH 0
#define PAAC_EVAL_BRICKS 1
#define PAAC_EVAL_RALLY 2
#define PAAC_EVAL_USER 3 /* the user's game: only in a library built with one (paac_user_game_info below) */
int paac_eval_step(int game, const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops,
                   const uint64_t* step_base_dev, uint64_t step_offset, uint64_t env_seed, uint32_t env_offset,
                   const int32_t* state_in, int32_t* state_out, const uint8_t* stack_in, uint8_t* stack_out, int32_t* actions_out,
                   float* score, int32_t* length, int32_t* done, int32_t* alive, paac_stream_t stream);
/* Sticky actions (--sticky_action_p; spec and numpy twin: paac_amd/sticky.py; Machado et al., arXiv 1709.06009): at every
 * step, with probability p, an environment executes the action it EXECUTED on its previous step instead of the chosen one.
 *   draw     u = the 24 high bits of word 0 of philox4x32-10(ctr = {g, t lo, t hi, stream}; key = seed) * 2^-24 as a float32;
 *            the step sticks iff u < p.  g = env_offset + ROW (duel: the two players of a board stick independently),
 *            t = *step_base_dev + step_offset (base NULL = 0).  Training: stream 0x53544B01, seed = the step's `seed`;
 *            evaluation: stream 0x45560004, seed = eval_seed, t = the evaluation step (no-op steps included).  Neither stream
 *            is one in use (0, 0x504D0000 + epoch, 0x45560001..3, 0x44500001, 0x44500003).
 *   executed = sticks ? prev_in[e] : chosen, where chosen = actions[e] (training) or the evaluation's own action; the game
 *            steps on `executed` exactly as the plain entry does on its action.  A duel row also works out its partner's
 *            executed action from actions[partner], prev_in[partner] and the partner's own draw: both rows hold the same pair.
 *   planes   prev_in i32 [N] is read, prev_out[e] (and prev_out2[e] when given: the ring's wrap-around slot) = 0 after a
 *            terminal step, else executed.  A run starts from a zeroed plane: 0 is every game's no-op.
 *   records  everything else -- states, stacks, rewards, masks, truncs, the episode bookkeeping, the evaluation's accounts -- as
 *            the plain entry's on the executed action; `actions` / actions_out keep the CHOSEN action (the agent is not told).
 * p = 0 gives the plain entry's outputs bit for bit.  One launch, the plain entry's grid; no reset form (the plain reset and a
 * zeroed plane).  Refused with a message, without a launch: everything the plain entry refuses, p outside [0, 1) or NaN, a
 * null block, null prev_in / prev_out, prev_in == prev_out or prev_out2.  paac_game_step_sticky serves every PAAC_EVAL_* id,
 * PAAC_EVAL_USER in a library built with a user game (the stock library refuses that id by name, as paac_game_step does). */
typedef struct {
  float p;
  const uint64_t* step_base_dev;
  uint64_t step_offset;
  const int32_t* prev_in;
  int32_t* prev_out;
  int32_t* prev_out2;
} paac_sticky;
int paac_game_step_sticky(int game, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                          int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                          uint8_t* stack_out2, const paac_env_records* rec, int option, const paac_sticky* sticky,
                          paac_stream_t stream);
int paac_duel_step_sticky(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                          int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                          uint8_t* stack_out2, const paac_env_records* rec, const paac_sticky* sticky, paac_stream_t stream);
int paac_eval_step_sticky(int game, const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops,
                          const uint64_t* step_base_dev, uint64_t step_offset, uint64_t env_seed, uint32_t env_offset,
                          const int32_t* state_in, int32_t* state_out, const uint8_t* stack_in, uint8_t* stack_out,
                          int32_t* actions_out, float* score, int32_t* length, int32_t* done, int32_t* alive, float p,
                          const int32_t* prev_in, int32_t* prev_out, paac_stream_t stream);
/* A head-to-head match on the duel board (spec: paac_amd/match.py): one step of N rows = N / 2 boards in one launch, behind the
 * TWO acting forwards that wrote probs [N, 6] -- rows [0, N / 2) by the bottom players' policy, rows [N / 2, N) by the top
 * players'.  paac_eval_step's argument list without `game`; rows, records and the board key g = env_offset + board are
 * paac_duel_step's, reset is paac_duel_reset.  With t = *step_base_dev + step_offset (base NULL = 0):
 *   no-ops   noops_g as paac_eval_step's, keyed by the BOARD: both rows of a board play action 0 while t < noops_g
 *   action   paac_eval_step's two rules on the row's own probs, counter {g, t lo, t hi, stream}, key eval_seed; stream
 *            0x45560001 for a bottom row (its actions are an evaluation's), 0x45560003 for a top row: the two players of a
 *            board never share a random word.  Each row also works out its partner's action from probs[(e + N / 2) % N] by the
 *            same rule on the partner's stream -- both rows of a board hold the same pair.  actions_out[e] = the row's own
 *   game     paac_duel_step's board step on the pair (seed env_seed); not in place
 *   accounts paac_eval_step's, per ROW with the row's own reward: score[b + N / 2] == -score[b], length and done are equal
 *            within a board.  The caller zeroes score / length / done and sets *alive = N (rows) before step 0; each row
 *            takes one off on its own first scored terminal step.
 * Refused with a message naming the argument, without a launch: N odd or below 2, A != 6, noops < 0, a null pointer (all but
 * step_base_dev), state_in == state_out or stack_in == stack_out. */
int paac_match_step(const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops, const uint64_t* step_base_dev,
                    uint64_t step_offset, uint64_t env_seed, uint32_t env_offset, const int32_t* state_in, int32_t* state_out,
                    const uint8_t* stack_in, uint8_t* stack_out, int32_t* actions_out, float* score, int32_t* length,
                    int32_t* done, int32_t* alive, paac_stream_t stream);
/* Duel against a pool of past selves (--duel_pool; spec: paac_amd/duel_pool.py): one training step of N BOARDS in one launch,
 * behind the learner's acting forward and sampler (actions [N]) and a frozen opponent's acting forward (ghost_probs [N, A],
 * A must be 6).  Every learner row is the bottom player of its own board; the top player is a ghost row of the opponent.
 * One pooled step is paac_duel_step on 2N rows with the ghosts as rows [N, 2N): the board key is g = env_offset + b.
 *   state    i32 [N,12]: the board in the bottom player's frame, the only record kept (the ghost's is its mirror)
 *   ghost    always sampled: paac_eval_step's inverse CDF on ghost_probs[b] with u = philox(ctr = {g, t lo, t hi, 0x44500001};
 *            key = sampler_seed), t = *step_base_dev + step_offset (base NULL = 0); written to ghost_actions_out[b] (i32 [N]:
 *            with `actions` it replays the step on the host twin)
 *   learner  stack_in -> stack_out (and stack_out2), state_out (and state_out2), the records of rec (rec->truncs nullable):
 *            what paac_duel_step writes for a bottom row
 *   ghosts   ghost_stack_in -> ghost_stack_out (and ghost_stack_out2, nullable): the plane a top row sees; nothing else
 * paac_duel_ghost_reset: episode 0's start boards and an empty history on both sides -- paac_duel_reset on 2N rows, split.
 * Refused with a message naming the argument, without a launch: N < 1, A != 6, a null pointer (all but step_base_dev, the
 * second outputs, rec->finished and rec->truncs), an input that is one of its outputs, learner and ghost stacks that are the
 * same buffer.  Both are capturable. */
int paac_duel_ghost_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                          uint8_t* ghost_stack_out, paac_stream_t stream);
int paac_duel_ghost_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const float* ghost_probs, int A,
                         uint64_t sampler_seed, const uint64_t* step_base_dev, uint64_t step_offset, const int32_t* state_in,
                         int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                         uint8_t* stack_out2, const uint8_t* ghost_stack_in, uint8_t* ghost_stack_out,
                         uint8_t* ghost_stack_out2, const paac_env_records* rec, int32_t* ghost_actions_out,
                         paac_stream_t stream);

/* paac_sample_mt + paac_synth_step (path A) in ONE launch: workgroup 0 samples (numpy-parity MT19937 stream) and does
 * the per-env bookkeeping while the other workgroups shift the observation stacks (stack_out2, nullable: a second copy
 * of the new stacks, like paac_synth_step's).  Limit: N*(A-1) <= 2304 (covers 256 environments x 4 actions and
 * 128 x 18).
 * walk_scratch (nullable): device memory of paac_walk_scratch_bytes(N, A) bytes, ZERO-INITIALISED once by the caller, then
 * left to the library and lent to every call of the same (N, A) in one stream order.  With it the large shards (more than
 * 64 environments or 1024 draws) spread the sampler's walk over several workgroups of the launch (same actions, same
 * stream position; 49 -> 14 us at 256 environments x 4 actions, 41 -> 24 us at 128 x 18); without it one workgroup walks
 * all environments.
 * raw_scratch (nullable, [N,2,210,160] u8): path B -- the launch's other workgroups write the step's raw screen pairs there
 * instead of shifting, and the preprocess launch (max, PIL-nearest resize, history push) follows, like paac_synth_step's. */
#define PAAC_FUSED_SAMPLE_MAX_DRAWS 2304
int64_t paac_walk_scratch_bytes(int N, int A);
int paac_sample_mt_synth_step(const float* probs, int A, uint32_t* mt_state, int32_t* actions, uint64_t seed,
                              uint32_t env_offset, int N, uint32_t terminal_threshold, const uint64_t* step_base_dev,
                              uint64_t step_offset, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                              float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                              void* walk_scratch, int64_t walk_scratch_bytes, uint8_t* raw_scratch, paac_stream_t stream);

/* hipGraph helpers: capture every launch issued on `stream` between begin/end, replay with launch. */
int paac_graph_begin(paac_stream_t stream);
int paac_graph_end(paac_stream_t stream, paac_graph** out);
int paac_graph_launch(paac_graph* g, paac_stream_t stream);
int paac_graph_destroy(paac_graph* g);

/* Test/debug: copy an internal activation to a caller device buffer (async on stream).
 * what: 1..3 = conv outputs a1..a3 [batch,OH,OW,C], 4 = fc activations h [batch,H] of the activation set used
 * last (acting or training); 21..23 / 24 = the same of the TRAINING set explicitly (rows kept by paac_keep_next_forward);
 * 11..13 / 14 = the gradients wrt them; 25 = the value head's outputs [batch] of the TRAINING set (after an update whose
 * returns took the bootstrap values from the training forward, rows [T*N, T*N + N) are those values); 26 = the policy
 * head's probabilities [batch, A] of the TRAINING set (what p_old is recorded from; needs the ctx for A, so
 * paac_debug_activation_size does not know it).  out_capacity: floats `out` holds; a copy larger than that is refused (nothing is
 * written).  Returns the element count. */
int64_t paac_debug_activation(paac_ctx* ctx, int what, int batch, float* out, int64_t out_capacity, paac_stream_t stream);
/* Test/debug: the element count paac_debug_activation copies for (what, batch) on geometry `arch` of this library (host
 * only, no device or ctx needed); -1 for a `what` the geometry does not have. */
int64_t paac_debug_activation_size(int arch, int what, int batch);

/* Test/debug: sampler workgroup `sampler_workgroup` of paac_act_step_mt's large-shard step launch reports an exactly-zero
 * conditional probability it has not seen (-1: off, the default) -- exercises the rare serial path of the distributed zero
 * detection on ordinary probabilities.  Process-wide; synchronises the device. */
int paac_debug_report_zero(int sampler_workgroup);

/* Tuning (tools/tune_gemm.py): override the launch configuration of GEMM op `op` (0 conv1_fwd, 1 conv2_fwd,
 * 2 conv3_fwd, 3 fc_fwd, 4 fc_wgrad, 5 fc_dgrad, 6 conv3_wgrad, 7 conv3_dgrad, 8 conv2_wgrad, 9 conv2_dgrad,
 * 10 conv1_wgrad, 11 conv tower: cfg = regions per sample, 1 / 2 / 4, -1 = by batch) for batch class 0 (batch <= 64), 1 (batch <= 512) or 2: cfg = index into the family's configuration table
 * (-1 = size heuristic), ksplit = blockIdx.z K split (0 = heuristic), xcd_dim = grid dimension tied to the XCD. */
int paac_debug_set_tuning(paac_ctx* ctx, int op, int batch_class, int cfg, int ksplit, int xcd_dim);
int paac_debug_get_tuning(paac_ctx* ctx, int op, int batch_class, int* cfg, int* ksplit, int* xcd_dim);
/* Which configuration ids the launchers have (no ctx, no device).  paac_debug_cfg_known: 1 when `cfg` is an id op `op` runs --
 * an entry of its family's table on the plain path, + 100 on the exact-bf16 path (conv1 only), + 200 on the split-bf16
 * path, + 300 with narrow tiles (forward), an id whose path does not instantiate the entry counting as its plain form; any
 * cfg < 0 (the size heuristic); for op 11 any value (region counts the tower does not have mean "by batch") -- else 0.
 * paac_debug_set_tuning and PAAC_TUNE_OVERRIDE refuse an id that is not known, and a launcher handed one fails its call.
 * paac_debug_cfg_body: the id of the table entry that runs for `cfg` (cfg itself where its path instantiates it, its plain
 * form where the launchers fall back), -1 for the heuristic / automatic choice, -2 for an id that is not known. */
int paac_debug_cfg_known(int op, int cfg);
int paac_debug_cfg_body(int op, int cfg);

/* The user architecture compiled into this library: returns 1 and fills nconv (2 or 3), filters3[3] (0 for an absent third
 * layer) and fc_width; returns 0 (and zeros) for the stock library. */
int paac_user_arch(int32_t* nconv, int32_t* filters3, int32_t* fc_width);
/* ... and its layers' kernel sizes and strides (VALID convolutions, networks.py:12-21; 0 for an absent layer). */
int paac_user_arch_layers(int32_t* sizes3, int32_t* strides3);

/* Diagnostic: writes {s_memtime shader-clock ticks, s_memrealtime 100 MHz ticks} to out2_dev[0..1]. */
int paac_debug_clock(uint64_t* out2_dev, paac_stream_t stream);

/* Per-kernel timing hooks for bench.py's roofline object: when enabled, every network / optimizer kernel
 * launch is bracketed by hipEvents on the launch stream (do not enable inside graph capture).
 * paac_prof_read synchronises the recorded events and returns, per launch, its kernel family, the batch it
 * processed and its duration in ms (up to max_events; the internal table holds 8192 launches); returns the
 * number of records written and clears the table.  The entry points that take no ctx (environment step, samplers,
 * n-step returns, preprocessing) are recorded in the table of the ctx profiling was last enabled on.
 * paac_prof_read_mix (call it BEFORE paac_prof_read, which clears the table; no synchronisation) returns per launch the
 * instruction mix of its contraction bodies, one byte per body in launch order: MFMA products issued per fp32 multiply
 * (1 = fp32 MFMA, 3 = exact-bf16 path, 6 = split-bf16 path; 0 = no contraction) -- so that a family is priced against the
 * ceiling of what it ran. */
#define PAAC_PROF_FAMILIES 26
int paac_prof_enable(paac_ctx* ctx, int on);
int paac_prof_read_mix(paac_ctx* ctx, int32_t* mix_out, int max_events);
int paac_prof_read(paac_ctx* ctx, int32_t* family_out, int32_t* batch_out, float* ms_out, int max_events);
const char* paac_prof_name(int family);

#ifdef __cplusplus
}
#endif
#endif /* PAAC_HIP_H */
