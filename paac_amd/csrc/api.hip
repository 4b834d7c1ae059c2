// C-ABI: context, parameter layout, forward/backward entry points, hipGraph helpers, timing hooks.
#include <stdarg.h>
#include <stdlib.h>

#include <new>

#include "common.h"
#include "synth_dev.h"

namespace paac {

static thread_local char g_err[512] = "";
thread_local ProfEvents g_prof = {nullptr, nullptr, 0, 0};
paac_ctx* g_prof_ctx = nullptr;

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

ArchSpec arch_spec(int arch) {
  ArchSpec s;
  memset(&s, 0, sizeof(s));
  if (arch == PAAC_ARCH_NATURE) {
    s.nconv = 3;
    s.conv[0] = ConvSpec{84, 84, 4, 20, 20, 32, 8, 4};
    s.conv[1] = ConvSpec{20, 20, 32, 9, 9, 64, 4, 2};
    s.conv[2] = ConvSpec{9, 9, 64, 7, 7, 64, 3, 1};
    s.flat = 3136;
    s.fc = 512;
#ifdef PAAC_USER_ARCH
  } else if (arch == PAAC_ARCH_USER) {
    // layer shapes from the build's -DPAAC_USER_* flags, like UserNet (net_common.h): VALID convolutions over 84 x 84 x 4
#ifndef PAAC_USER_K1
#define PAAC_USER_K1 8
#define PAAC_USER_S1 4
#define PAAC_USER_K2 4
#define PAAC_USER_S2 2
#define PAAC_USER_K3 3
#define PAAC_USER_S3 1
#endif
    constexpr int o1 = (84 - PAAC_USER_K1) / PAAC_USER_S1 + 1, o2 = (o1 - PAAC_USER_K2) / PAAC_USER_S2 + 1;
    constexpr int o3 = PAAC_USER_NCONV == 3 ? (o2 - PAAC_USER_K3) / PAAC_USER_S3 + 1 : o2;
    s.nconv = PAAC_USER_NCONV;
    s.conv[0] = ConvSpec{84, 84, 4, o1, o1, PAAC_USER_C1, PAAC_USER_K1, PAAC_USER_S1};
    s.conv[1] = ConvSpec{o1, o1, PAAC_USER_C1, o2, o2, PAAC_USER_C2, PAAC_USER_K2, PAAC_USER_S2};
    if (PAAC_USER_NCONV == 3) s.conv[2] = ConvSpec{o2, o2, PAAC_USER_C2, o3, o3, PAAC_USER_C3, PAAC_USER_K3, PAAC_USER_S3};
    s.flat = PAAC_USER_NCONV == 3 ? o3 * o3 * PAAC_USER_C3 : o2 * o2 * PAAC_USER_C2;
    s.fc = PAAC_USER_H;
#endif
  } else {
    s.nconv = 2;
    s.conv[0] = ConvSpec{84, 84, 4, 20, 20, 16, 8, 4};
    s.conv[1] = ConvSpec{20, 20, 16, 9, 9, 32, 4, 2};
    s.flat = 2592;
    s.fc = 256;
  }
  return s;
}

// which of the library's two compiled geometries besides Nature: the reference's NIPS trunk, or a user architecture
bool arch_supported(int arch) {
#ifdef PAAC_USER_ARCH
  return arch == PAAC_ARCH_NATURE || arch == PAAC_ARCH_USER;
#else
  return arch == PAAC_ARCH_NATURE || arch == PAAC_ARCH_NIPS;
#endif
}

int64_t wslab_floats_needed(int arch);
size_t tower_pack_bytes();
void default_tuning(paac_ctx* c);
int cfg_body(int op, int cfg);      // net_bwd.hip: -2 = an id the launchers refuse
int fc_splits_max();

static const char* kFamilyNames[PAAC_PROF_FAMILIES] = {
    "conv1_fwd", "conv2_fwd", "conv3_fwd", "fc_fwd", "heads_fwd", "heads_bwd", "fc_wgrad", "fc_dgrad",
    "conv3_wgrad", "conv3_dgrad", "conv2_wgrad", "conv2_dgrad", "conv1_wgrad", "grad_finalize", "clip_rmsprop", "misc",
    "env_step", "sample_env_step", "sample_mt", "sample_philox", "nstep_returns", "preprocess_stack", "conv_tower",
    "fc_conv3_wgrad", "conv2_conv1_wgrad", "dgrad_tower"};

}  // namespace paac

using namespace paac;

// The entries that read what an acting step's sampler writes (actions, values, rewards, masks) refuse to run while the last
// paac_act_step_pipe's sample is still owed.
#define PAAC_NO_PENDING_SAMPLE(ctx, fn)                                                                                  \
  PAAC_REQUIRE(!(ctx)->act_owed->partial, "%s: the last paac_act_step_pipe's sample is still pending (that step's actions, "  \
               "values and records are not written yet): pay it with paac_bootstrap_forward_trunk, another "                \
               "paac_act_step_pipe or paac_act_step_flush first", fn)

struct paac_graph {
  hipGraph_t graph;
  hipGraphExec_t exec;
};

extern "C" {

const char* paac_last_error(void) { return g_err; }
int paac_version(void) { return 100; }

int paac_param_layout(int arch, int num_actions, paac_layout* out) {
  PAAC_REQUIRE(out, "paac_param_layout: null out");
  PAAC_REQUIRE(arch_supported(arch), "paac_param_layout: arch %d is not compiled into this library (a library holds Nature "
               "and either the NIPS geometry or one user architecture, paac_user_arch)", arch);
  PAAC_REQUIRE(num_actions >= 2 && num_actions <= 32, "paac_param_layout: num_actions %d not in [2,32]", num_actions);
  memset(out, 0, sizeof(*out));
  const ArchSpec s = arch_spec(arch);
  int t = 0;
  int64_t off = 0, unp = 0;
  auto add = [&](const char* name, int rank, int d0, int d1, int d2, int d3) {
    int64_t size = (int64_t)d0 * (rank > 1 ? d1 : 1) * (rank > 2 ? d2 : 1) * (rank > 3 ? d3 : 1);
    snprintf(out->name[t], sizeof(out->name[t]), "%s", name);
    out->rank[t] = rank;
    out->shape[t][0] = d0; out->shape[t][1] = rank > 1 ? d1 : 0;
    out->shape[t][2] = rank > 2 ? d2 : 0; out->shape[t][3] = rank > 3 ? d3 : 0;
    out->offset[t] = off;
    out->size[t] = size;
    off += (size + 3) / 4 * 4;
    unp += size;
    ++t;
  };
  char nm[32];
  for (int i = 0; i < s.nconv; ++i) {
    snprintf(nm, sizeof(nm), "conv%d_weights", i + 1);
    add(nm, 4, s.conv[i].k, s.conv[i].k, s.conv[i].cin, s.conv[i].cout);
    snprintf(nm, sizeof(nm), "conv%d_biases", i + 1);
    add(nm, 1, s.conv[i].cout, 0, 0, 0);
  }
  snprintf(nm, sizeof(nm), "fc%d_weights", s.nconv + 1);
  add(nm, 2, s.flat, s.fc, 0, 0);
  snprintf(nm, sizeof(nm), "fc%d_biases", s.nconv + 1);
  add(nm, 1, s.fc, 0, 0, 0);
  add("actor_output_weights", 2, s.fc, num_actions, 0, 0);
  add("actor_output_biases", 1, num_actions, 0, 0, 0);
  add("critic_output_weights", 2, s.fc, 1, 0, 0);
  add("critic_output_biases", 1, 1, 0, 0, 0);
  out->num_tensors = t;
  out->total = off;
  out->total_unpadded = unp;
  return 0;
}

int paac_create(const paac_cfg* cfg, paac_ctx** out) {
  PAAC_REQUIRE(cfg && out, "paac_create: null argument");
  PAAC_REQUIRE(cfg->max_batch > 0, "paac_create: max_batch %d", cfg->max_batch);
  int ndev = 0;
  PAAC_CHECK_HIP(hipGetDeviceCount(&ndev));
  PAAC_REQUIRE(ndev > 0, "paac_create: no HIP device visible (this library is MI355X-only; there is no CPU path)");
  PAAC_REQUIRE(cfg->device >= 0 && cfg->device < ndev, "paac_create: device %d of %d", cfg->device, ndev);
  PAAC_CHECK_HIP(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  PAAC_CHECK_HIP(hipGetDeviceProperties(&prop, cfg->device));
  PAAC_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
               "paac_create: device %d is %s; libpaac_hip is built for gfx950 (MI355X) only", cfg->device,
               prop.gcnArchName);
  paac_ctx* c = new (std::nothrow) paac_ctx;
  PAAC_REQUIRE(c, "paac_create: out of host memory");
  memset(c, 0, sizeof(*c));
  c->cfg = *cfg;
  if (paac_param_layout(cfg->arch, cfg->num_actions, &c->layout) != 0) {
    delete c;
    return -1;
  }
  c->spec = arch_spec(cfg->arch);
  c->max_batch = cfg->max_batch;
  for (int o = 0; o < OP_COUNT; ++o)
    for (int k = 0; k < 3; ++k) c->tune[o][k] = Tune{-1, 0, -1};
  default_tuning(c);
  // diagnostic: PAAC_TUNE_OVERRIDE="op:class:cfg:ksplit:xcd[,...]" replaces entries of the table (the numbering of
  // paac_debug_set_tuning), so that a whole bench.py run can be taken with another launch configuration
  if (const char* ov = getenv("PAAC_TUNE_OVERRIDE")) {
    int op, cls, cf, ks, xc, used = 0;
    // every entry is applied or refused: an unreadable entry, an op / class outside the table or a configuration id the
    // launchers do not have fails the creation (a typo must not time a run with another configuration -- or none)
    while (*ov) {
      const bool read = sscanf(ov, "%d:%d:%d:%d:%d%n", &op, &cls, &cf, &ks, &xc, &used) == 5;
      const bool ends = read && (ov[used] == ',' || ov[used] == 0);
      if (!ends || op < 0 || op >= OP_COUNT || cls < 0 || cls > 2 || cfg_body(op, cf) < -1) {
        char entry[48];
        size_t n = strcspn(ov, ",");
        if (n >= sizeof(entry)) n = sizeof(entry) - 1;
        memcpy(entry, ov, n);
        entry[n] = 0;
        if (!ends) set_error("paac_create: PAAC_TUNE_OVERRIDE entry \"%s\" is not op:class:cfg:ksplit:xcd", entry);
        else if (op < 0 || op >= OP_COUNT || cls < 0 || cls > 2)
          set_error("paac_create: PAAC_TUNE_OVERRIDE entry \"%s\": op %d / class %d outside the table (ops 0..%d, classes 0..2)",
                    entry, op, cls, OP_COUNT - 1);
        else set_error("paac_create: PAAC_TUNE_OVERRIDE entry \"%s\": op %d has no configuration id %d", entry, op, cf);
        delete c;
        return -1;
      }
      c->tune[op][cls] = Tune{cf, ks, xc};
      ov += used;
      if (*ov == ',') ++ov;
    }
  }
  const int64_t B = cfg->max_batch;
  const int A = cfg->num_actions;
  c->fc_splits_max = fc_splits_max();
  for (int w = 0; w < 2; ++w) {
    Workspace& W = c->ws[w];
    for (int i = 0; i < c->spec.nconv; ++i) {
      const ConvSpec& cs = c->spec.conv[i];
      // rows rounded up to 16: the packed conv3 -> fc hand-off (tower.h / fc_heads.h) addresses whole 16-row tiles
      PAAC_CHECK_HIP(hipMalloc(&W.act[i], (size_t)((B + 15) / 16 * 16) * cs.oh * cs.ow * cs.cout * sizeof(float)));
    }
    PAAC_CHECK_HIP(hipMalloc(&W.fc_slab, (size_t)c->fc_splits_max * B * c->spec.fc * sizeof(float)));
    PAAC_CHECK_HIP(hipMalloc(&W.h, (size_t)B * c->spec.fc * sizeof(float)));
    PAAC_CHECK_HIP(hipMalloc(&W.probs, (size_t)B * A * sizeof(float)));
    PAAC_CHECK_HIP(hipMalloc(&W.logits, (size_t)B * A * sizeof(float)));
    PAAC_CHECK_HIP(hipMalloc(&W.values, (size_t)B * sizeof(float)));
  }
  for (int i = 0; i < c->spec.nconv; ++i) {
    const ConvSpec& cs = c->spec.conv[i];
    PAAC_CHECK_HIP(hipMalloc(&c->dact[i], (size_t)B * cs.oh * cs.ow * cs.cout * sizeof(float)));
  }
  PAAC_CHECK_HIP(hipMalloc(&c->dh, (size_t)B * c->spec.fc * sizeof(float)));
  if (paac::dh_planes_supported(c->spec.fc)) {
    PAAC_CHECK_HIP(hipMalloc(&c->dh_planes, paac::dh_planes_bytes((int)B, c->spec.fc)));
    PAAC_CHECK_HIP(hipMemset(c->dh_planes, 0, paac::dh_planes_bytes((int)B, c->spec.fc)));
  }
  { const char* v = getenv("PAAC_FC_DGRAD_ONCE"); c->fc_dgrad_once = !(v && *v && atoi(v) == 0); }
  PAAC_CHECK_HIP(hipMalloc(&c->dl_buf, (size_t)B * paac::kDlStride * sizeof(float)));
  PAAC_CHECK_HIP(hipMalloc(&c->ppo_rows, (size_t)B * 2 * sizeof(float)));
  PAAC_CHECK_HIP(hipMalloc(&c->vclip_rows, (size_t)B * sizeof(float)));
  c->wslab_floats = wslab_floats_needed(cfg->arch);
  PAAC_CHECK_HIP(hipMalloc(&c->wslab, (size_t)c->wslab_floats * sizeof(float)));
  PAAC_CHECK_HIP(hipMalloc(&c->partials, 8192 * sizeof(float)));
  PAAC_CHECK_HIP(hipMemset(c->partials, 0, 8192 * sizeof(float)));
  PAAC_CHECK_HIP(hipMalloc(&c->zeros, (size_t)(c->spec.fc > 1024 ? c->spec.fc : 1024) * sizeof(float)));
  PAAC_CHECK_HIP(hipMemset(c->zeros, 0, (size_t)(c->spec.fc > 1024 ? c->spec.fc : 1024) * sizeof(float)));
  c->keep_row = -1;
  c->heads_pending_h = 0;
  PAAC_CHECK_HIP(hipMalloc(&c->mt_ahead, mt_ahead_bytes()));
  PAAC_CHECK_HIP(hipMemset(c->mt_ahead, 0, mt_ahead_bytes()));
  c->act_owed = new (std::nothrow) ActSample{};
  PAAC_REQUIRE(c->act_owed, "paac_create: out of host memory");
  c->act_region = 0;
  { const char* v = getenv("PAAC_ACT_TOWER_RIDER"); c->act_tower_rider = (v && *v) ? atoi(v) : 1; }
  PAAC_REQUIRE(c->act_tower_rider >= 0 && c->act_tower_rider <= 2, "paac_create: PAAC_ACT_TOWER_RIDER=%d (0, 1 or 2)",
               c->act_tower_rider);
  PAAC_CHECK_HIP(hipMalloc(&c->act_fin_rec, sizeof(ActFinishRecord)));
  PAAC_CHECK_HIP(hipMemset(c->act_fin_rec, 0, sizeof(ActFinishRecord)));
  {
    const char* v = getenv("PAAC_TOWER");
    c->tower_on = (cfg->arch == PAAC_ARCH_NATURE) && !(v && *v && atoi(v) == 0);
    { const char* q = getenv("PAAC_FC_QUARTER"); c->no_quarter_tiles = (q && *q && atoi(q) == 0) ? 1 : 0; }
    c->tower2_on = (cfg->arch == PAAC_ARCH_NIPS) && tower2_available() && !(v && *v && atoi(v) == 0);
    c->managed_weights = 0;
    c->tower_pack = nullptr;
    if (c->tower_on || c->tower2_on) PAAC_CHECK_HIP(hipMalloc(&c->tower_pack, tower_pack_bytes()));
    PAAC_CHECK_HIP(hipMalloc(&c->fc_pack, (size_t)c->spec.flat * c->spec.fc * sizeof(float)));
  }
  c->ev_start = new hipEvent_t[paac_ctx::PROF_MAX_EVENTS];
  c->ev_stop = new hipEvent_t[paac_ctx::PROF_MAX_EVENTS];
  c->ev_family = new int[paac_ctx::PROF_MAX_EVENTS];
  c->ev_batch = new int[paac_ctx::PROF_MAX_EVENTS];
  c->ev_mix = new int[paac_ctx::PROF_MAX_EVENTS];
  c->ev_count = 0;
  c->prof_on = 0;
  for (int i = 0; i < paac_ctx::PROF_MAX_EVENTS; ++i) {
    c->ev_start[i] = nullptr;
    c->ev_stop[i] = nullptr;
  }
  *out = c;
  return 0;
}

int paac_destroy(paac_ctx* c) {
  if (!c) return 0;
  for (int w = 0; w < 2; ++w) {
    Workspace& W = c->ws[w];
    for (int i = 0; i < 3; ++i)
      if (W.act[i]) (void)hipFree(W.act[i]);
    float* bufs[] = {W.fc_slab, W.h, W.probs, W.logits, W.values};
    for (float* b : bufs)
      if (b) (void)hipFree(b);
  }
  for (int i = 0; i < 3; ++i)
    if (c->dact[i]) (void)hipFree(c->dact[i]);
  float* bufs[] = {c->dh, c->wslab, c->partials, c->dl_buf, c->zeros, c->ppo_rows, c->vclip_rows};
  for (float* b : bufs)
    if (b) (void)hipFree(b);
  if (c->mt_ahead) (void)hipFree(c->mt_ahead);
  if (c->act_fin_rec) (void)hipFree(c->act_fin_rec);
  if (c->dh_planes) (void)hipFree(c->dh_planes);
  if (c->tower_pack) (void)hipFree(c->tower_pack);
  if (c->fc_pack) (void)hipFree(c->fc_pack);
  for (int i = 0; i < paac_ctx::PROF_MAX_EVENTS; ++i) {
    if (c->ev_start[i]) (void)hipEventDestroy(c->ev_start[i]);
    if (c->ev_stop[i]) (void)hipEventDestroy(c->ev_stop[i]);
  }
  delete[] c->ev_start;
  delete[] c->ev_stop;
  delete[] c->ev_family;
  delete[] c->ev_batch;
  delete[] c->ev_mix;
  delete c->act_owed;
  delete c;
  return 0;
}

// The tail of the forward and acting entries: the status of the entry's last launcher, then what HIP has recorded meanwhile.
static int launched(int rc) {
  if (rc) return rc;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// The head partials a kHeadsDefer forward left, as the launch that finishes the heads takes them.
static HeadsPartials partials_of(const paac_ctx* ctx, const float* params, const ForwardCall& call, float* values_out) {
  const paac_layout& L = ctx->layout;
  const int nt = L.num_tensors;
  return HeadsPartials{call.partial, call.ntiles, params + L.offset[nt - 3], params + L.offset[nt - 1], values_out};
}

int paac_forward(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* logits, float* probs,
                 float* values, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states, "paac_forward: null argument");
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "paac_forward: batch %d outside (0, max_batch=%d]", batch,
               ctx->max_batch);
  ForwardCall call{.ws = 0, .logits = logits, .probs = probs, .values = values};
  return launched(launch_forward(ctx, params, states, batch, call, (hipStream_t)stream));
}

int paac_pack_weights(paac_ctx* ctx, const float* params, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params, "paac_pack_weights: null argument");
  const int rc = launch_pack_weights(ctx, params, (hipStream_t)stream);
  if (rc) return rc;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_set_managed_weights(paac_ctx* ctx, int on) {
  PAAC_REQUIRE(ctx, "paac_set_managed_weights: null ctx");
  ctx->managed_weights = on ? 1 : 0;
  return 0;
}

int paac_train_forward(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* values,
                       paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states, "paac_train_forward: null argument");
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "paac_train_forward: batch %d outside (0, max_batch=%d]", batch,
               ctx->max_batch);
  ForwardCall call{.ws = 1, .values = values};
  return launched(launch_forward(ctx, params, states, batch, call, (hipStream_t)stream));
}

int paac_train_forward_trunk(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states, "paac_train_forward_trunk: null argument");
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "paac_train_forward_trunk: batch %d outside (0, max_batch=%d]", batch,
               ctx->max_batch);
  ForwardCall call{.ws = 1, .heads = kHeadsTrunkOnly};
  return launched(launch_forward(ctx, params, states, batch, call, (hipStream_t)stream));
}

int paac_keep_next_forward(paac_ctx* ctx, int train_row) {
  PAAC_REQUIRE(ctx, "paac_keep_next_forward: null ctx");
  PAAC_REQUIRE(train_row >= -1 && train_row < ctx->max_batch, "paac_keep_next_forward: row %d outside [-1, max_batch=%d)",
               train_row, ctx->max_batch);
  ctx->keep_row = train_row;
  return 0;
}

// What the conv tower launch of an acting forward is offered to carry (csrc/tower.h: RIDER; the forward settles what it does
// carry): the heads finish of the owed sample, at the limits of heads_finish_fused, and -- step: the forward's own environment
// step -- its frame shift, where the stacks written are not the ones the tower reads.
static TowerRider tower_rider_of(const paac_ctx* ctx, const ActSample& owed, const SynthStep* step) {
  TowerRider tr{};
  if (ctx->act_tower_rider >= 1 && owed.partial && owed.N <= kActFinMaxN && owed.A <= kActFinMaxA && owed.ntiles <= kActFinMaxTiles)
    tr.fin = ActFinish{owed.partial, owed.ntiles, owed.ba, owed.bc, owed.probs_out, owed.values_out, owed.A, owed.N,
                       ctx->act_fin_rec};
  if (ctx->act_tower_rider >= 2 && step && step->stack_out != step->stack_in && step->stack_out2 != step->stack_in) tr.shift = *step;
  return tr;
}

int paac_act_tower_rode(const paac_ctx* ctx) { return ctx ? ctx->act_tower_rode : 0; }

int paac_act_finish_layout(int64_t* out, int n) {
  PAAC_REQUIRE(out && n >= 8, "paac_act_finish_layout: eight words");
  const int64_t v[8] = {(int64_t)sizeof(ActFinishRecord), (int64_t)offsetof(ActFinishRecord, pj), (int64_t)offsetof(ActFinishRecord, thr),
                        (int64_t)offsetof(ActFinishRecord, probs), (int64_t)offsetof(ActFinishRecord, any_zero), kActFinMaxN,
                        kActFinMaxA, kActFinMaxTiles};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return 0;
}

int paac_bootstrap_forward_trunk(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, int train_row,
                                 paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states, "paac_bootstrap_forward_trunk: null argument");
  PAAC_REQUIRE(batch > 0 && train_row >= 0 && train_row + batch <= ctx->max_batch,
               "paac_bootstrap_forward_trunk: rows [%d, %d) outside max_batch=%d", train_row, train_row + batch, ctx->max_batch);
  // a pipelined acting step's sample is owed: this forward's fc launch carries it (no frame shift: nothing steps here)
  ActRider rider{};
  rider.owed = *ctx->act_owed;
  if (rider.owed.partial) {
    PAAC_REQUIRE(batch <= PAAC_ACT_STEP_MAX_ENVS && forward_has_fc_heads(ctx) &&
                 (size_t)(ctx->spec.fc / 8) * batch * (ctx->cfg.num_actions + 1) <= act_region_floats(ctx),
                 "paac_bootstrap_forward_trunk: a forward of %d rows cannot carry the pending sample of paac_act_step_pipe "
                 "(paac_act_step_flush pays it)", batch);
  }
  // Acting-shaped forward of the N bootstrap observations whose rows complete a training set the acting steps have kept
  // (paac_keep_next_forward): conv tower + fc, rows kept at [train_row, train_row + batch) -- of the bootstrap rows the update
  // reads the fc activations only, the backward covers the rollout rows; no heads -- the backward's first launch takes the
  // bootstrap values from the kept fc activations like it does after a trunk-only training forward.
  const TowerRider trider = tower_rider_of(ctx, rider.owed, nullptr);      // (the heads finish of step T - 1 rides its tower)
  ForwardCall call{.ws = 0, .heads = kHeadsDefer, .keep_row = train_row, .keep_h_only = true,
                   .rider = rider.owed.partial ? &rider : nullptr, .tower_rider = &trider};
  const int rc = launch_forward(ctx, params, states, batch, call, (hipStream_t)stream);
  if (call.rode) ctx->act_owed->partial = nullptr;
  if (rc) return rc;
  ctx->heads_pending_rows = train_row + batch;
  ctx->heads_pending_splits = 1;
  ctx->heads_pending_h = 1;
  return launched(0);
}

int paac_forward_sample(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* probs,
                        float* values, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                        uint32_t env_offset, int32_t* actions, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states && actions, "paac_forward_sample: null argument");
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "paac_forward_sample: batch %d outside (0, max_batch=%d]", batch,
               ctx->max_batch);
  return launched(launch_forward_sample(ctx, params, states, batch, probs, values, seed, step_base_dev, step_offset, env_offset,
                                        actions, nullptr, (hipStream_t)stream));
}

int paac_forward_sample_synth_step(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, float* probs,
                                   float* values, uint64_t seed, const uint64_t* step_base_dev, uint64_t step_offset,
                                   uint32_t env_offset, int32_t* actions, uint64_t env_seed, uint32_t terminal_threshold,
                                   uint8_t* stack_out, float* rewards_out, float* masks_out, float* ep_reward,
                                   int32_t* ep_len, void* finished, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states && actions, "paac_forward_sample_synth_step: null argument");
  SynthStep st;          // (the heads launch takes env_offset and the step id from the sampler's arguments, which are the step's)
  if (synth_step_of("paac_forward_sample_synth_step", "null argument", false, &st, env_seed, env_offset, batch, terminal_threshold,
                    step_base_dev, step_offset, states, stack_out, nullptr, rewards_out, masks_out, ep_reward, ep_len, finished,
                    nullptr))
    return -1;
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "paac_forward_sample_synth_step: batch %d outside (0, max_batch=%d]",
               batch, ctx->max_batch);
  return launched(launch_forward_sample(ctx, params, states, batch, probs, values, seed, step_base_dev, step_offset, env_offset,
                                        actions, &st, (hipStream_t)stream));
}

int paac_act_step_mt(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, uint32_t* mt_state,
                     int32_t* actions, float* probs_out, float* values_out, uint64_t env_seed, uint32_t env_offset,
                     uint32_t terminal_threshold, const uint64_t* step_base_dev, uint64_t step_offset, uint8_t* stack_out,
                     uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                     void* finished, uint8_t* raw_scratch, void* walk_scratch, int64_t walk_scratch_bytes,
                     paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states && mt_state && actions && probs_out && values_out, "paac_act_step_mt: null argument");
  // the acting forward that finishes its heads into the caller's arrays, and the one that leaves the fc kernel's head partials
  // for the sampler launch to finish (partials_of)
  const ForwardCall finish{.ws = 0, .probs = probs_out, .values = values_out}, defer{.ws = 0, .heads = kHeadsDefer};
  const hipStream_t s = (hipStream_t)stream;
  if (stack_out == nullptr) {
    // policy forward + sampler only (the environments live on the host: paac.py:104-110 without :115-116): three launches up
    // to PAAC_ACT_STEP_MAX_ENVS environments, paac_forward + paac_sample_mt beyond
    PAAC_REQUIRE(!stack_out2 && !raw_scratch, "paac_act_step_mt: no environment step (stack_out == NULL) takes no stack_out2 / "
                 "raw_scratch");
    PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch && batch <= PAAC_ACT_STEP_MAX_ENVS &&
                 (int64_t)batch * (ctx->cfg.num_actions - 1) <= 1024,
                 "paac_act_step_mt: sampling without an environment step covers up to %d environments and 1024 draws (use "
                 "paac_forward + paac_sample_mt); got %d x %d actions", PAAC_ACT_STEP_MAX_ENVS, batch, ctx->cfg.num_actions);
    if (!forward_has_fc_heads(ctx)) {
      // no head partials on this geometry: the plain forward finishes the heads, the sampler reads its probabilities
      ForwardCall call = finish;
      if (const int rc = launch_forward(ctx, params, states, batch, call, s)) return rc;
      return launched(launch_sample_mt_probs(probs_out, ctx->cfg.num_actions, mt_state, actions, batch, s));
    }
    SynthStep none{};            // no environment step: heads finish + sampler over `batch` rows
    none.N = batch;
    ForwardCall call = defer;
    if (const int rc = launch_forward(ctx, params, states, batch, call, s)) return rc;
    return launched(launch_sample_env_step_heads(partials_of(ctx, params, call, values_out), probs_out, ctx->cfg.num_actions,
                                                 mt_state, actions, none, nullptr, s));
  }
  SynthStep st;
  if (synth_step_of("paac_act_step_mt", "null argument", false, &st, env_seed, env_offset, batch, terminal_threshold, step_base_dev,
                    step_offset, states, stack_out, stack_out2, rewards_out, masks_out, ep_reward, ep_len, finished, raw_scratch))
    return -1;
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch && batch <= PAAC_ACT_STEP_MAX_ENVS_LARGE,
               "paac_act_step_mt: batch %d outside (0, min(max_batch=%d, %d)]", batch, ctx->max_batch,
               PAAC_ACT_STEP_MAX_ENVS_LARGE);
  PAAC_REQUIRE((int64_t)batch * (ctx->cfg.num_actions - 1) <= PAAC_FUSED_SAMPLE_MAX_DRAWS,
               "paac_act_step_mt: N*(A-1) = %ld exceeds %d (use paac_forward + paac_sample_mt + paac_synth_step)",
               (long)batch * (ctx->cfg.num_actions - 1), PAAC_FUSED_SAMPLE_MAX_DRAWS);
  if (!forward_has_fc_heads(ctx)) {
    // no head partials on this geometry (fc_heads_waves == 0): paac_forward + paac_sample_mt_synth_step's launch
    ForwardCall call = finish;
    if (const int rc = launch_forward(ctx, params, states, batch, call, s)) return rc;
    return launched(launch_sample_mt_synth_step(probs_out, ctx->cfg.num_actions, mt_state, actions, st, walk_scratch,
                                                walk_scratch_bytes, nullptr, s));
  }
  if (batch > PAAC_ACT_STEP_MAX_ENVS || (int64_t)batch * (ctx->cfg.num_actions - 1) > 1024) {
    // the large shards (128 x 18, 256 x 4): policy forward with its heads finish, then the sampler + environment-step launch
    // with the walks spread over several workgroups -- whose MT19937 doubles a spare workgroup of the fc launch makes
    // meanwhile (csrc/mt_ahead.h)
    const bool tail = (ctx->tower_on || ctx->tower2_on) && ctx->managed_weights && batch <= PAAC_ACT_STEP_MAX_ENVS_LARGE;
    ForwardCall call = finish;
    if (tail) {
      call.ahead_state = mt_state;
      call.ahead_D = batch * (ctx->cfg.num_actions - 1);
    }
    // (three launches when the walks can be spread -- walk_scratch lent -- and the action set is small: the sampler workgroups
    // then also finish the heads of the environments they visit, from the fc kernel's per-tile partials.  Measured: 256 x 4
    // 16.2 + 4.3 us -> 18.7 us per step, 1.898 -> 1.927 M env-steps/s; 128 x 18: 18.4 + 4.5 -> 24.0 us, SLOWER -- up to 24
    // rows x 19 outputs x 32 partials and an 18-way softmax at the head of every sampler workgroup's chain cost more than the
    // launch they replace -- so the fold is taken up to 8 actions.  PAAC_HEADS_IN_SAMPLER=0 / =1 force it off / on.)
    static const int fold_knob = [] {
      const char* v = getenv("PAAC_HEADS_IN_SAMPLER");
      return (v && *v) ? (atoi(v) != 0 ? 1 : 0) : -1;
    }();
    const bool fold = fold_knob >= 0 ? fold_knob == 1 : ctx->cfg.num_actions <= 8;
    if (tail && fold && sampler_folds_heads(batch, ctx->cfg.num_actions, walk_scratch))
      call.heads = kHeadsDefer;      // (the outputs are then the sampler launch's to write)
    if (const int rc = launch_forward(ctx, params, states, batch, call, s)) return rc;
    const HeadsPartials hp = partials_of(ctx, params, call, values_out);
    return launched(launch_sample_mt_synth_step(probs_out, ctx->cfg.num_actions, mt_state, actions, st, walk_scratch,
                                                walk_scratch_bytes, tail ? ctx->mt_ahead : nullptr, s,
                                                call.heads == kHeadsDefer ? &hp : nullptr));
  }
  // Up to 64 environments the sampler's state blocks and doubles already hide behind the loads of the head partials
  // (misc.hip: synth_step_a_mth_kernel): making them one launch ahead (csrc/mt_ahead.h) measured SLOWER here -- 658 k against
  // 669 k env-steps/s at the headline shape, the extra loads sit at the head of the sampler workgroup's chain --, so it is off
  // unless PAAC_MT_AHEAD_SMALL=1 asks for it.  The large shards (above) use it.
  static const bool ahead_on = [] {
    const char* v = getenv("PAAC_MT_AHEAD_SMALL");
    return v && *v && atoi(v) != 0;
  }();
  ForwardCall call = defer;
  if (ahead_on) {
    call.ahead_state = mt_state;
    call.ahead_D = batch * (ctx->cfg.num_actions - 1);
  }
  if (const int rc = launch_forward(ctx, params, states, batch, call, s)) return rc;
  return launched(launch_sample_env_step_heads(partials_of(ctx, params, call, values_out), probs_out, ctx->cfg.num_actions,
                                               mt_state, actions, st, ahead_on ? ctx->mt_ahead : nullptr, s));
}

int paac_act_step_pipe(paac_ctx* ctx, const float* params, const uint8_t* states, int batch, uint32_t* mt_state,
                       int32_t* actions, float* probs_out, float* values_out, uint64_t env_seed, uint32_t env_offset,
                       uint32_t terminal_threshold, const uint64_t* step_base_dev, uint64_t step_offset, uint8_t* stack_out,
                       uint8_t* stack_out2, float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len,
                       void* finished, uint8_t* raw_scratch, void* walk_scratch, int64_t walk_scratch_bytes,
                       paac_stream_t stream) {
  (void)walk_scratch;
  (void)walk_scratch_bytes;
  PAAC_REQUIRE(ctx && params && states && mt_state && actions && probs_out && values_out, "paac_act_step_pipe: null argument");
  PAAC_REQUIRE(!raw_scratch, "paac_act_step_pipe: path B (raw_scratch) keeps paac_act_step_mt's route -- its preprocess launch "
               "follows the step");
  SynthStep st;
  if (synth_step_of("paac_act_step_pipe", "null argument (the pipelined step always steps the environments)", false, &st, env_seed,
                    env_offset, batch, terminal_threshold, step_base_dev, step_offset, states, stack_out, stack_out2, rewards_out,
                    masks_out, ep_reward, ep_len, finished, nullptr))
    return -1;
  const int A = ctx->cfg.num_actions;
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch && batch <= PAAC_ACT_STEP_MAX_ENVS && (int64_t)batch * (A - 1) <= 1024 &&
               forward_has_fc_heads(ctx),
               "paac_act_step_pipe: up to min(max_batch=%d, %d) environments and 1024 draws on a geometry with the fc + head "
               "partials kernel (use paac_act_step_mt); got %d x %d actions", ctx->max_batch, PAAC_ACT_STEP_MAX_ENVS, batch, A);
  // two alternating regions of head partials, [tiles <= H / 8][batch][A + 1] each, in the acting fc slab buffer
  PAAC_REQUIRE((size_t)(ctx->spec.fc / 8) * batch * (A + 1) <= act_region_floats(ctx),
               "paac_act_step_pipe: two regions of head partials for %d x %d actions do not fit the fc slab buffer of "
               "max_batch=%d (use paac_act_step_mt)", batch, A, ctx->max_batch);
  ActRider rider{};
  rider.owed = *ctx->act_owed;
  rider.shift = st;
  const TowerRider trider = tower_rider_of(ctx, rider.owed, &st);
  ForwardCall call{.ws = 0, .heads = kHeadsDefer, .rider = &rider, .tower_rider = &trider};
  const int rc = launch_forward(ctx, params, states, batch, call, (hipStream_t)stream);
  if (call.rode) {   // the earlier debt rode that launch; this step's takes its place
    const HeadsPartials hp = partials_of(ctx, params, call, values_out);
    *ctx->act_owed = ActSample{hp.partial, hp.ntiles, hp.ba, hp.bc, probs_out, values_out, A, mt_state, actions, env_seed,
                               env_offset, batch, terminal_threshold, step_base_dev, step_offset, st.rec};
  }
  return launched(rc);
}

int paac_act_step_flush(paac_ctx* ctx, paac_stream_t stream) {
  PAAC_REQUIRE(ctx, "paac_act_step_flush: null ctx");
  if (!ctx->act_owed->partial) return 0;
  const int rc = launch_act_sample_flush(*ctx->act_owed, (hipStream_t)stream);
  if (rc) return rc;
  ctx->act_owed->partial = nullptr;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_act_step_pending(const paac_ctx* ctx) { return (ctx && ctx->act_owed->partial) ? 1 : 0; }

// The fields of a paac_returns that do not depend on the entry: the rollout records, estimator, lambda, the schedule pointers.
static int check_returns(const char* fn, const paac_returns* ret) {
  PAAC_REQUIRE(ret->rewards && ret->masks && ret->values && ret->y_out && ret->adv_out, "%s: null rollout record", fn);
  PAAC_REQUIRE(returns_estimator(ret) == PAAC_RETURNS_NSTEP || returns_estimator(ret) == PAAC_RETURNS_GAE,
               "%s: estimator %d (PAAC_RETURNS_NSTEP = 0, PAAC_RETURNS_GAE = 1)", fn, returns_estimator(ret));
  PAAC_REQUIRE(ret->gae_lambda >= 0.0 && ret->gae_lambda <= 1.0, "%s: gae_lambda %g outside [0, 1]", fn, ret->gae_lambda);
  PAAC_REQUIRE(!ret->global_step_dev || (ret->lr_out_dev && ret->lr_annealing_steps > 0),
               "%s: schedule bookkeeping needs lr_out_dev and lr_annealing_steps", fn);
  return 0;
}

// What every paac_loss_backward* entry does behind the refusals of its own arguments: the shared checks (then those of the
// returns record, for the two entries that take one: they read the batch), the training forward unless it has run, the
// launch.  fn: the entry called, named in every message.
static int loss_backward_entry(const char* fn, paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                               int batch, float entropy_beta, float* grad, float* loss_out, const BackwardCall& call,
                               int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params && states && actions && grad && (call.ret || (call.y && call.adv)), "%s: null argument", fn);
  PAAC_REQUIRE(batch > 0 && batch <= ctx->max_batch, "%s: batch %d outside (0, max_batch=%d]", fn, batch, ctx->max_batch);
  PAAC_REQUIRE(phase >= 0 && phase <= 3, "%s: phase %d", fn, phase);
  PAAC_NO_PENDING_SAMPLE(ctx, fn);
  if (const paac_returns* ret = call.ret) {
    PAAC_REQUIRE(ret->T > 0 && ret->N > 0 && ret->T * ret->N == batch, "%s: T*N = %d*%d != batch %d", fn, ret->T, ret->N, batch);
    if (const int rc = check_returns(fn, ret)) return rc;
    PAAC_REQUIRE(ret->v_boot || (forward_done && batch + ret->N <= ctx->max_batch),
                 "%s: v_boot == NULL takes the bootstrap values from rows [batch, batch + N) of a training forward that has "
                 "already run over batch + N rows", fn);
  }
  int rc = 0;
  if (!forward_done && phase != 2) {
    ForwardCall fwd{.ws = 1};
    rc = launch_forward(ctx, params, states, batch, fwd, (hipStream_t)stream);
    if (rc) return rc;
  }
  ctx->last_ws = 1;
  rc = launch_backward(ctx, params, states, actions, batch, entropy_beta, grad, loss_out, phase, call, (hipStream_t)stream);
  if (rc) return rc;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_loss_backward(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions, const float* y,
                       const float* adv, int batch, float entropy_beta, float* grad, float* loss_out,
                       int forward_done, int phase, paac_stream_t stream) {
  const BackwardCall call{.y = y, .adv = adv, .loss = kLossA3c};
  return loss_backward_entry("paac_loss_backward", ctx, params, states, actions, batch, entropy_beta, grad, loss_out, call,
                             forward_done, phase, stream);
}

int paac_loss_backward_returns(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                               const paac_returns* ret, int batch, float entropy_beta, float* grad, float* loss_out,
                               int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(ret, "paac_loss_backward_returns: null argument");
  const BackwardCall call{.ret = ret, .loss = kLossA3c};
  return loss_backward_entry("paac_loss_backward_returns", ctx, params, states, actions, batch, entropy_beta, grad, loss_out,
                             call, forward_done, phase, stream);
}

// (p_old_out: this is epoch 1 of a --ppo_epochs cycle -- the same arithmetic, plus the store of p_old)
int paac_loss_backward_returns_record(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                                      const paac_returns* ret, float* p_old_out, int batch, float entropy_beta, float* grad,
                                      float* loss_out, int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(ret, "paac_loss_backward_returns_record: null argument");
  PAAC_REQUIRE(p_old_out, "paac_loss_backward_returns_record: null p_old_out");
  const BackwardCall call{.ret = ret, .loss = kLossA3cRecord, .p_old_out = p_old_out};
  return loss_backward_entry("paac_loss_backward_returns_record", ctx, params, states, actions, batch, entropy_beta, grad,
                             loss_out, call, forward_done, phase, stream);
}

int paac_loss_backward_record(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                              const float* y, const float* adv, float* p_old_out, int batch, float entropy_beta, float* grad,
                              float* loss_out, int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(p_old_out, "paac_loss_backward_record: null p_old_out");
  const BackwardCall call{.y = y, .adv = adv, .loss = kLossA3cRecord, .p_old_out = p_old_out};
  return loss_backward_entry("paac_loss_backward_record", ctx, params, states, actions, batch, entropy_beta, grad, loss_out,
                             call, forward_done, phase, stream);
}

int paac_loss_backward_ppo(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions, const float* y,
                           const float* adv, const float* p_old, float clip_eps, int batch, float entropy_beta, float* grad,
                           float* loss_out, float* ppo_stats_out, int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(p_old, "paac_loss_backward_ppo: null p_old");
  PAAC_REQUIRE(clip_eps > 0.f && clip_eps < 1.f, "paac_loss_backward_ppo: clip_eps %g outside (0, 1)", (double)clip_eps);   // (NaN fails)
  const BackwardCall call{.y = y, .adv = adv, .loss = kLossPpo, .p_old = p_old, .clip_eps = clip_eps,
                          .ppo_stats_out = ppo_stats_out};
  return loss_backward_entry("paac_loss_backward_ppo", ctx, params, states, actions, batch, entropy_beta, grad, loss_out, call,
                             forward_done, phase, stream);
}

// Elements of activation `what` (paac_debug_activation) for `batch` rows of geometry `spec`; -1: no such activation.
static int64_t debug_activation_elems(const ArchSpec& spec, int what, int batch) {
  if (what == 25) return batch;
  if (what >= 21 && what <= 24) what -= 20;
  if (what >= 11 && what <= 10 + spec.nconv) what -= 10;
  if (what >= 1 && what <= spec.nconv) {
    const ConvSpec& cs = spec.conv[what - 1];
    return (int64_t)batch * cs.oh * cs.ow * cs.cout;
  }
  if (what == 4 || what == 14) return (int64_t)batch * spec.fc;
  return -1;
}

int paac_returns_norm_tick(paac_ctx* ctx, const float* params, const paac_returns* ret, float* adv_n_out, double* stats_out,
                           paac_stream_t stream) {
  PAAC_REQUIRE(ret && adv_n_out, "paac_returns_norm_tick: null argument");
  PAAC_REQUIRE(ret->T > 0 && ret->N > 0, "paac_returns_norm_tick: T=%d N=%d", ret->T, ret->N);
  if (const int rc = check_returns("paac_returns_norm_tick", ret)) return rc;
  if (ctx) PAAC_NO_PENDING_SAMPLE(ctx, "paac_returns_norm_tick");
  const float* v_boot = ret->v_boot;
  if (!v_boot) {
    const int64_t batch = (int64_t)ret->T * ret->N;
    PAAC_REQUIRE(ctx && params && batch + ret->N <= ctx->max_batch,
                 "paac_returns_norm_tick: v_boot == NULL takes the bootstrap values from rows [T*N, T*N + N) of a training "
                 "forward that has already run over T*N + N rows of this ctx");
    const int rc = launch_bootstrap_heads(ctx, params, (int)batch, ret->N, (hipStream_t)stream);
    if (rc) return rc;
    v_boot = ctx->ws[1].values + batch;
  }
  const int rc = launch_returns_norm(ret, v_boot, adv_n_out, stats_out, (hipStream_t)stream);
  if (rc) return rc;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_record_policy(paac_ctx* ctx, const float* params, const int32_t* actions, int batch, float* p_old_out, float* v_out,
                       int value_rows, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && params, "paac_record_policy: null argument");
  PAAC_REQUIRE(p_old_out || v_out, "paac_record_policy: nothing to record (p_old_out and v_out are both NULL)");
  PAAC_REQUIRE(!p_old_out || actions, "paac_record_policy: p_old_out needs the actions");
  PAAC_NO_PENDING_SAMPLE(ctx, "paac_record_policy");
  if (!p_old_out) batch = 0;
  if (!v_out) value_rows = 0;
  const int rows = batch > value_rows ? batch : value_rows;
  PAAC_REQUIRE(batch >= 0 && value_rows >= 0 && rows > 0 && rows <= ctx->max_batch,
               "paac_record_policy: batch %d / value_rows %d outside (0, max_batch=%d]", batch, value_rows, ctx->max_batch);
  // a trunk-only forward (or kept acting rows) is waiting for its heads: the launch a backward that cannot fuse them runs
  if (ctx->heads_pending_rows > 0) {
    PAAC_REQUIRE(rows <= ctx->heads_pending_rows, "paac_record_policy: the pending training forward covers %d rows, %d are asked "
                 "for", ctx->heads_pending_rows, rows);
    const int rc = launch_deferred_heads(ctx, params, (hipStream_t)stream);
    if (rc) return rc;
  }
  const int rc = launch_record_policy(ctx, actions, batch, value_rows, p_old_out, v_out, (hipStream_t)stream);
  if (rc) return rc;
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_loss_backward_ppo_vclip(paac_ctx* ctx, const float* params, const uint8_t* states, const int32_t* actions,
                                 const float* y, const float* adv, const float* p_old, const float* v_old, float clip_eps,
                                 float vclip_eps, int batch, float entropy_beta, float* grad, float* loss_out,
                                 float* ppo_stats_out, int forward_done, int phase, paac_stream_t stream) {
  PAAC_REQUIRE(p_old, "paac_loss_backward_ppo_vclip: null p_old");
  PAAC_REQUIRE(v_old, "paac_loss_backward_ppo_vclip: null v_old");
  PAAC_REQUIRE(clip_eps > 0.f && clip_eps < 1.f, "paac_loss_backward_ppo_vclip: clip_eps %g outside (0, 1)", (double)clip_eps);   // (NaN fails)
  PAAC_REQUIRE(vclip_eps > 0.f, "paac_loss_backward_ppo_vclip: vclip_eps %g is not positive (0 = off: paac_loss_backward_ppo)",
               (double)vclip_eps);                                                                                                // (NaN fails)
  const BackwardCall call{.y = y, .adv = adv, .loss = kLossPpoVclip, .p_old = p_old, .clip_eps = clip_eps,
                          .ppo_stats_out = ppo_stats_out, .v_old = v_old, .vclip_eps = vclip_eps};
  return loss_backward_entry("paac_loss_backward_ppo_vclip", ctx, params, states, actions, batch, entropy_beta, grad, loss_out,
                             call, forward_done, phase, stream);
}

int64_t paac_debug_activation_size(int arch, int what, int batch) {
  PAAC_REQUIRE(batch > 0, "paac_debug_activation_size: batch %d", batch);
  const int64_t n = debug_activation_elems(arch_spec(arch), what, batch);
  if (n < 0) {
    set_error("paac_debug_activation_size: what=%d", what);
    return -1;
  }
  return n;
}

int64_t paac_debug_activation(paac_ctx* ctx, int what, int batch, float* out, int64_t out_capacity, paac_stream_t stream) {
  PAAC_REQUIRE(ctx && out && batch > 0 && batch <= ctx->max_batch, "paac_debug_activation: bad arguments");
  if (what == 26) {                                        // policy outputs [batch, A] of the TRAINING set
    const int64_t np = (int64_t)batch * ctx->cfg.num_actions;
    PAAC_REQUIRE(np <= out_capacity, "paac_debug_activation: what=26 needs %ld floats, out holds %ld", (long)np, (long)out_capacity);
    PAAC_CHECK_HIP(hipMemcpyAsync(out, ctx->ws[1].probs, (size_t)np * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return np;
  }
  const int64_t n = debug_activation_elems(ctx->spec, what, batch);
  if (n < 0) {
    set_error("paac_debug_activation: what=%d", what);
    return -1;
  }
  PAAC_REQUIRE(n <= out_capacity, "paac_debug_activation: what=%d needs %ld floats, out holds %ld", what, (long)n,
               (long)out_capacity);
  if (what == 25) {                                        // value head outputs of the TRAINING set
    PAAC_CHECK_HIP(hipMemcpyAsync(out, ctx->ws[1].values, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return n;
  }
  const bool training_set = what >= 21 && what <= 24;      // 21..24: a1..a3 / h of the TRAINING set whichever was used last
  if (training_set) what -= 20;
  const Workspace& W = ctx->ws[training_set ? 1 : ctx->last_ws];
  const float* src;
  if (what >= 1 && what <= ctx->spec.nconv)
    src = W.act[what - 1];
  else if (what == 4)
    src = W.h;
  else if (what >= 11 && what <= 10 + ctx->spec.nconv)
    src = ctx->dact[what - 11];
  else
    src = ctx->dh;
  PAAC_CHECK_HIP(hipMemcpyAsync(out, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return n;
}

int paac_debug_set_tuning(paac_ctx* ctx, int op, int batch_class, int cfg, int ksplit, int xcd_dim) {
  PAAC_REQUIRE(ctx && op >= 0 && op < OP_COUNT && batch_class >= 0 && batch_class <= 2, "paac_debug_set_tuning: bad op/class");
  PAAC_REQUIRE(cfg_body(op, cfg) >= -1, "paac_debug_set_tuning: op %d has no configuration id %d (paac_debug_cfg_known)", op, cfg);
  ctx->tune[op][batch_class] = Tune{cfg, ksplit, xcd_dim};
  return 0;
}

int paac_debug_cfg_known(int op, int cfg) { return cfg_body(op, cfg) >= -1 ? 1 : 0; }
int paac_debug_cfg_body(int op, int cfg) { return cfg_body(op, cfg); }

int paac_debug_get_tuning(paac_ctx* ctx, int op, int batch_class, int* cfg, int* ksplit, int* xcd_dim) {
  PAAC_REQUIRE(ctx && op >= 0 && op < OP_COUNT && batch_class >= 0 && batch_class <= 2 && cfg && ksplit && xcd_dim,
               "paac_debug_get_tuning: bad argument");
  const Tune t = ctx->tune[op][batch_class];
  *cfg = t.cfg;
  *ksplit = t.ksplit;
  *xcd_dim = t.xcd;
  return 0;
}

// ---- hipGraph helpers -------------------------------------------------------------------------
int paac_graph_begin(paac_stream_t stream) {
  PAAC_CHECK_HIP(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return 0;
}

int paac_graph_end(paac_stream_t stream, paac_graph** out) {
  PAAC_REQUIRE(out, "paac_graph_end: null out");
  hipGraph_t g = nullptr;
  PAAC_CHECK_HIP(hipStreamEndCapture((hipStream_t)stream, &g));
  hipGraphExec_t ex = nullptr;
  hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(g);
    set_error("hipGraphInstantiate -> %s", hipGetErrorString(e));
    return -2;
  }
  paac_graph* pg = new paac_graph{g, ex};
  *out = pg;
  return 0;
}

int paac_graph_launch(paac_graph* g, paac_stream_t stream) {
  PAAC_REQUIRE(g, "paac_graph_launch: null graph");
  PAAC_CHECK_HIP(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return 0;
}

int paac_graph_destroy(paac_graph* g) {
  if (!g) return 0;
  (void)hipGraphExecDestroy(g->exec);
  (void)hipGraphDestroy(g->graph);
  delete g;
  return 0;
}

// ---- timing hooks -----------------------------------------------------------------------------
int paac_prof_enable(paac_ctx* ctx, int on) {
  PAAC_REQUIRE(ctx, "paac_prof_enable: null ctx");
  if (on) {
    for (int i = 0; i < paac_ctx::PROF_MAX_EVENTS; ++i) {
      if (!ctx->ev_start[i]) PAAC_CHECK_HIP(hipEventCreate(&ctx->ev_start[i]));
      if (!ctx->ev_stop[i]) PAAC_CHECK_HIP(hipEventCreate(&ctx->ev_stop[i]));
    }
  }
  ctx->prof_on = on ? 1 : 0;
  if (on) g_prof_ctx = ctx;
  else if (g_prof_ctx == ctx) g_prof_ctx = nullptr;
  return 0;
}

int paac_prof_read(paac_ctx* ctx, int32_t* family_out, int32_t* batch_out, float* ms_out, int max_events) {
  PAAC_REQUIRE(ctx, "paac_prof_read: null ctx");
  int n = 0;
  for (int i = 0; i < ctx->ev_count; ++i) {
    PAAC_CHECK_HIP(hipEventSynchronize(ctx->ev_stop[i]));
    float ms = 0.f;
    PAAC_CHECK_HIP(hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_stop[i]));
    if (n < max_events) {
      if (family_out) family_out[n] = ctx->ev_family[i];
      if (batch_out) batch_out[n] = ctx->ev_batch[i];
      if (ms_out) ms_out[n] = ms;
      ++n;
    }
  }
  ctx->ev_count = 0;
  return n;
}

int paac_prof_read_mix(paac_ctx* ctx, int32_t* mix_out, int max_events) {
  PAAC_REQUIRE(ctx && mix_out, "paac_prof_read_mix: null argument");
  int n = 0;
  for (int i = 0; i < ctx->ev_count && n < max_events; ++i) mix_out[n++] = ctx->ev_mix[i];
  return n;
}

int paac_user_arch(int32_t* nconv, int32_t* filters3, int32_t* fc_width) {
#ifdef PAAC_USER_ARCH
  if (nconv) *nconv = PAAC_USER_NCONV;
  if (filters3) {
    filters3[0] = PAAC_USER_C1;
    filters3[1] = PAAC_USER_C2;
    filters3[2] = PAAC_USER_NCONV == 3 ? PAAC_USER_C3 : 0;
  }
  if (fc_width) *fc_width = PAAC_USER_H;
  return 1;
#else
  if (nconv) *nconv = 0;
  if (fc_width) *fc_width = 0;
  if (filters3) filters3[0] = filters3[1] = filters3[2] = 0;
  return 0;
#endif
}

int paac_user_arch_layers(int32_t* sizes3, int32_t* strides3) {
#ifdef PAAC_USER_ARCH
  const ArchSpec s = arch_spec(PAAC_ARCH_USER);
  for (int i = 0; i < 3; ++i) {
    if (sizes3) sizes3[i] = i < s.nconv ? s.conv[i].k : 0;
    if (strides3) strides3[i] = i < s.nconv ? s.conv[i].stride : 0;
  }
  return 1;
#else
  for (int i = 0; i < 3; ++i) {
    if (sizes3) sizes3[i] = 0;
    if (strides3) strides3[i] = 0;
  }
  return 0;
#endif
}

const char* paac_prof_name(int family) {
  if (family < 0 || family >= PAAC_PROF_FAMILIES) return "";
  return kFamilyNames[family];
}

}  // extern "C"
