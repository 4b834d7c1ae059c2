// Device helpers of the synthetic environments (spec: paac_amd/synthetic.py), shared by the env-step kernels
// (csrc/misc.hip) and the heads kernel that absorbs the step in the counter-based-sampler mode (csrc/heads.h).
#pragma once
#include "common.h"

namespace paac {

constexpr int PRE_BANDS = 7;           // 84 rows = 7 bands x 12 rows

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t synth_key(uint64_t seed, uint32_t env, uint64_t id) {
  uint32_t k = lowbias32((uint32_t)seed ^ lowbias32(env + 0x9E3779B9u));
  k = lowbias32(k ^ (uint32_t)(seed >> 32) ^ lowbias32((uint32_t)id * 0x85EBCA6Bu + (uint32_t)(id >> 32) + 0x7F4A7C15u));
  return k;
}
__device__ __forceinline__ uint32_t synth_word(uint32_t key, uint32_t w) { return lowbias32(key + w * 0x9E3779B9u + 0x165667B1u); }

struct FinishedRing {
  int32_t count;
  int32_t pad;
  float reward[4096];
  int32_t len[4096];
};

// What a step records per environment: clipped reward and continuation mask of this step, the running episode totals, the
// ring of finished episodes (nullable).
struct StepRecords {
  float *rewards, *masks, *ep_reward;
  int32_t* ep_len;
  FinishedRing* fin;
};
// ... and, for the device games' step (game_step_kernel), the truncation plane of --bootstrap_truncated beside them
// (nullable: nothing is written, nothing is read).  The synthetic step never truncates: SynthStep carries the block above,
// and the kernels that take one keep their arguments.
struct EnvRecords : StepRecords {
  float* truncs;   // [N] for the step; 1.f truncated, 0.f otherwise
};

// One step of N synthetic environments: the generator's key (seed, first global environment, step id = *step_base + step_off
// + 1), the stacks read and written (stack_out2: the observation ring's wrap-around copy; raw: path B's screen pairs instead
// of the shift) and the records.  A value-initialised SynthStep is "no environment step": active() is the one test of that.
struct SynthStep {
  uint64_t seed;
  uint32_t env_offset;
  int N;
  uint32_t thresh;
  const uint64_t* step_base;
  uint64_t step_off;
  const uint32_t* stack_in;
  uint32_t *stack_out, *stack_out2;
  StepRecords rec;
  uint32_t* raw;
  __host__ __device__ bool active() const { return rec.rewards != nullptr; }
  __device__ uint64_t id() const { return (step_base ? *step_base : 0ull) + step_off + 1ull; }
};

// Per-env bookkeeping shared by both paths: emulator_runner.py:30-31 + paac.py:119-138.  ep_reward0 / ep_len0 = the
// running totals before this step (callers that have something to wait for load them early).
// hr5 = lowbias32(key ^ 0xA511E9B3) % 5 and term = lowbias32(key ^ 0x3C6EF372) < thresh do not depend on the action:
// a caller that waits for the action computes them first (synth_reward_slot / synth_terminal).
__device__ __forceinline__ uint32_t synth_reward_slot(uint32_t key) { return lowbias32(key ^ 0xA511E9B3u) % 5u; }
__device__ __forceinline__ bool synth_terminal(uint32_t key, uint32_t thresh) { return lowbias32(key ^ 0x3C6EF372u) < thresh; }
// env_bookkeep: the same records for a step whose unclipped reward r and terminal flag are already known (csrc/catch_dev.h).
__device__ __forceinline__ bool env_bookkeep(float r, bool term, int e, float ep_reward0, int32_t ep_len0, const StepRecords& rec) {
  rec.rewards[e] = fminf(fmaxf(r, -1.f), 1.f);   // actor_learner.py:95-101
  rec.masks[e] = term ? 0.f : 1.f;               // paac.py:119
  const float tot = ep_reward0 + r;
  const int len = ep_len0 + 1;
  if (term) {
    if (rec.fin) {
      const int slot = atomicAdd(&rec.fin->count, 1) & 4095;
      rec.fin->reward[slot] = tot;
      rec.fin->len[slot] = len;
    }
    rec.ep_reward[e] = 0.f;
    rec.ep_len[e] = 0;
  } else {
    rec.ep_reward[e] = tot;
    rec.ep_len[e] = len;
  }
  return term;
}
__device__ __forceinline__ bool synth_bookkeep_hashed(uint32_t hr5, bool term, int e, int act, float ep_reward0,
                                                      int32_t ep_len0, const StepRecords& rec) {
  const float table[5] = {-2.f, 0.f, 0.f, 1.f, 3.f};
  return env_bookkeep(table[(hr5 + (uint32_t)act) % 5u], term, e, ep_reward0, ep_len0, rec);
}
__device__ __forceinline__ bool synth_bookkeep_with(uint32_t key, int e, int act, uint32_t thresh, float ep_reward0,
                                                    int32_t ep_len0, const StepRecords& rec) {
  return synth_bookkeep_hashed(synth_reward_slot(key), synth_terminal(key, thresh), e, act, ep_reward0, ep_len0, rec);
}
__device__ __forceinline__ bool synth_bookkeep(uint32_t key, int e, const int32_t* actions, uint32_t thresh,
                                               const StepRecords& rec) {
  return synth_bookkeep_with(key, e, actions ? actions[e] : 0, thresh, rec.ep_reward[e], rec.ep_len[e], rec);
}

// Frame shift of one (env, band) unit of path A: push the step's new 84x84 plane into the 4-deep history
// (one dword = the 4 channels of a pixel).  unit = env * PRE_BANDS + band; 256 threads, 252 of them own one quad of four
// pixels each: ONE generator word is the quad's four new bytes, one 16-byte load and one 16-byte store per thread.
// In two halves, so that a caller with work of its own (the acting fc launch's workgroups, csrc/fc_heads.h) can put it between
// the load of the old stack and the store of the new one: synth_shift_load requests the thread's 16 bytes, synth_shift_store
// pushes the new bytes and writes.  Threads 252.. of the 256 own nothing in either half.
constexpr int SHIFT_QUADS = OBS_PIX / PRE_BANDS / 4;  // 252: 12 rows of 21 quads
// (The _at forms take the thread's index among the unit's 256 instead of threadIdx.x: the conv tower's helper waves, csrc/tower.h.)
__device__ __forceinline__ uint4 synth_shift_load_at(const int i, int unit, const uint32_t* __restrict__ stack_in) {
  if (i >= SHIFT_QUADS) return make_uint4(0u, 0u, 0u, 0u);
  const long quad = (long)(unit / PRE_BANDS) * (OBS_PIX / 4) + (unit % PRE_BANDS) * SHIFT_QUADS + i;
  return reinterpret_cast<const uint4*>(stack_in)[quad];
}
__device__ __forceinline__ uint4 synth_shift_load(int unit, const uint32_t* __restrict__ stack_in) {
  return synth_shift_load_at((int)threadIdx.x, unit, stack_in);
}
__device__ __forceinline__ void synth_shift_store_at(const int i, uint64_t seed, uint32_t env_offset, uint64_t id, uint32_t thresh,
                                                     int unit, uint4 old, uint32_t* __restrict__ stack_out,
                                                     uint32_t* __restrict__ stack_out2, const bool force_reset = false) {
  const int e = unit / PRE_BANDS;
  const int band = unit % PRE_BANDS;
  if (i >= SHIFT_QUADS) return;
  const int q = band * SHIFT_QUADS + i;                 // = y * 21 + (x >> 2): the generator's word index
  const long quad = (long)e * (OBS_PIX / 4) + q;
  const uint32_t key = synth_key(seed, env_offset + (uint32_t)e, id);
  const bool reset = force_reset || lowbias32(key ^ 0x3C6EF372u) < thresh;
  if (reset) old = make_uint4(0u, 0u, 0u, 0u);
  const uint32_t w = synth_word(key, (uint32_t)q);
  const uint4 outv = make_uint4((old.x >> 8) | ((w & 255u) << 24), (old.y >> 8) | (((w >> 8) & 255u) << 24),
                                (old.z >> 8) | (((w >> 16) & 255u) << 24), (old.w >> 8) | ((w >> 24) << 24));
  reinterpret_cast<uint4*>(stack_out)[quad] = outv;
  if (stack_out2) reinterpret_cast<uint4*>(stack_out2)[quad] = outv;   // second copy (the observation ring's wrap-around slot)
}
__device__ __forceinline__ void synth_shift_store(uint64_t seed, uint32_t env_offset, uint64_t id, uint32_t thresh, int unit,
                                                  uint4 old, uint32_t* __restrict__ stack_out,
                                                  uint32_t* __restrict__ stack_out2, const bool force_reset = false) {
  synth_shift_store_at((int)threadIdx.x, seed, env_offset, id, thresh, unit, old, stack_out, stack_out2, force_reset);
}
__device__ __forceinline__ void synth_shift_band(uint64_t seed, uint32_t env_offset, uint64_t id, uint32_t thresh, int unit,
                                                 const uint32_t* __restrict__ stack_in, uint32_t* __restrict__ stack_out,
                                                 uint32_t* __restrict__ stack_out2 = nullptr,
                                                 const bool force_reset = false) {
  // the old stack is requested whether or not this step resets the environment (1 step in 100 reads 16 bytes for nothing):
  // the reset flag hangs on the step id, which the caller has just LOADED -- asked for only when needed, the two round
  // trips to memory ran one after the other in every workgroup of the launch
  const uint4 old = force_reset ? make_uint4(0u, 0u, 0u, 0u) : synth_shift_load(unit, stack_in);
  synth_shift_store(seed, env_offset, id, thresh, unit, old, stack_out, stack_out2, force_reset);
}

// The pipelined acting step (paac_act_step_pipe, csrc/api.hip): what the sampler of one acting step still owes after the
// step's fc launch -- the heads finish, the MT19937 sampler and the bookkeeping of `N` environments, read from the head
// partials the fc launch left -- and what the NEXT fc launch carries beside its own work: that debt and the frame shift of
// its own step (shift.stack_in == nullptr: none, the bootstrap forward's launch).
// The heads finish of an owed sample done ahead of its sampler, by the conv tower launch that lies between the fc launch that
// left the partials and the fc launch that carries the sampler (csrc/tower.h: RIDER): what heads_finish_fused (fc_heads.h)
// leaves for the sampler's walks, at the limits of that routine -- one record per context, since fc(t) completes before
// tower(t + 1) starts.  any_zero: one word per finishing wave -- tower workgroups 0 .. 3, one helper wave each -- (the reader ORs the four).
constexpr int kActFinMaxN = 32, kActFinMaxA = 7, kActFinMaxTiles = 64;
struct ActFinishRecord {
  double pj[kActFinMaxN * (kActFinMaxA - 1)];      // conditional probabilities [N][A - 1]
  double thr[kActFinMaxN * (kActFinMaxA - 1)];     // packed walk thresholds, same order
  float probs[kActFinMaxN * kActFinMaxA];          // probabilities [N][A]
  int32_t any_zero[4];                             // != 0: some conditional probability is exactly zero
};
static_assert(sizeof(ActFinishRecord) <= 4096, "the finish record is a few KB");
struct ActSample {
  const float* partial;            // nullptr: nothing owed
  int ntiles;
  const float *ba, *bc;
  float *probs_out, *values_out;
  int A;
  uint32_t* mt_state;
  int32_t* actions;
  uint64_t seed;
  uint32_t env_offset;
  int N;
  uint32_t thresh;
  const uint64_t* step_base;
  uint64_t step_off;
  StepRecords rec;
  const ActFinishRecord* finished; // the heads of this debt are finished and the record holds them (set by the forward for the fc
                                   // launch behind a tower that carried the finish; nullptr: the sampler finishes them itself)
};
struct ActRider {
  ActSample owed;
  SynthStep shift;
};
// ... and what the conv tower launch in front of that fc launch carries on its helper waves (PAAC_ACT_TOWER_RIDER): the heads
// finish of the owed sample (fin.partial == nullptr: none) and the frame shift of its own step (shift.stack_in == nullptr: none;
// the fc launch then shifts nothing).
struct ActFinish {
  const float* partial;
  int ntiles;
  const float *ba, *bc;
  float *probs_out, *values_out;
  int A, N;
  ActFinishRecord* rec;
};
struct TowerRider {
  ActFinish fin;
  SynthStep shift;
};

// Path B: one of PRE_BANDS parts of environment e's raw 2 x 210 x 160 gray screen pair for step `id` (16,800 generator
// words = 4,200 16-byte stores per environment, 600 per unit).  unit = env * PRE_BANDS + part; 256 threads.
__device__ __forceinline__ void synth_raw_unit(uint64_t seed, uint32_t env_offset, uint64_t id, int unit,
                                               uint32_t* __restrict__ raw) {
  const int e = unit / PRE_BANDS;
  const int part = unit % PRE_BANDS;
  const uint32_t rkey = synth_key(seed, env_offset + (uint32_t)e, id) ^ 0x5bd1e995u;
  constexpr int WORDS = 2 * PAAC_RAW_H * PAAC_RAW_W / 4;   // 16800
  constexpr int PER = WORDS / 4 / PRE_BANDS;               // 600
  uint4* out = reinterpret_cast<uint4*>(raw + (long)e * WORDS);
  for (int q = part * PER + (int)threadIdx.x; q < (part + 1) * PER; q += 256)
    out[q] = make_uint4(synth_word(rkey, (uint32_t)(4 * q)), synth_word(rkey, (uint32_t)(4 * q + 1)),
                        synth_word(rkey, (uint32_t)(4 * q + 2)), synth_word(rkey, (uint32_t)(4 * q + 3)));
}

}  // namespace paac
