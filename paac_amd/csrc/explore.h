// --explore_bonus (spec and numpy twin: paac_amd/explore.py): a count-based exploration bonus on a SimHash of the observation
// ("#Exploration", Tang et al., arXiv 1611.04717).  Instantiated in misc.hip alone.
//
// explore_signs_kernel -- once per run: the +-1 matrix S[28224, 64] from the seed, as int8 in the order the projection reads it
//   * [k-step 441][column tile 4][lane 64][16 bytes]: byte b of lane (j = lane % 16, g = lane / 16) of column tile c at k-step s
//     is S[64 s + 16 g + b][16 c + j] -- one B fragment of v_mfma_i32_16x16x64_i8 is one coalesced 1 KB load, 16 bytes per lane.
// explore_kernel -- the whole bonus in one launch: projection, codes, increments, counts-after read, bonus, reward add
//   * The projection P = (x - 128) S runs on v_mfma_i32_16x16x64_i8, exact in int32.  The A fragment of lane (i = lane % 16, g) at
//     k-step s is the 16 bytes x[row i][64 s + 16 g ..] straight out of the observation ring, one XOR with 0x80808080 per dword
//     (uint8 -> centred int8, no widening).  The instruction sums over all 64 (g, byte) pairs and A and B index them alike, so
//     giving both operands the SAME k for the same (g, byte) is all the layout the sum needs.
//   * Work split: a workgroup owns 32 rows (two row tiles: every B fragment is used twice) and one of `ksplit` contiguous ranges
//     of the 441 k-steps (ksplit a divisor of 441, chosen by the host: explore_ksplit); its four waves take the range's k-steps
//     round-robin, each with all four column tiles -- 2 A + 4 B fragment loads and 8 MFMAs per k-step, the next step's loads
//     requested before this step's MFMAs.  Rows at or beyond `rows` read the last row and are dropped.
//   * The sign operand comes as int8 in fragment order out of L2 (1.8 MB: it stays resident) rather than as a 226 KB bit matrix
//     expanded in registers: the expansion is ~6 VALU operations per dword, 96 per k-step and lane against 8 MFMAs of 8 passes --
//     the VALU would be the bound -- while the int8 matrix costs L2 reads only: 1.8 MB per 32 rows.
//   * Reduction: the four waves' accumulators are added through LDS, then one int32 atomicAdd per element into the scratch
//     P[rows, 64] (integer adds commute: the sum is exact and deterministic).  Tickets: the last workgroup of a row group to
//     arrive reads its 32 rows back (one row per wave pass, the code is the wave's ballot of P >= 0), puts the scratch back to
//     zero, adds 1 to each row's slot of the table and parks the slot; the last row group to finish -- every increment of the
//     call is then in the table -- reads n = counts[slot] for every row and writes bonus and reward.  No second launch, no host.
#pragma once
#include "common.h"

namespace paac {

constexpr int kExpK = OBS_PIX * OBS_C;               // 28224 bytes of one stack
constexpr int kExpSteps = kExpK / 64;                // 441 k-steps
constexpr int kExpRowsWg = 32;                       // rows of one workgroup
constexpr int kExpFillWgs = 240;                     // workgroups the K split aims at (of 256 CUs)
constexpr int kExpKsplitMax = 63;
constexpr uint32_t kExpStream = 0x4558504Cu;         // "EXPL": the fourth counter word (explore.STREAM)
static_assert(kExpK % 64 == 0 && kExpSteps == 441, "the k-steps of one stack");

typedef int i32x4 __attribute__((ext_vector_type(4)));

// The K split of a call: the smallest divisor of 441 that fills the GPU, so a large shard is not split more than needed.
inline int explore_ksplit(int rows) {
  const int groups = (rows + kExpRowsWg - 1) / kExpRowsWg;
  const int divisors[] = {1, 3, 7, 9, 21, 49, 63};
  for (int d : divisors)
    if (groups * d >= kExpFillWgs) return d;
  return kExpKsplitMax;
}
// int32 words of the scratch of a call with `rows` rows: P[groups * 32][64], the parked slots, a ticket per row group and one more
inline int64_t explore_scratch_words(int rows) {
  const int64_t groups = (rows + kExpRowsWg - 1) / kExpRowsWg;
  return groups * (kExpRowsWg * 65 + 1) + 1;
}

struct ExploreArgs {
  const uint8_t* states;
  const i32x4* signs;
  int32_t* counts;
  int32_t* scratch;
  float* rewards;
  float* bonus_out;
  uint64_t* codes_out;      // nullable
  int rows, bits, table_bits, ksplit, groups;
  float beta;
};

__global__ __launch_bounds__(256) void explore_signs_kernel(const uint32_t k0, const uint32_t k1, i32x4* __restrict__ signs) {
  const int id = blockIdx.x * 256 + threadIdx.x;          // (step, column tile, lane): the grid is exactly 441 * 4 * 64 threads
  const int lane = id & 63, ct = (id >> 6) & 3, ks = id >> 8;
  const int j = 16 * ct + (lane & 15), g = lane >> 4;
  i32x4 v;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      uint32_t c[4] = {(uint32_t)(ks * 64 + 16 * g + 4 * d + b), (uint32_t)(j >> 5), 0u, kExpStream};
      philox4x32_10(c, k0, k1);
      word |= (((c[0] >> (j & 31)) & 1u) ? 0x01u : 0xFFu) << (8 * b);
    }
    v[d] = (int)word;
  }
  signs[id] = v;
}

// The last of `expected` arrivals at *ticket?  Every thread's stores are drained to the L2 first, thread 0 publishes them with a
// device-scope release in front of the ticket and acquires behind the last one (misc.hip's hand-off); the last arrival puts
// the ticket back to 0 for the next launch, which is stream-ordered behind this one.
__device__ __forceinline__ bool explore_last_arrival(int32_t* ticket, int expected, int* last_s) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const int old = atomicAdd(ticket, 1);
    *last_s = old == expected - 1;
    if (*last_s) {
      __threadfence();
      __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  return *last_s != 0;
}

__device__ __forceinline__ uint64_t explore_splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct ExploreFrags {
  i32x4 a[2], b[4];
};
__device__ __forceinline__ void explore_load(ExploreFrags& f, const uint8_t* p0, const uint8_t* p1, const i32x4* signs, int ks) {
  f.a[0] = *reinterpret_cast<const i32x4*>(p0 + ks * 64);
  f.a[1] = *reinterpret_cast<const i32x4*>(p1 + ks * 64);
#pragma unroll
  for (int c = 0; c < 4; ++c) f.b[c] = signs[(ks * 4 + c) * 64];
}

__global__ __launch_bounds__(256) void explore_kernel(const ExploreArgs a) {
  __shared__ int red[4][2048];
  __shared__ int last_s;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rg = blockIdx.x / a.ksplit, part = blockIdx.x - rg * a.ksplit;
  const int per = kExpSteps / a.ksplit, ks_end = (part + 1) * per;
  const int row0 = rg * kExpRowsWg;
  int32_t* const P = a.scratch;
  int32_t* const slots = a.scratch + (int64_t)a.groups * kExpRowsWg * 64;
  int32_t* const tickets = slots + (int64_t)a.groups * kExpRowsWg;

  // ---- projection: this wave's k-steps of the workgroup's range, 32 rows x 64 columns ---------------------------------------
  const int i = lane & 15, g = lane >> 4;
  const uint8_t* p0 = a.states + (size_t)min(row0 + i, a.rows - 1) * kExpK + 16 * g;
  const uint8_t* p1 = a.states + (size_t)min(row0 + 16 + i, a.rows - 1) * kExpK + 16 * g;
  const i32x4* signs = a.signs + lane;
  i32x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = (i32x4){0, 0, 0, 0};
  int ks = part * per + wave;
  ExploreFrags cur, nxt;
  if (ks < ks_end) explore_load(cur, p0, p1, signs, ks);
  for (; ks < ks_end; ks += 4) {
    const bool more = ks + 4 < ks_end;
    if (more) explore_load(nxt, p0, p1, signs, ks + 4);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const i32x4 x = cur.a[t] ^ (i32x4){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(x, cur.b[c], acc[t][c], 0, 0, 0);
    }
    if (more) cur = nxt;
  }

  // ---- the four waves' partials through LDS, one atomicAdd per element of P --------------------------------------------------
  // D layout: accumulator v of lane (j = lane % 16, q = lane / 16) is row 4 q + v, column j of the tile
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int v = 0; v < 4; ++v) red[wave][((t * 4 + c) * 4 + v) * 64 + lane] = acc[t][c][v];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int x = q * 256 + tid, e = x >> 6, ln = x & 63;
    const int row = row0 + 16 * (e >> 4) + 4 * (ln >> 4) + (e & 3), col = 16 * ((e >> 2) & 3) + (ln & 15);
    const int sum = (red[0][x] + red[1][x]) + (red[2][x] + red[3][x]);
    if (row < a.rows) atomicAdd(&P[(int64_t)row * 64 + col], sum);
  }
  if (!explore_last_arrival(&tickets[rg], a.ksplit, &last_s)) return;

  // ---- the row group is complete: codes, slots, increments; the scratch goes back to zero ------------------------------------
  for (int rr = wave; rr < kExpRowsWg; rr += 4) {
    const int row = row0 + rr;
    if (row >= a.rows) break;
    int32_t* cell = &P[(int64_t)row * 64 + lane];
    const int p = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cell, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t code = __ballot(p >= 0 && lane < a.bits);
    if (lane == 0) {
      const uint32_t slot = (uint32_t)(explore_splitmix64(code) >> (64 - a.table_bits));
      atomicAdd(&a.counts[slot], 1);
      slots[row] = (int32_t)slot;
      if (a.codes_out) a.codes_out[row] = code;
    }
  }
  if (!explore_last_arrival(&tickets[a.groups], a.groups, &last_s)) return;

  // ---- every increment of the call is in the table: counts-after read, bonus, reward add -------------------------------------
  for (int row = tid; row < a.rows; row += 256) {
    const int slot = __hip_atomic_load(&slots[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    slots[row] = 0;          // (the whole scratch is left zero)
    const int n = __hip_atomic_load(&a.counts[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float bonus = a.beta / sqrtf((float)n);
    a.bonus_out[row] = bonus;
    a.rewards[row] += bonus;
  }
}

}  // namespace paac
