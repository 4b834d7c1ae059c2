// What the device games share (catch_dev.h, bricks_dev.h, rally_dev.h; kernels: game_step_kernel and eval_step_kernel in
// csrc/games.hip): where a thread's quad is, and the push of a new plane into an observation's history.
// A game is one trait struct G in its header:
//   State, kWords                                    the state record in registers, its int32 words in memory
//   load(state, e), store(state, e, s)               record e of a [N, kWords] buffer
//   start(seed, env)                                 episode 0's start state
//   advance(seed, env, s, a, opt, &reward, &term[, &trunc])
//                                                    one step, a pure function of its arguments (opt: the game's one integer
//                                                    option, bricks' single_life; 0 where a game has none).  trunc (optional,
//                                                    --bootstrap_truncated): the step was terminal ONLY because the game's step
//                                                    cap was reached -- a step that also ends the episode for a real reason is
//                                                    not truncated, a game without a cap (catch) never is; term keeps its meaning
//   shift_quad(s, q, old, fresh)                     quad q of the observation: the plane of s pushed into `old`
// A PAIRED game (duel_dev.h) declares `static constexpr bool kPaired = true`: its N rows are N / 2 boards with two players
// each, and a row's step is a pure function of (state_in[e], actions[e], actions[partner(e, N)]).  It provides instead
//   is_top(e, N), board(e, N), partner(e, N)         the row's side, its board (the hash key is env_offset + board) and the
//                                                    row that plays the other side
//   start(seed, env_offset, e, N)                    episode 0's start record of row e
//   advance(seed, g, s, a_own, a_partner, is_top, &reward, &term, &trunc)
// and has no evaluation form (eval_step_kernel is not instantiated for it); what it has instead is the match form,
// match_step_kernel in csrc/games.hip: two policies' probabilities in one block, one on each side of every board.
#pragma once
#include <type_traits>

#include "synth_dev.h"

namespace paac {

// Whether trait G is a paired game: true only where G says so.
template <class G, class = void>
struct game_is_paired : std::false_type {};
template <class G>
struct game_is_paired<G, std::void_t<decltype(G::kPaired)>> : std::bool_constant<G::kPaired> {};

constexpr int QUADS_PER_ROW = OBS_W / 4;                  // 21
constexpr int QUADS_PER_BAND = OBS_PIX / PRE_BANDS / 4;   // 252: 12 rows of 21 quads

// Workgroup (e, band) of a grid (N, 7), 256 threads: 252 of them own one quad of four pixels (one dword = the 4 channels of a
// pixel), q = y * 21 + (x >> 2) within the observation.
struct QuadThread {
  int e, band, i, q;
  bool owner;
  long quad;       // the quad's index in an [N, 84, 84, 4] buffer, counted in 16-byte units
  long load_quad;  // what the thread loads: its quad, or the band's first one (the four threads that own none)
};

__device__ __forceinline__ QuadThread quad_thread() {
  QuadThread t;
  t.e = blockIdx.x;
  t.band = blockIdx.y;
  t.i = threadIdx.x;
  t.owner = t.i < QUADS_PER_BAND;
  t.q = t.band * QUADS_PER_BAND + t.i;
  t.quad = (long)t.e * (OBS_PIX / 4) + t.q;
  t.load_quad = t.owner ? t.quad : t.quad - t.i;
  return t;
}

// Pixel row y and first pixel column x of quad q.
__device__ __forceinline__ void quad_yx(int q, int* y, int* x) {
  *y = q / QUADS_PER_ROW;
  *x = (q % QUADS_PER_ROW) * 4;
}

// Four pixels of the new plane, each already in the top byte of its dword (p << 24), pushed into the 4-deep history `old` (an
// empty history if `fresh`: after a terminal step).  `fresh` masks the history instead of branching on it: the plane's bytes
// are worked out first and the wait for the stack load comes after them.
__device__ __forceinline__ uint4 push_plane(uint4 old, bool fresh, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  const uint32_t keep = fresh ? 0u : 0x00FFFFFFu;
  return make_uint4(((old.x >> 8) & keep) | p0, ((old.y >> 8) & keep) | p1, ((old.z >> 8) & keep) | p2,
                    ((old.w >> 8) & keep) | p3);
}

}  // namespace paac
