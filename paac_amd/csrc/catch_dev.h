// The catch environments on the device (spec: paac_amd/catch.py): the game trait CatchGame (see csrc/game_dev.h) of the step
// and evaluation kernels in csrc/games.hip.
#pragma once
#include "game_dev.h"

namespace paac {

constexpr int CATCH_CELLS = 14;        // board cells per side
constexpr int CATCH_CELL = 6;          // pixels per cell side: 14 x 6 = 84

struct CatchState {
  int32_t bx, by, dx, px, k;
};

__device__ __forceinline__ uint32_t catch_pixel(const CatchState& s, int y, int x) {
  const int cy = y / CATCH_CELL, cx = x / CATCH_CELL;
  return (cy == s.by && cx == s.bx) ? 255u : ((cy == CATCH_CELLS - 1 && cx == s.px) ? 128u : 0u);
}

struct CatchGame {
  typedef CatchState State;
  static constexpr int kWords = 8;     // int32 words of a state record: bx, by, dx, px, k, then padding (two 16-byte halves)

  static __device__ __forceinline__ State start(uint64_t seed, uint32_t env, int32_t k = 0) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)k);
    State s;
    s.bx = (int32_t)(lowbias32(h ^ 0xC47C0001u) % (uint32_t)CATCH_CELLS);
    s.px = (int32_t)(lowbias32(h ^ 0xC47C0002u) % (uint32_t)CATCH_CELLS);
    s.dx = (int32_t)(lowbias32(h ^ 0xC47C0003u) % 3u) - 1;
    s.by = k == 0 ? (int32_t)(lowbias32(h ^ 0xC47C0004u) % (uint32_t)(CATCH_CELLS - 1)) : 0;
    s.k = k;
    return s;
  }

  static __device__ __forceinline__ State load(const int32_t* __restrict__ state, int e) {
    const int4 lo = reinterpret_cast<const int4*>(state)[2 * e];
    State s;
    s.bx = lo.x; s.by = lo.y; s.dx = lo.z; s.px = lo.w;
    s.k = state[e * kWords + 4];
    return s;
  }

  static __device__ __forceinline__ void store(int32_t* __restrict__ state, int e, const State& s) {
    reinterpret_cast<int4*>(state)[2 * e] = make_int4(s.bx, s.by, s.dx, s.px);
    reinterpret_cast<int4*>(state)[2 * e + 1] = make_int4(s.k, 0, 0, 0);
  }

  // One step of state s under action a (1 = left, 2 = right, anything else = stay), a pure function of its arguments: the
  // state the next step starts from (the next episode's start state after a terminal step), the reward and the terminal flag.
  // Never truncated: 13 steps is the game's rule, not a limit.
  static __device__ __forceinline__ State advance(uint64_t seed, uint32_t env, State s, int a, int /*opt*/, float* reward,
                                                  bool* term, bool* trunc = nullptr) {
    if (trunc) *trunc = false;
    if (a == 1) s.px = max(s.px - 1, 0);
    else if (a == 2) s.px = min(s.px + 1, CATCH_CELLS - 1);
    int nx = s.bx + s.dx;
    if (nx < 0 || nx > CATCH_CELLS - 1) {
      s.dx = -s.dx;
      nx = s.bx + s.dx;
    }
    s.bx = nx;
    s.by += 1;
    *term = s.by == CATCH_CELLS - 1;
    *reward = *term ? (s.bx == s.px ? 1.f : -1.f) : 0.f;
    return *term ? start(seed, env, s.k + 1) : s;
  }

  // Quad q of an observation with the plane of state s pushed into its history `old` (an empty one if `fresh`).  A quad may
  // straddle two cells (6 is no multiple of 4): every pixel asks for itself.
  static __device__ __forceinline__ uint4 shift_quad(const State& s, int q, uint4 old, bool fresh) {
    int y, x;
    quad_yx(q, &y, &x);
    return push_plane(old, fresh, catch_pixel(s, y, x) << 24, catch_pixel(s, y, x + 1) << 24, catch_pixel(s, y, x + 2) << 24,
                      catch_pixel(s, y, x + 3) << 24);
  }
};

}  // namespace paac
