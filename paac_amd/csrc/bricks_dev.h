// The bricks environments on the device (spec: paac_amd/bricks.py): the game trait BricksGame (see csrc/game_dev.h) of the
// step and evaluation kernels in csrc/games.hip.
#pragma once
#include "game_dev.h"

namespace paac {

constexpr int BRICKS_CELLS = 14;         // board cells per side
constexpr int BRICKS_CELL = 6;           // pixels per cell side: 14 x 6 = 84
constexpr int BRICKS_LIVES = 3;
constexpr int BRICKS_MAX_STEPS = 500;
constexpr int BRICKS_ROW0 = 2;           // the bricks' first board row; three rows of them
constexpr int BRICKS_FULL_ROW = 0x3FFF;
constexpr int BRICKS_SERVE_ROW = 5;

struct BricksState {
  int32_t bx, by, dx, dy, px, lives, steps, k, r0, r1, r2;
};

// The ball served for the n-th time in the episode of key h, over the paddle where it stands.
__device__ __forceinline__ void bricks_serve(uint32_t h, int n, BricksState& s) {
  s.bx = s.px;
  s.by = BRICKS_SERVE_ROW;
  s.dy = 1;
  s.dx = (lowbias32(h ^ (0xB41C0002u + 16u * (uint32_t)n)) & 1u) ? 1 : -1;
}

// The bricks of board row cy as a 14-bit mask (0 outside rows 2..4).  Arithmetic, not a switch: cy differs from thread to thread.
__device__ __forceinline__ uint32_t bricks_row_mask(const BricksState& s, int cy) {
  const int br = cy - BRICKS_ROW0;
  return (uint32_t)((-(int)(br == 0) & s.r0) | (-(int)(br == 1) & s.r1) | (-(int)(br == 2) & s.r2));
}

// Pixel x of a pixel row in board row cy, `row` = bricks_row_mask(s, cy).  Selects and bitwise ands only, no branches.
__device__ __forceinline__ uint32_t bricks_pixel(const BricksState& s, int cy, uint32_t row, int x) {
  const int cx = x / BRICKS_CELL;
  const uint32_t brick = ((row >> cx) & 1u) << 6;                                                  // 64 or 0
  const bool paddle = (cy == BRICKS_CELLS - 1) & ((uint32_t)(cx - s.px) < 2u);                     // no bricks in row 13
  const bool ball = (cy == s.by) & (cx == s.bx);
  return ball ? 255u : (paddle ? 128u : brick);
}

struct BricksGame {
  typedef BricksState State;
  static constexpr int kWords = 12;      // int32 words of a state record: the 11 of State, then padding (three 16-byte parts)

  static __device__ __forceinline__ State load(const int32_t* __restrict__ state, int e) {
    const int4* p = reinterpret_cast<const int4*>(state) + 3 * e;
    const int4 a = p[0], b = p[1], c = p[2];
    State s;
    s.bx = a.x; s.by = a.y; s.dx = a.z; s.dy = a.w;
    s.px = b.x; s.lives = b.y; s.steps = b.z; s.k = b.w;
    s.r0 = c.x; s.r1 = c.y; s.r2 = c.z;
    return s;
  }

  static __device__ __forceinline__ void store(int32_t* __restrict__ state, int e, const State& s) {
    int4* p = reinterpret_cast<int4*>(state) + 3 * e;
    p[0] = make_int4(s.bx, s.by, s.dx, s.dy);
    p[1] = make_int4(s.px, s.lives, s.steps, s.k);
    p[2] = make_int4(s.r0, s.r1, s.r2, 0);
  }

  static __device__ __forceinline__ State start(uint64_t seed, uint32_t env, int32_t k = 0) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)k);
    State s;
    s.px = (int32_t)(lowbias32(h ^ 0xB41C0001u) % (uint32_t)(BRICKS_CELLS - 1));
    s.lives = BRICKS_LIVES;
    s.steps = 0;
    s.k = k;
    s.r0 = s.r1 = s.r2 = BRICKS_FULL_ROW;
    bricks_serve(h, 0, s);
    return s;
  }

  // One step of state s under action a (1 = left, 2 = right, anything else = stay), a pure function of its arguments: the
  // state the next step starts from (the next episode's start state after a terminal step), the reward and the terminal flag.
  // single_life != 0: losing a ball ends the episode.  *trunc: the step is terminal only because steps reached the cap.
  static __device__ __forceinline__ State advance(uint64_t seed, uint32_t env, State s, int a, int single_life, float* reward,
                                                  bool* term, bool* trunc = nullptr) {
    const bool single = single_life != 0;
    if (a == 1) s.px = max(s.px - 1, 0);
    else if (a == 2) s.px = min(s.px + 1, BRICKS_CELLS - 2);
    int nx = s.bx + s.dx;
    if (nx < 0 || nx > BRICKS_CELLS - 1) {
      s.dx = -s.dx;
      nx = s.bx;
    }
    int ny = s.by + s.dy;
    const int br = ny - BRICKS_ROW0;                                         // the brick row the ball heads for, if 0..2
    const int mask = br == 0 ? s.r0 : (br == 1 ? s.r1 : (br == 2 ? s.r2 : 0));
    const int bit = 1 << nx;
    float r = 0.f;
    bool over = false, lost = false;
    if (ny < 0) {
      s.dy = 1;
      ny = s.by;
    } else if (mask & bit) {
      if (br == 0) s.r0 &= ~bit;
      else if (br == 1) s.r1 &= ~bit;
      else s.r2 &= ~bit;
      r = 1.f;
      s.dy = -s.dy;
      nx = s.bx;
      ny = s.by;
    } else if (ny == BRICKS_CELLS - 1) {
      if (nx == s.px || nx == s.px + 1) {
        s.dy = -1;
        s.dx = nx == s.px ? -1 : 1;
        ny = s.by;
        if ((s.r0 | s.r1 | s.r2) == 0) s.r0 = s.r1 = s.r2 = BRICKS_FULL_ROW;
      } else {
        s.lives -= 1;
        lost = true;
        over = s.lives == 0 || single;
      }
    }
    s.bx = nx;
    s.by = ny;
    s.steps += 1;
    if (trunc) *trunc = !over && s.steps == BRICKS_MAX_STEPS;
    over = over || s.steps == BRICKS_MAX_STEPS;
    *reward = r;
    *term = over;
    if (over) return start(seed, env, s.k + 1);
    if (lost) bricks_serve(synth_key(seed, env, (uint64_t)(uint32_t)s.k), BRICKS_LIVES - s.lives, s);
    return s;
  }

  // Quad q of an observation with the plane of state s pushed into its history `old` (an empty one if `fresh`).  A quad may
  // straddle two cells (6 is no multiple of 4): every pixel asks for itself; what hangs on the row is worked out once.
  static __device__ __forceinline__ uint4 shift_quad(const State& s, int q, uint4 old, bool fresh) {
    int y, x;
    quad_yx(q, &y, &x);
    const int cy = y / BRICKS_CELL;
    const uint32_t row = bricks_row_mask(s, cy);
    return push_plane(old, fresh, bricks_pixel(s, cy, row, x) << 24, bricks_pixel(s, cy, row, x + 1) << 24,
                      bricks_pixel(s, cy, row, x + 2) << 24, bricks_pixel(s, cy, row, x + 3) << 24);
  }
};

}  // namespace paac
