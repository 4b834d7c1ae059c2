// The rally environments on the device (spec: paac_amd/rally.py): the game trait RallyGame (see csrc/game_dev.h) of the step
// and evaluation kernels in csrc/games.hip.
#pragma once
#include "game_dev.h"

namespace paac {

constexpr int RALLY_CELLS = 14;          // board cells per side
constexpr int RALLY_CELL = 6;            // pixels per cell side: 14 x 6 = 84
constexpr int RALLY_POINTS = 5;
constexpr int RALLY_MAX_STEPS = 1000;
constexpr int RALLY_REACT_ROW = 5;       // the opponent reacts to a ball flying up in rows 1..5
constexpr uint32_t RALLY_LAZY = 4u;      // ... except on one step in four

struct RallyState {
  int32_t bx, by, dx, dy, px, ox, mine, theirs, steps, k;
};

// The ball served for the n-th time in the episode of key h, towards the agent or the opponent; the paddles stay.
__device__ __forceinline__ void rally_serve(uint32_t h, int n, bool towards_agent, RallyState& s) {
  const uint32_t w = lowbias32(h ^ (0xA11E0002u + 16u * (uint32_t)n));
  s.bx = (int32_t)((w >> 1) % (uint32_t)RALLY_CELLS);
  s.dx = (w & 1u) ? 1 : -1;
  s.by = towards_agent ? 6 : 7;
  s.dy = towards_agent ? 1 : -1;
}

// What a pixel row in board row cy can show beside the ball: the column and the pixel value of the paddle in it (value 0 in
// rows 1..12), and whether the ball is in the row.  Worked out once per quad.
struct RallyRow {
  int padx;
  uint32_t padv, ball;       // ball: all ones or 0
};

__device__ __forceinline__ RallyRow rally_row(const RallyState& s, int cy) {
  RallyRow r;
  r.padx = cy == 0 ? s.ox : s.px;
  r.padv = (-(uint32_t)(cy == 0) & 64u) | (-(uint32_t)(cy == RALLY_CELLS - 1) & 128u);
  r.ball = -(uint32_t)(cy == s.by);
  return r;
}

// Pixel x of a pixel row, `row` = rally_row(s, cy).  Masks and bitwise operations only, no branches: written as `?:` chains the
// compiler made an exec-masked branch of every pixel.
__device__ __forceinline__ uint32_t rally_pixel(const RallyState& s, const RallyRow& row, int x) {
  const int cx = x / RALLY_CELL;
  const uint32_t ball = row.ball & -(uint32_t)(cx == s.bx);
  const uint32_t paddle = -(uint32_t)((uint32_t)(cx - row.padx) < 2u) & row.padv;
  return (ball & 255u) | (~ball & paddle);
}

struct RallyGame {
  typedef RallyState State;
  static constexpr int kWords = 12;      // int32 words of a state record: the 10 of State, then padding (three 16-byte parts)

  static __device__ __forceinline__ State load(const int32_t* __restrict__ state, int e) {
    const int4* p = reinterpret_cast<const int4*>(state) + 3 * e;
    const int4 a = p[0], b = p[1], c = p[2];
    State s;
    s.bx = a.x; s.by = a.y; s.dx = a.z; s.dy = a.w;
    s.px = b.x; s.ox = b.y; s.mine = b.z; s.theirs = b.w;
    s.steps = c.x; s.k = c.y;
    return s;
  }

  static __device__ __forceinline__ void store(int32_t* __restrict__ state, int e, const State& s) {
    int4* p = reinterpret_cast<int4*>(state) + 3 * e;
    p[0] = make_int4(s.bx, s.by, s.dx, s.dy);
    p[1] = make_int4(s.px, s.ox, s.mine, s.theirs);
    p[2] = make_int4(s.steps, s.k, 0, 0);
  }

  static __device__ __forceinline__ State start(uint64_t seed, uint32_t env, int32_t k = 0) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)k);
    State s;
    s.px = (int32_t)(lowbias32(h ^ 0xA11E0001u) % (uint32_t)(RALLY_CELLS - 1));
    s.ox = (int32_t)(lowbias32(h ^ 0xA11E0003u) % (uint32_t)(RALLY_CELLS - 1));
    s.mine = s.theirs = s.steps = 0;
    s.k = k;
    rally_serve(h, 0, true, s);
    return s;
  }

  // One step of state s under action a (ALE Pong's minimal set: 2, 4 = right, 3, 5 = left, anything else = stay), a pure
  // function of its arguments: the state the next step starts from (the next episode's start state after a terminal step), the
  // reward and the terminal flag.  Everything here is the same for all threads of a workgroup (one environment per workgroup
  // column): the branches and the opponent's look-ahead loop, of at most RALLY_REACT_ROW iterations, are uniform.
  // *trunc: the step is terminal only because steps reached the cap (neither side reached RALLY_POINTS on it).
  static __device__ __forceinline__ State advance(uint64_t seed, uint32_t env, State s, int a, int /*opt*/, float* reward,
                                                  bool* term, bool* trunc = nullptr) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)s.k);
    if (a == 2 || a == 4) s.px = min(s.px + 1, RALLY_CELLS - 2);
    else if (a == 3 || a == 5) s.px = max(s.px - 1, 0);
    if (s.dy < 0 && s.by <= RALLY_REACT_ROW && lowbias32(h ^ (0xA11E1000u + (uint32_t)s.steps)) % RALLY_LAZY != 0u) {
      int tx = s.bx, d = s.dx;                                               // the column the ball enters row 0 in
      for (int i = 0; i < s.by; ++i) {
        const int n = tx + d;
        const bool wall = n < 0 || n > RALLY_CELLS - 1;
        d = wall ? -d : d;
        tx = wall ? tx : n;
      }
      if (tx < s.ox) s.ox -= 1;
      else if (tx > s.ox + 1) s.ox += 1;
    }
    int nx = s.bx + s.dx;
    if (nx < 0 || nx > RALLY_CELLS - 1) {
      s.dx = -s.dx;
      nx = s.bx;
    }
    int ny = s.by + s.dy;
    float r = 0.f;
    if (ny == RALLY_CELLS - 1) {
      if (nx == s.px || nx == s.px + 1) {
        s.dy = -1;
        s.dx = nx == s.px ? -1 : 1;
        ny = s.by;
      } else {
        s.theirs += 1;
        r = -1.f;
      }
    } else if (ny == 0) {
      if (nx == s.ox || nx == s.ox + 1) {
        s.dy = 1;
        s.dx = nx == s.ox ? -1 : 1;
        ny = s.by;
      } else {
        s.mine += 1;
        r = 1.f;
      }
    }
    s.bx = nx;
    s.by = ny;
    s.steps += 1;
    const bool decided = s.mine == RALLY_POINTS || s.theirs == RALLY_POINTS;
    const bool over = decided || s.steps == RALLY_MAX_STEPS;
    if (trunc) *trunc = !decided && s.steps == RALLY_MAX_STEPS;
    *reward = r;
    *term = over;
    if (over) return start(seed, env, s.k + 1);
    if (r != 0.f) rally_serve(h, s.mine + s.theirs, r < 0.f, s);
    return s;
  }

  // Quad q of an observation with the plane of state s pushed into its history `old` (an empty one if `fresh`).  A quad may
  // straddle two cells (6 is no multiple of 4): every pixel asks for itself; what hangs on the row is worked out once.
  static __device__ __forceinline__ uint4 shift_quad(const State& s, int q, uint4 old, bool fresh) {
    int y, x;
    quad_yx(q, &y, &x);
    const RallyRow row = rally_row(s, y / RALLY_CELL);
    return push_plane(old, fresh, rally_pixel(s, row, x) << 24, rally_pixel(s, row, x + 1) << 24,
                      rally_pixel(s, row, x + 2) << 24, rally_pixel(s, row, x + 3) << 24);
  }
};

}  // namespace paac
