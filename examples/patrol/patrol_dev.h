// The patrol environments on the device (spec: patrol.py beside this file): the game trait PatrolGame (contract: the package's
// csrc/game_dev.h) that --emulator user --device_game compiles into the step and evaluation kernels of csrc/games.hip.
// Nothing here touches memory but load / store: no LDS, no atomics; the kernels do one 16-byte load and one 16-byte store of
// the observation per thread.
#pragma once
#include "game_dev.h"

namespace paac {

constexpr int PATROL_CELLS = 14;         // board cells per side
constexpr int PATROL_CELL = 6;           // pixels per cell side: 14 x 6 = 84
constexpr int PATROL_LIVES = 3;
constexpr int PATROL_MAX_STEPS = 1000;
constexpr int PATROL_SHOT_SPEED = 2;
constexpr uint32_t PATROL_WAIT = 32u;
constexpr int PATROL_ACTIONS = 18;

// Drone i lives in row 3 * i + 2: rows 2, 5, 8, 11.

// ALE's 18 actions as (mx, my, fire): mx + 1 and my + 1 of action a in bits [2a, 2a + 2) of one 64-bit constant each; fire is
// action 1 and actions 10..17.
constexpr uint64_t patrol_pack(const int (&v)[PATROL_ACTIONS]) {
  uint64_t w = 0;
  for (int a = 0; a < PATROL_ACTIONS; ++a) w |= (uint64_t)(v[a] + 1) << (2 * a);
  return w;
}
constexpr int PATROL_MX_OF[PATROL_ACTIONS] = {0, 0, 0, 1, -1, 0, 1, -1, 1, -1, 0, 1, -1, 0, 1, -1, 1, -1};
constexpr int PATROL_MY_OF[PATROL_ACTIONS] = {0, 0, -1, 0, 0, 1, -1, -1, 1, 1, -1, 0, 0, 1, -1, -1, 1, 1};
constexpr uint64_t PATROL_MX = patrol_pack(PATROL_MX_OF);
constexpr uint64_t PATROL_MY = patrol_pack(PATROL_MY_OF);

// The record in registers (patrol_row says what keeps it there).
struct PatrolState {
  int32_t px, py, face, lives, sx, sy, sd, steps;
  int32_t x0, x1, x2, x3, d0, d1, d2, d3;
  int32_t k;
};

// A drone sent to wait: -x steps remain, it will enter flying d.
struct PatrolDrone {
  int32_t x, d;
};
__device__ __forceinline__ PatrolDrone patrol_park(uint32_t h, uint32_t salt) {
  const uint32_t w = lowbias32(h ^ salt);
  PatrolDrone p;
  p.x = -(int32_t)(1u + (w >> 1) % PATROL_WAIT);
  p.d = (w & 1u) ? 1 : -1;
  return p;
}

// What a pixel row in board row cy can show: the column of the row's drone (-1: no lane, or the drone waits -- no cell has a
// negative column), whether craft and shot are in the row (all ones or 0), and the first of the craft's two brighter pixel
// columns within its cell.  Worked out once per quad.
struct PatrolRow {
  int dronex, nose;
  uint32_t craft, shot;
};

__device__ __forceinline__ PatrolRow patrol_row(const PatrolState& s, int cy) {
  PatrolRow r;
  const int lane = cy / 3;
  // the lane's drone by masks, not by `?:` among the four: the compiler turns such a chain into ONE load from a selected
  // address, the record then has to live in memory -- it put it into the LDS, 17 KB per workgroup, and the step took four
  // times as long
  const uint32_t x = ((uint32_t)s.x0 & -(uint32_t)(lane == 0)) | ((uint32_t)s.x1 & -(uint32_t)(lane == 1)) |
                     ((uint32_t)s.x2 & -(uint32_t)(lane == 2)) | ((uint32_t)s.x3 & -(uint32_t)(lane == 3));
  const uint32_t in_lane = -(uint32_t)(cy % 3 == 2 && cy < PATROL_CELLS - 2);
  r.dronex = (int)((x & in_lane) | ~in_lane);              // -1 outside the lanes
  r.nose = s.face > 0 ? PATROL_CELL - 2 : 0;
  r.craft = -(uint32_t)(cy == s.py);
  r.shot = -(uint32_t)(s.sd != 0 && cy == s.sy);
  return r;
}

// Pixel x of a pixel row, `row` = patrol_row(s, cy).  Masks and bitwise operations only, no branches (rally_dev.h records why).
__device__ __forceinline__ uint32_t patrol_pixel(const PatrolState& s, const PatrolRow& row, int x) {
  const int cx = x / PATROL_CELL;
  const int within = x - cx * PATROL_CELL;
  const uint32_t shot = row.shot & -(uint32_t)(cx == s.sx);
  const uint32_t craft = row.craft & -(uint32_t)(cx == s.px);
  const uint32_t nose = -(uint32_t)((uint32_t)(within - row.nose) < 2u);
  const uint32_t craftv = 128u | (nose & 96u);
  const uint32_t drone = -(uint32_t)(cx == row.dronex) & 64u;
  return (shot & 255u) | (~shot & ((craft & craftv) | (~craft & drone)));
}

// One drone as a value, the shot as three plain integers: the step below works on copies in registers and writes the record once at its end
// (pieces that updated the record's fields through references ended with part of it in scratch memory).

// The per-drone pieces of a step, for the drone q of board row `row` whose parking of this step is w.
// 3.: the craft (px, py) walked into it.
__device__ __forceinline__ PatrolDrone patrol_walked(PatrolDrone q, int row, int px, int py, PatrolDrone w, bool& hit) {
  const bool in = q.x == px && row == py;                  // (x >= 0 follows: px is)
  hit = hit || in;
  return in ? w : q;
}
// 4.: the shot flew into its cell.
__device__ __forceinline__ PatrolDrone patrol_struck(PatrolDrone q, int row, int sx, int sy, int32_t& sd, PatrolDrone w,
                                                     float& r) {
  const bool in = sd != 0 && q.x == sx && row == sy;
  r += in ? 1.f : 0.f;
  sd = in ? 0 : sd;
  return in ? w : q;
}
// 5.: it waits, enters or flies on, and may meet the shot or the craft where it arrives.
__device__ __forceinline__ PatrolDrone patrol_drone(PatrolDrone q, int row, int px, int py, int sx, int sy, int32_t& sd,
                                                    PatrolDrone w, float& r, bool& hit) {
  const bool waiting = q.x < 0;
  const int32_t moved = q.x + (waiting ? 1 : q.d);
  const bool there = waiting ? moved >= 0 : (moved >= 0 && moved <= PATROL_CELLS - 1);
  const int32_t x = (waiting && there) ? (q.d > 0 ? 0 : PATROL_CELLS - 1) : moved;
  const bool escaped = !waiting && !there;
  const bool killed = there && sd != 0 && x == sx && row == sy;
  const bool touched = there && !killed && x == px && row == py;
  r += killed ? 1.f : 0.f;
  sd = killed ? 0 : sd;
  hit = hit || touched;
  PatrolDrone out;
  out.x = x;
  out.d = q.d;
  return (escaped || killed || touched) ? w : out;
}

struct PatrolGame {
  typedef PatrolState State;
  static constexpr int kWords = 20;      // int32 words of a state record: the 17 of State, then three zeros (five 16-byte parts)
  static constexpr int kActions = PATROL_ACTIONS;
  static constexpr int kMaxSteps = PATROL_MAX_STEPS;

  static __device__ __forceinline__ State load(const int32_t* __restrict__ state, int e) {
    const int4* p = reinterpret_cast<const int4*>(state) + 5 * e;
    const int4 a = p[0], b = p[1], c = p[2], d = p[3], f = p[4];
    State s;
    s.px = a.x; s.py = a.y; s.face = a.z; s.lives = a.w;
    s.sx = b.x; s.sy = b.y; s.sd = b.z; s.steps = b.w;
    s.x0 = c.x; s.x1 = c.y; s.x2 = c.z; s.x3 = c.w;
    s.d0 = d.x; s.d1 = d.y; s.d2 = d.z; s.d3 = d.w;
    s.k = f.x;
    return s;
  }

  static __device__ __forceinline__ void store(int32_t* __restrict__ state, int e, const State& s) {
    int4* p = reinterpret_cast<int4*>(state) + 5 * e;
    p[0] = make_int4(s.px, s.py, s.face, s.lives);
    p[1] = make_int4(s.sx, s.sy, s.sd, s.steps);
    p[2] = make_int4(s.x0, s.x1, s.x2, s.x3);
    p[3] = make_int4(s.d0, s.d1, s.d2, s.d3);
    p[4] = make_int4(s.k, 0, 0, 0);
  }

  static __device__ __forceinline__ State start(uint64_t seed, uint32_t env, int32_t k = 0) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)k);
    State s;
    s.px = (int32_t)(lowbias32(h ^ 0x9A7E0001u) % (uint32_t)PATROL_CELLS);
    s.py = (int32_t)(lowbias32(h ^ 0x9A7E0002u) % (uint32_t)PATROL_CELLS);
    s.face = 1;
    s.lives = PATROL_LIVES;
    s.sx = s.sy = s.sd = s.steps = 0;
    s.k = k;
    const PatrolDrone p0 = patrol_park(h, 0x9A7E0010u), p1 = patrol_park(h, 0x9A7E0011u), p2 = patrol_park(h, 0x9A7E0012u),
                     p3 = patrol_park(h, 0x9A7E0013u);
    s.x0 = p0.x; s.x1 = p1.x; s.x2 = p2.x; s.x3 = p3.x;
    s.d0 = p0.d; s.d1 = p1.d; s.d2 = p2.d; s.d3 = p3.d;
    return s;
  }

  // One step of state s under action a (ALE's full set; any other number is NOOP), a pure function of its arguments: the state
  // the next step starts from (the next episode's start state after a terminal step), the reward and the terminal flag.
  // Everything here is the same for all threads of a workgroup (one environment per workgroup column): scalar work, and but
  // for the episode's end without a branch -- the shot's two cells of flight and the four drones are written out, every
  // outcome a select.  opt != 0: single_life, every hit ends the episode.
  // *trunc: the step is terminal only because steps reached the cap (no life lost on it ended the episode).
  static __device__ __forceinline__ State advance(uint64_t seed, uint32_t env, State s, int a, int opt, float* reward,
                                                  bool* term, bool* trunc = nullptr) {
    const uint32_t h = synth_key(seed, env, (uint64_t)(uint32_t)s.k);
    // Every parking of drone i in this step uses one salt, so it has one outcome: the four are hashed once, up front and
    // unconditionally, and a parking below is two moves.  (Every wave of the environment's 28 walks through the whole step.)
    const uint32_t salt = 0x9A7E1000u + 16u * (uint32_t)s.steps;
    const PatrolDrone w0 = patrol_park(h, salt), w1 = patrol_park(h, salt + 1u), w2 = patrol_park(h, salt + 2u),
                     w3 = patrol_park(h, salt + 3u);
    const uint32_t ua = (uint32_t)a < (uint32_t)PATROL_ACTIONS ? (uint32_t)a : 0u;
    const int mx = (int)((PATROL_MX >> (2u * ua)) & 3u) - 1;
    const int my = (int)((PATROL_MY >> (2u * ua)) & 3u) - 1;
    const bool fire = ua == 1u || ua >= 10u;
    float r = 0.f;
    bool hit = false;
    // 1. the craft
    const int face = mx != 0 ? mx : s.face;
    const int px = min(max(s.px + mx, 0), PATROL_CELLS - 1), py = min(max(s.py + my, 0), PATROL_CELLS - 1);
    // 2. a new shot
    const bool fired = fire && s.sd == 0;
    int32_t sx = fired ? px : s.sx, sd = fired ? face : s.sd;
    const int32_t sy = fired ? py : s.sy;
    PatrolDrone q0, q1, q2, q3;
    q0.x = s.x0; q0.d = s.d0; q1.x = s.x1; q1.d = s.d1; q2.x = s.x2; q2.d = s.d2; q3.x = s.x3; q3.d = s.d3;
    // 3. drones walked into
    q0 = patrol_walked(q0, 2, px, py, w0, hit);
    q1 = patrol_walked(q1, 5, px, py, w1, hit);
    q2 = patrol_walked(q2, 8, px, py, w2, hit);
    q3 = patrol_walked(q3, 11, px, py, w3, hit);
    // 4. the shot flies: SHOT_SPEED cells, one at a time (a spent shot stays where it is)
#pragma unroll
    for (int n = 0; n < PATROL_SHOT_SPEED; ++n) {
      sx += sd;                                            // (a spent shot has sd == 0)
      sd = (sx < 0 || sx > PATROL_CELLS - 1) ? 0 : sd;
      q0 = patrol_struck(q0, 2, sx, sy, sd, w0, r);
      q1 = patrol_struck(q1, 5, sx, sy, sd, w1, r);
      q2 = patrol_struck(q2, 8, sx, sy, sd, w2, r);
      q3 = patrol_struck(q3, 11, sx, sy, sd, w3, r);
    }
    // 5. the drones, in order
    q0 = patrol_drone(q0, 2, px, py, sx, sy, sd, w0, r, hit);
    q1 = patrol_drone(q1, 5, px, py, sx, sy, sd, w1, r, hit);
    q2 = patrol_drone(q2, 8, px, py, sx, sy, sd, w2, r, hit);
    q3 = patrol_drone(q3, 11, px, py, sx, sy, sd, w3, r, hit);
    s.px = px; s.py = py; s.face = face;
    s.sx = sx; s.sy = sy; s.sd = sd;
    s.x0 = q0.x; s.x1 = q1.x; s.x2 = q2.x; s.x3 = q3.x;
    s.d0 = q0.d; s.d1 = q1.d; s.d2 = q2.d; s.d3 = q3.d;
    // 6., 7.
    if (hit) {
      s.lives -= 1;
      r -= 1.f;
    }
    s.steps += 1;
    const bool dead = s.lives == 0 || (opt != 0 && hit);
    const bool over = dead || s.steps == PATROL_MAX_STEPS;
    if (trunc) *trunc = over && !dead;
    *reward = r;
    *term = over;
    if (over) s = start(seed, env, s.k + 1);               // (one return: with two, part of the record went through scratch memory)
    return s;
  }

  // Quad q of an observation with the plane of state s pushed into its history `old` (an empty one if `fresh`).  A quad may
  // straddle two cells (6 is no multiple of 4): every pixel asks for itself; what hangs on the row is worked out once.
  static __device__ __forceinline__ uint4 shift_quad(const State& s, int q, uint4 old, bool fresh) {
    int y, x;
    quad_yx(q, &y, &x);
    const PatrolRow row = patrol_row(s, y / PATROL_CELL);
    return push_plane(old, fresh, patrol_pixel(s, row, x) << 24, patrol_pixel(s, row, x + 1) << 24,
                      patrol_pixel(s, row, x + 2) << 24, patrol_pixel(s, row, x + 3) << 24);
  }
};

}  // namespace paac
