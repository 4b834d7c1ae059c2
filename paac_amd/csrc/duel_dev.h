// The duel environments on the device (spec: paac_amd/duel.py): rally played against the learner itself.  N rows = N / 2
// boards of the rally board; row e < N / 2 is the bottom player of board e, row e + N / 2 the top player of the same board, and
// each row keeps the board as seen from its own side (a top row's record is mirror(the bottom row's)).  The game trait DuelGame
// (see csrc/game_dev.h) of game_step_kernel in csrc/games.hip: a PAIRED trait -- a row's step reads its partner's action beside
// its own.  State, record, serve and pixels are rally's (rally_dev.h), unchanged.
#pragma once
#include "rally_dev.h"

namespace paac {

// The board as the other player sees it: a vertical flip (columns stay: LEFT / RIGHT mean the same for both players) with the
// paddles and the points exchanged.  An involution.  Selects only: `on` is the same for a whole workgroup.
__device__ __forceinline__ RallyState duel_mirror(const RallyState& s, bool on) {
  RallyState m = s;
  m.by = on ? RALLY_CELLS - 1 - s.by : s.by;
  m.dy = on ? -s.dy : s.dy;
  m.px = on ? s.ox : s.px;
  m.ox = on ? s.px : s.ox;
  m.mine = on ? s.theirs : s.mine;
  m.theirs = on ? s.mine : s.theirs;
  return m;
}

// The state episode k of board g starts from, in the bottom player's frame: rally's start state, the first serve towards the
// bottom player in even episodes and towards the top player in odd ones.
__device__ __forceinline__ RallyState duel_start_board(uint64_t seed, uint32_t g, int32_t k) {
  const uint32_t h = synth_key(seed, g, (uint64_t)(uint32_t)k);
  RallyState s;
  s.px = (int32_t)(lowbias32(h ^ 0xA11E0001u) % (uint32_t)(RALLY_CELLS - 1));
  s.ox = (int32_t)(lowbias32(h ^ 0xA11E0003u) % (uint32_t)(RALLY_CELLS - 1));
  s.mine = s.theirs = s.steps = 0;
  s.k = k;
  rally_serve(h, 0, (k & 1) == 0, s);
  return s;
}

struct DuelGame {
  typedef RallyState State;
  static constexpr int kWords = 12;      // rally's record
  static constexpr bool kPaired = true;  // game_step_kernel: the step takes the partner row's action too (game_dev.h)

  static __device__ __forceinline__ State load(const int32_t* __restrict__ state, int e) { return RallyGame::load(state, e); }
  static __device__ __forceinline__ void store(int32_t* __restrict__ state, int e, const State& s) {
    RallyGame::store(state, e, s);
  }

  // Row e of N: the bottom (e < N / 2) or the top player of board e % (N / 2).
  static __device__ __forceinline__ bool is_top(int e, int N) { return e >= (N >> 1); }
  static __device__ __forceinline__ int board(int e, int N) { return is_top(e, N) ? e - (N >> 1) : e; }
  static __device__ __forceinline__ int partner(int e, int N) { return is_top(e, N) ? e - (N >> 1) : e + (N >> 1); }

  // Episode 0's start record of row e of N.
  static __device__ __forceinline__ State start(uint64_t seed, uint32_t env_offset, int e, int N) {
    return duel_mirror(duel_start_board(seed, env_offset + (uint32_t)board(e, N), 0), is_top(e, N));
  }

  // One step of a row: s is the row's own record of board g (mirrored if the row is the top player), a_own the row's action,
  // a_partner the other player's.  The board is stepped in the bottom player's frame -- rally's step with the scripted
  // opponent replaced by the top player's paddle move -- and handed back in the row's.  Both rows of a board compute the same
  // board step.  Everything is the same for all threads of a workgroup (one row per workgroup column); there is no loop.
  // reward: the bottom player's for a bottom row, 0 - that for a top row (a zero stays +0.0).
  static __device__ __forceinline__ State advance(uint64_t seed, uint32_t g, State s, int a_own, int a_partner, bool top,
                                                  float* reward, bool* term, bool* trunc) {
    s = duel_mirror(s, top);
    const int a_bottom = top ? a_partner : a_own, a_top = top ? a_own : a_partner;
    const uint32_t h = synth_key(seed, g, (uint64_t)(uint32_t)s.k);
    if (a_bottom == 2 || a_bottom == 4) s.px = min(s.px + 1, RALLY_CELLS - 2);
    else if (a_bottom == 3 || a_bottom == 5) s.px = max(s.px - 1, 0);
    if (a_top == 2 || a_top == 4) s.ox = min(s.ox + 1, RALLY_CELLS - 2);
    else if (a_top == 3 || a_top == 5) s.ox = max(s.ox - 1, 0);
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
    *trunc = !decided && s.steps == RALLY_MAX_STEPS;
    *reward = top ? 0.f - r : r;
    *term = over;
    if (over) s = duel_start_board(seed, g, s.k + 1);
    else if (r != 0.f) rally_serve(h, s.mine + s.theirs, r < 0.f, s);
    return duel_mirror(s, top);
  }

  static __device__ __forceinline__ uint4 shift_quad(const State& s, int q, uint4 old, bool fresh) {
    return RallyGame::shift_quad(s, q, old, fresh);
  }
};

}  // namespace paac
