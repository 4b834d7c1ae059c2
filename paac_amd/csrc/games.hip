// The device games (catch, bricks, rally, duel: one trait each, csrc/game_dev.h and the game's header): the step kernel,
// GPU-resident evaluation, head-to-head matches and the duel against a pool of past selves; and, in a library built for one,
// a user's game (-DPAAC_USER_GAME): the same two kernel templates instantiated for a trait from outside the package.
#include "common.h"
#include "game_dev.h"
#include "catch_dev.h"
#include "bricks_dev.h"
#include "rally_dev.h"
#include "duel_dev.h"
// A user's game (--emulator user --device_game; paac_amd/user_game.py): one more trait, from a header outside the package,
// in a library of its own (paac_amd/build.py: build_user_game).  It obeys game_dev.h's contract for a non-paired game and
// states two numbers more: kActions (the policy's width) and kMaxSteps (the longest episode, evaluation's step budget).
#ifdef PAAC_USER_GAME
#if !defined(PAAC_USER_GAME_HEADER) || !defined(PAAC_USER_GAME_TRAIT)
#error "PAAC_USER_GAME needs PAAC_USER_GAME_HEADER (the header to include) and PAAC_USER_GAME_TRAIT (the trait struct in it)"
#endif
#include PAAC_USER_GAME_HEADER
#endif

namespace paac {

#ifdef PAAC_USER_GAME
typedef PAAC_USER_GAME_TRAIT UserGame;
template <class G, class = void>
struct declares_paired : std::false_type {};
template <class G>
struct declares_paired<G, std::void_t<decltype(G::kPaired)>> : std::true_type {};
static_assert(!declares_paired<UserGame>::value,
              "a user game must not declare kPaired: paired games (two rows per board) are not supported as user games");
static_assert(UserGame::kWords > 0 && UserGame::kWords % 4 == 0,
              "a user game's kWords must be positive and a multiple of 4 (the record is loaded in 16-byte parts)");
static_assert(UserGame::kActions >= 2 && UserGame::kActions <= 32,
              "a user game's kActions must be within [2, 32] (what paac_eval_step accepts)");
static_assert(UserGame::kMaxSteps > 0, "a user game's kMaxSteps must be positive");
#endif

// The device games (catch, bricks, rally: one trait G each, csrc/game_dev.h and the game's header).  The shape of
// synth_step_a_kernel: grid (N, 7), 256 threads, 252 of them own one quad of four pixels -- one 16-byte load of the old stack,
// requested before the state record is looked at (whether or not the step ends the episode: one round trip, not two), one
// 16-byte store (and the optional second one), no LDS.  The new state is a pure function of (state_in[e], actions[e], opt):
// every band workgroup of an environment recomputes it in registers, one thread of band 0 writes it out and does the
// bookkeeping.  Nothing in the launch writes what the launch reads: state_in / state_out and stack_in / stack_out are different
// buffers.  state_in == nullptr: reset -- episode 0's start state, an empty history; actions / stack_in / the records are not
// touched.
// A paired game (duel: game_dev.h, duel_dev.h) widens that contract by one word: the new state of row e is a pure function of
// (state_in[e], actions[e], actions[partner of e]) -- one more 4-byte load beside the own action's, of a value the launch
// before this one wrote; N is even.  Still no row writes what another row reads, no atomics, no LDS.
//
// Sticky actions (--sticky_action_p; spec: paac_amd/sticky.py): the compile-time form kSticky of the two step kernels.  With
// probability p the environment executes the action it executed on its previous step instead of the one chosen: one Philox
// block per row and step, counter {g, t lo, t hi, stream}, key the seed, g = env_offset + ROW (a paired game's two players
// stick independently), t = *step_base + step_off.  The previous action is one more 4-byte load per row, from prev_in, asked
// for beside the action's; every band workgroup recomputes draw and executed action in registers; thread 0 of band 0 stores
// prev_out[e] (and prev_out2[e], the ring's wrap-around slot) = 0 after a terminal step, else the executed action.  prev_in is
// never prev_out or prev_out2: nothing the launch reads is written by it.  The plain form (kSticky = false) takes the
// arguments it always took and is the code it always was: the sticky form's arguments ride in the TYPE of the last one.
// paac_amd/sticky.py: STICKY_STREAM / EVAL_STREAM_STICKY are the same numbers.
constexpr uint32_t kStickyStream = 0x53544B01u;
constexpr uint32_t kEvalStreamSticky = 0x45560004u;

// The executed action of row g at step t: `prev` where the draw sticks, else `chosen`.  p = 0 never sticks (u >= 0).
__device__ __forceinline__ int sticky_action(int chosen, int prev, float p, uint64_t seed, uint32_t g, uint64_t t,
                                             uint32_t stream) {
  uint32_t c[4] = {g, (uint32_t)t, (uint32_t)(t >> 32), stream};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
  return u < p ? prev : chosen;
}

// What a sticky training step takes beyond the plain one's arguments (include/paac_hip.h: paac_sticky).
struct StickyStep {
  float p;
  const uint64_t* step_base;
  uint64_t step_off;
  const int32_t* prev_in;
  int32_t* prev_out;
  int32_t* prev_out2;
};
struct StickyOpt {
  int opt;
  StickyStep st;
};
// game_step_kernel's last argument: the game's integer option, with the sticky block behind it in the sticky form.
template <bool kSticky>
struct step_tail {
  typedef int type;
};
template <>
struct step_tail<true> {
  typedef StickyOpt type;
};

template <class G, bool kSticky = false>
__global__ __launch_bounds__(256) void game_step_kernel(uint64_t seed, uint32_t env_offset, int N,
                                                        const int32_t* __restrict__ actions,
                                                        const int32_t* __restrict__ state_in, int32_t* __restrict__ state_out,
                                                        int32_t* __restrict__ state_out2,
                                                        const uint32_t* __restrict__ stack_in, uint32_t* __restrict__ stack_out,
                                                        uint32_t* __restrict__ stack_out2, const EnvRecords rec,
                                                        const typename step_tail<kSticky>::type tail) {
  const QuadThread t = quad_thread();
  const int e = t.e;
  uint4 old = make_uint4(0u, 0u, 0u, 0u);
  typename G::State s;
  float r = 0.f;
  bool term = false, trunc = false;
  int opt, executed = 0;
  if constexpr (kSticky) opt = tail.opt;
  else opt = tail;
  if (state_in) {
    // every thread loads (the four that own no quad read the band's first one): with the load under a condition the compiler
    // pulls the history's shift up behind it, and with the shift the wait -- the state record would be asked for only then
    old = reinterpret_cast<const uint4*>(stack_in)[t.load_quad];
    if constexpr (kSticky) {
      // everything the step reads is asked for here, before the draws: the actions and the previous actions of the row (and
      // of its partner), the tick and the state record -- one round trip
      const StickyStep& st = tail.st;
      const uint64_t tk = (st.step_base ? *st.step_base : 0ull) + st.step_off;
      const typename G::State s0 = G::load(state_in, e);
      const int chosen = actions[e], prev = st.prev_in[e];
      if constexpr (game_is_paired<G>::value) {
        // the partner's executed action by the same device function on the partner's own row key: both rows of a board hold
        // the same pair bit for bit (match_step_kernel's way with the partner's action)
        const int pe = G::partner(e, N);
        const int chosen_p = actions[pe], prev_p = st.prev_in[pe];
        executed = sticky_action(chosen, prev, st.p, seed, env_offset + (uint32_t)e, tk, kStickyStream);
        const int executed_p = sticky_action(chosen_p, prev_p, st.p, seed, env_offset + (uint32_t)pe, tk, kStickyStream);
        s = G::advance(seed, env_offset + (uint32_t)G::board(e, N), s0, executed, executed_p, G::is_top(e, N), &r, &term, &trunc);
      } else {
        executed = sticky_action(chosen, prev, st.p, seed, env_offset + (uint32_t)e, tk, kStickyStream);
        s = G::advance(seed, env_offset + (uint32_t)e, s0, executed, opt, &r, &term, &trunc);
      }
    } else if constexpr (game_is_paired<G>::value) {
      // a paired game (game_dev.h): the other player's action too -- the sampler's launch wrote both before this one started
      s = G::advance(seed, env_offset + (uint32_t)G::board(e, N), G::load(state_in, e), actions[e], actions[G::partner(e, N)],
                     G::is_top(e, N), &r, &term, &trunc);
    } else {
      s = G::advance(seed, env_offset + (uint32_t)e, G::load(state_in, e), actions[e], opt, &r, &term, &trunc);
    }
  } else {
    if constexpr (game_is_paired<G>::value) s = G::start(seed, env_offset, e, N);
    else s = G::start(seed, env_offset + (uint32_t)e);
  }
  if (t.band == 0 && t.i == 0) {
    G::store(state_out, e, s);
    if (state_out2) G::store(state_out2, e, s);
    if (state_in) {
      env_bookkeep(r, term, e, rec.ep_reward[e], rec.ep_len[e], rec);
      if (rec.truncs) rec.truncs[e] = trunc ? 1.f : 0.f;     // --bootstrap_truncated: why the episode ended (game_dev.h)
      if constexpr (kSticky) {
        const int keep = term ? 0 : executed;                // the first step of an episode has no previous action: the no-op
        tail.st.prev_out[e] = keep;
        if (tail.st.prev_out2) tail.st.prev_out2[e] = keep;
      }
    }
  }
  if (!t.owner) return;
  const uint4 outv = G::shift_quad(s, t.q, old, term);     // a terminal step drops the history it loaded
  reinterpret_cast<uint4*>(stack_out)[t.quad] = outv;
  if (stack_out2) reinterpret_cast<uint4*>(stack_out2)[t.quad] = outv;   // second copy (the observation ring's wrap-around slot)
}

// =============================================================================================
// GPU-resident evaluation (spec: paac_amd/evaluation.py): one evaluation step of N environments of a stateful game per launch
// -- the action is chosen from the acting forward's probs, the game advances, the first scored episode is accounted.  The
// shape of game_step_kernel above: grid (N, 7), 256 threads, 252 of them own one quad; the stack load is requested first (by
// every thread, game_step_kernel's reason), then the action and the new state are worked out in registers by every band
// workgroup of the environment -- both are pure functions of (probs[e], state_in[e], t) -- and thread 0 of band 0 writes the
// record, the action and the accounts.  state_in / stack_in are never state_out / stack_out; score / length / done of
// environment e are read and written by that one thread only.  A finished environment keeps being stepped (parking it would
// make every band read `done`, which band 0 writes): nothing of that shows in score / length / done.
// The two Philox streams of an evaluation (counter word 3); the rollout sampler's is 0, the minibatch shuffles' are
// 0x504D0000 + epoch.  paac_amd/evaluation.py: EVAL_STREAM_ACTION / EVAL_STREAM_NOOP are the same numbers.
constexpr uint32_t kEvalStreamAction = 0x45560001u;
constexpr uint32_t kEvalStreamNoop = 0x45560002u;

// The sticky form (kSticky, see game_step_kernel): the draw's stream is kEvalStreamSticky, its key the evaluation's seed, its
// step the evaluation step t, no-op steps included (there the chosen action is 0 and so is the previous one).  actions_out
// keeps the CHOSEN action: the trace replays through wrapped twins, which draw again.
struct StickyAlive {
  int32_t* alive;
  float p;
  const int32_t* prev_in;
  int32_t* prev_out;
};
// eval_step_kernel's last argument: the alive counter, with the sticky arguments behind it in the sticky form.
template <bool kSticky>
struct eval_tail {
  typedef int32_t* type;
};
template <>
struct eval_tail<true> {
  typedef StickyAlive type;
};

template <class G, bool kSticky = false>
__global__ __launch_bounds__(256) void eval_step_kernel(const float* __restrict__ probs, int A, int greedy, uint64_t eval_seed,
                                                        int noops, const uint64_t* __restrict__ step_base, uint64_t step_off,
                                                        uint64_t env_seed, uint32_t env_offset, int N,
                                                        const int32_t* __restrict__ state_in, int32_t* __restrict__ state_out,
                                                        const uint32_t* __restrict__ stack_in, uint32_t* __restrict__ stack_out,
                                                        int32_t* __restrict__ actions_out, float* score, int32_t* length,
                                                        int32_t* done, const typename eval_tail<kSticky>::type tail) {
  const QuadThread th = quad_thread();
  const int e = th.e;
  // every thread loads (the four that own no quad read the band's first one): see game_step_kernel
  const uint4 old = reinterpret_cast<const uint4*>(stack_in)[th.load_quad];
  int32_t* alive;
  int prev = 0;
  if constexpr (kSticky) {
    alive = tail.alive;
    prev = tail.prev_in[e];                                  // asked for up front, beside the probabilities
  } else {
    alive = tail;
  }
  const uint32_t g = env_offset + (uint32_t)e;
  const uint64_t t = (step_base ? *step_base : 0ull) + step_off;
  uint32_t noops_e = 0u;
  if (noops > 0) {
    uint32_t c[4] = {g, 0u, 0u, kEvalStreamNoop};
    philox4x32_10(c, (uint32_t)eval_seed, (uint32_t)(eval_seed >> 32));
    noops_e = c[0] % ((uint32_t)noops + 1u);
  }
  const bool playing = t >= (uint64_t)noops_e;
  int act = 0;                                             // the no-op of every game
  if (playing) {
    const float* __restrict__ p = probs + (long)e * A;
    if (greedy) {
      float best = p[0];
      for (int j = 1; j < A; ++j) {
        const float v = p[j];
        if (v > best) {                                    // strictly: the lowest index wins a tie
          best = v;
          act = j;
        }
      }
    } else {
      uint32_t c[4] = {g, (uint32_t)t, (uint32_t)(t >> 32), kEvalStreamAction};
      philox4x32_10(c, (uint32_t)eval_seed, (uint32_t)(eval_seed >> 32));
      const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
      act = A - 1;
      float cum = 0.f;
      for (int j = 0; j < A - 1; ++j) {
        cum += p[j];
        if (u < cum) {
          act = j;
          break;
        }
      }
    }
  }
  float r = 0.f;
  bool term = false;
  int executed = act;
  if constexpr (kSticky) executed = sticky_action(act, prev, tail.p, eval_seed, g, t, kEvalStreamSticky);
  // evaluation plays whole episodes: opt = 0 (bricks' single_life is off)
  const typename G::State s = G::advance(env_seed, g, G::load(state_in, e), executed, 0, &r, &term);
  if (th.band == 0 && th.i == 0) {
    G::store(state_out, e, s);
    actions_out[e] = act;
    if constexpr (kSticky) tail.prev_out[e] = term ? 0 : executed;
    if (playing && done[e] == 0) {                         // the first episode that starts after the no-ops, its last step included
      score[e] += r;
      length[e] += 1;
      if (term) {
        done[e] = 1;
        atomicSub(alive, 1);
      }
    }
  }
  if (!th.owner) return;
  reinterpret_cast<uint4*>(stack_out)[th.quad] = G::shift_quad(s, th.q, old, term);
}

// =============================================================================================
// Head-to-head matches (spec: paac_amd/match.py): one step of N rows = N / 2 duel boards per launch, two policies' probs in
// one [N, 6] block -- rows [0, N / 2) the bottom players', rows [N / 2, N) the top players'.  eval_step_kernel's shape and
// reasons: grid (N, 7), 256 threads, 252 own one quad, the stack load requested first by every thread, one 16-byte store, no
// LDS.  Every band workgroup of row e works out, uniformly and in registers, the board's no-op count, its own action from
// probs[e] and its partner's from probs[partner] -- the same device function on the other stream, so both rows of a board hold
// the same pair bit for bit -- and the new record (DuelGame::advance).  Thread 0 of band 0 writes the record, the row's own
// action and the row's accounts; `alive` counts ROWS.  Nothing the launch reads is written by it: no row writes what another
// row reads (the partner's probs are the forward's output, the partner's action is recomputed, not loaded).
// The top player's Philox stream; the bottom player's is kEvalStreamAction, so the bottom rows' actions are an evaluation's.
// paac_amd/match.py: MATCH_STREAM_TOP is the same number.
constexpr uint32_t kMatchStreamTop = 0x45560003u;

constexpr int kMatchActions = 6;          // the duel board's (paac_match_step refuses any other A)

// One row of probs in registers: six unconditional loads, so that both rows of a board are asked for before anything is
// computed on either (uniform in the workgroup: scalar loads).
struct MatchRow {
  float p[kMatchActions];
};
__device__ __forceinline__ MatchRow match_row(const float* __restrict__ probs, int e) {
  MatchRow row;
#pragma unroll
  for (int j = 0; j < kMatchActions; ++j) row.p[j] = probs[(long)e * kMatchActions + j];
  return row;
}

// evaluation.eval_action's two rules on one row of probs: the action of board g at step t on `stream`.  (A restatement of the
// choice inside eval_step_kernel, kept beside it rather than shared with it: that kernel's device code stays as it was.)
// Unrolled and without an early exit: the running sums are the same float32 additions in the same order, and the first hit
// keeps the action.
__device__ __forceinline__ int match_action(const MatchRow& row, int greedy, uint64_t seed, uint32_t g, uint64_t t,
                                            uint32_t stream) {
  int act = 0;
  if (greedy) {
    float best = row.p[0];
#pragma unroll
    for (int j = 1; j < kMatchActions; ++j) {
      const float v = row.p[j];
      if (v > best) {                                      // strictly: the lowest index wins a tie
        best = v;
        act = j;
      }
    }
  } else {
    uint32_t c[4] = {g, (uint32_t)t, (uint32_t)(t >> 32), stream};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);
    act = kMatchActions - 1;
    bool chosen = false;
    float cum = 0.f;
#pragma unroll
    for (int j = 0; j < kMatchActions - 1; ++j) {
      cum += row.p[j];
      if (!chosen && u < cum) {
        act = j;
        chosen = true;
      }
    }
  }
  return act;
}

__global__ __launch_bounds__(256) void match_step_kernel(const float* __restrict__ probs, int greedy, uint64_t eval_seed,
                                                         int noops, const uint64_t* __restrict__ step_base, uint64_t step_off,
                                                         uint64_t env_seed, uint32_t env_offset, int N,
                                                         const int32_t* __restrict__ state_in, int32_t* __restrict__ state_out,
                                                         const uint32_t* __restrict__ stack_in, uint32_t* __restrict__ stack_out,
                                                         int32_t* __restrict__ actions_out, float* score, int32_t* length,
                                                         int32_t* done, int32_t* alive) {
  typedef DuelGame G;
  const QuadThread th = quad_thread();
  const int e = th.e;
  // every thread loads (the four that own no quad read the band's first one): see game_step_kernel
  const uint4 old = reinterpret_cast<const uint4*>(stack_in)[th.load_quad];
  const bool top = G::is_top(e, N);
  // everything the step reads is asked for here, whether or not the board is past its no-ops: one round trip to memory, not
  // one per player behind the no-op count
  const uint64_t t = (step_base ? *step_base : 0ull) + step_off;
  const MatchRow own = match_row(probs, e), other = match_row(probs, G::partner(e, N));
  const G::State s0 = G::load(state_in, e);
  const uint32_t g = env_offset + (uint32_t)G::board(e, N);          // the BOARD's key: no-ops and both streams hang on it
  uint32_t noops_g = 0u;
  if (noops > 0) {
    uint32_t c[4] = {g, 0u, 0u, kEvalStreamNoop};
    philox4x32_10(c, (uint32_t)eval_seed, (uint32_t)(eval_seed >> 32));
    noops_g = c[0] % ((uint32_t)noops + 1u);
  }
  const bool playing = t >= (uint64_t)noops_g;
  int a_own = 0, a_partner = 0;                            // the no-op, for both players of the board
  if (playing) {
    a_own = match_action(own, greedy, eval_seed, g, t, top ? kMatchStreamTop : kEvalStreamAction);
    a_partner = match_action(other, greedy, eval_seed, g, t, top ? kEvalStreamAction : kMatchStreamTop);
  }
  float r = 0.f;
  bool term = false, trunc = false;
  const G::State s = G::advance(env_seed, g, s0, a_own, a_partner, top, &r, &term, &trunc);
  if (th.band == 0 && th.i == 0) {
    G::store(state_out, e, s);
    actions_out[e] = a_own;
    if (playing && done[e] == 0) {                         // the first episode that starts after the no-ops, its last step included
      score[e] += r;
      length[e] += 1;
      if (term) {
        done[e] = 1;
        atomicSub(alive, 1);
      }
    }
  }
  if (!th.owner) return;
  reinterpret_cast<uint4*>(stack_out)[th.quad] = G::shift_quad(s, th.q, old, term);
}

// =============================================================================================
// Duel against a pool of past selves (spec: paac_amd/duel_pool.py): one training step of N BOARDS per launch.  Every learner
// row is the bottom player of its own board; the top player is a ghost, a row of a frozen earlier copy of the policy, whose
// probabilities ghost_probs [N, 6] a second context's forward wrote.  The shape and reasons of the kernels above: grid (2N, 7),
// 256 threads, 252 own one quad, the stack quad requested first by every thread, one 16-byte store (and the optional wrap
// store), no LDS.  Workgroup column e < N is the learner row of board e, column e >= N the ghost of board e - N.  Every
// workgroup of board b asks up front for state_in[b] -- the board in the bottom player's frame, the only record kept --
// actions[b], the six floats of ghost_probs[b] (uniform: scalar loads) and the tick, works out the ghost's action (always
// sampled: match_action's inverse CDF on one Philox block, counter {g, t lo, t hi, kGhostStream}, key the sampler's seed) and
// the board step (DuelGame::advance as a bottom row).  A learner column does what game_step_kernel<DuelGame> does for a bottom
// row, and thread 0 of its band 0 also writes the ghost's action (the plane a rollout is replayed from).  A ghost column pushes
// the plane of duel_mirror(new record) -- in registers, never stored -- into the ghost's stack and writes nothing else; a
// terminal step drops the history on both sides.  Nothing the launch writes is read by it.
// state_in == nullptr: reset -- episode 0's start board, an empty history on both sides; actions / ghost_probs / the stacks
// read / the records / ghost_actions_out are not touched.
// paac_amd/duel_pool.py: GHOST_STREAM is the same number.
constexpr uint32_t kGhostStream = 0x44500001u;

__global__ __launch_bounds__(256) void ghost_step_kernel(uint64_t seed, uint32_t env_offset, int N,
                                                         const int32_t* __restrict__ actions,
                                                         const float* __restrict__ ghost_probs, uint64_t sampler_seed,
                                                         const uint64_t* __restrict__ step_base, uint64_t step_off,
                                                         const int32_t* __restrict__ state_in, int32_t* __restrict__ state_out,
                                                         int32_t* __restrict__ state_out2,
                                                         const uint32_t* __restrict__ stack_in, uint32_t* __restrict__ stack_out,
                                                         uint32_t* __restrict__ stack_out2,
                                                         const uint32_t* __restrict__ ghost_stack_in,
                                                         uint32_t* __restrict__ ghost_stack_out,
                                                         uint32_t* __restrict__ ghost_stack_out2, const EnvRecords rec,
                                                         int32_t* __restrict__ ghost_actions_out) {
  typedef DuelGame G;
  const QuadThread th = quad_thread();
  const bool ghost = th.e >= N;                            // uniform in the workgroup
  const int b = ghost ? th.e - N : th.e;
  // the column's own stack buffers hold N rows each: the quad indices count from the board, not from the column
  const long shift = ghost ? (long)N * (OBS_PIX / 4) : 0l;
  uint4 old = make_uint4(0u, 0u, 0u, 0u);
  G::State s;
  float r = 0.f;
  bool term = false, trunc = false;
  int a_ghost = 0;
  const uint32_t g = env_offset + (uint32_t)b;             // the BOARD's key
  if (state_in) {
    // every thread loads (the four that own no quad read the band's first one): see game_step_kernel
    old = reinterpret_cast<const uint4*>(ghost ? ghost_stack_in : stack_in)[th.load_quad - shift];
    const uint64_t t = (step_base ? *step_base : 0ull) + step_off;
    const MatchRow probs = match_row(ghost_probs, b);
    const G::State s0 = G::load(state_in, b);
    const int a_learner = actions[b];
    a_ghost = match_action(probs, 0, sampler_seed, g, t, kGhostStream);
    s = G::advance(seed, g, s0, a_learner, a_ghost, /*top=*/false, &r, &term, &trunc);
  } else {
    s = duel_start_board(seed, g, 0);
  }
  if (!ghost && th.band == 0 && th.i == 0) {
    G::store(state_out, b, s);
    if (state_out2) G::store(state_out2, b, s);
    if (state_in) {
      env_bookkeep(r, term, b, rec.ep_reward[b], rec.ep_len[b], rec);
      if (rec.truncs) rec.truncs[b] = trunc ? 1.f : 0.f;
      ghost_actions_out[b] = a_ghost;
    }
  }
  if (!th.owner) return;
  // the ghost sees the board from the top: the mirrored record's plane (selects only: `ghost` is uniform)
  const uint4 outv = RallyGame::shift_quad(duel_mirror(s, ghost), th.q, old, term);
  uint32_t* __restrict__ out = ghost ? ghost_stack_out : stack_out;
  uint32_t* __restrict__ out2 = ghost ? ghost_stack_out2 : stack_out2;
  reinterpret_cast<uint4*>(out)[th.quad - shift] = outv;
  if (out2) reinterpret_cast<uint4*>(out2)[th.quad - shift] = outv;   // second copy (the observation ring's wrap-around slot)
}

// paac_<game>_reset / paac_<game>_step of the device games: `name` is the entry point's, for the messages.
template <class G>
static int game_reset(const char* name, uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                      paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && state_out && stack_out, "%s: bad arguments", name);
  hipLaunchKernelGGL(game_step_kernel<G>, dim3(N, PRE_BANDS), dim3(256), 0, (hipStream_t)stream, seed, env_offset, N,
                     (const int32_t*)nullptr, (const int32_t*)nullptr, state_out, (int32_t*)nullptr, (const uint32_t*)nullptr,
                     (uint32_t*)stack_out, (uint32_t*)nullptr, EnvRecords{}, 0);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

template <class G>
static int game_step(const char* name, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions,
                     const int32_t* state_in, int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in,
                     uint8_t* stack_out, uint8_t* stack_out2, const EnvRecords& rec, int opt, paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && actions && state_in && state_out && stack_in && stack_out && rec.rewards && rec.masks && rec.ep_reward &&
               rec.ep_len, "%s: bad arguments", name);
  PAAC_REQUIRE(state_in != state_out && state_in != state_out2 && stack_in != stack_out && stack_in != stack_out2,
               "%s: the step cannot run in place (every band workgroup of an environment reads state_in)", name);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
  launch_k(game_step_kernel<G>, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, seed, env_offset, N, actions, state_in, state_out,
           state_out2, (const uint32_t*)stack_in, (uint32_t*)stack_out, (uint32_t*)stack_out2, rec, opt);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// What the sticky entries refuse about their own arguments, in the name of the entry: p outside [0, 1) (a NaN fails both
// comparisons), a null plane, a plane read and written by one launch.
static int sticky_check(const char* name, float p, const int32_t* prev_in, const int32_t* prev_out, const int32_t* prev_out2) {
  PAAC_REQUIRE(p >= 0.f && p < 1.f, "%s: sticky p=%g is outside [0, 1)", name, (double)p);
  PAAC_REQUIRE(prev_in && prev_out, "%s: null prev_in / prev_out", name);
  PAAC_REQUIRE(prev_in != prev_out && prev_in != prev_out2,
               "%s: prev_in is prev_out or prev_out2: the step cannot run in place (every band workgroup of an environment "
               "reads prev_in)", name);
  return 0;
}

// game_step with sticky actions: the same refusals, then the sticky block's, then game_step_kernel's sticky form.
template <class G>
static int game_step_sticky(const char* name, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions,
                            const int32_t* state_in, int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in,
                            uint8_t* stack_out, uint8_t* stack_out2, const EnvRecords& rec, int opt, const paac_sticky* sticky,
                            paac_stream_t stream) {
  PAAC_REQUIRE(N > 0 && actions && state_in && state_out && stack_in && stack_out && rec.rewards && rec.masks && rec.ep_reward &&
               rec.ep_len, "%s: bad arguments", name);
  PAAC_REQUIRE(state_in != state_out && state_in != state_out2 && stack_in != stack_out && stack_in != stack_out2,
               "%s: the step cannot run in place (every band workgroup of an environment reads state_in)", name);
  PAAC_REQUIRE(sticky, "%s: null sticky block", name);
  if (int rc = sticky_check(name, sticky->p, sticky->prev_in, sticky->prev_out, sticky->prev_out2)) return rc;
  const StickyOpt tail = {opt, {sticky->p, sticky->step_base_dev, sticky->step_offset, sticky->prev_in, sticky->prev_out,
                                sticky->prev_out2}};
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
  launch_k(game_step_kernel<G, true>, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, seed, env_offset, N, actions, state_in,
           state_out, state_out2, (const uint32_t*)stack_in, (uint32_t*)stack_out, (uint32_t*)stack_out2, rec, tail);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// The records of a step as the kernels take them: from the five pointers of a per-game entry (no truncation plane), or from
// the public block.
static EnvRecords env_records_of(float* rewards, float* masks, float* ep_reward, int32_t* ep_len, void* finished,
                                 float* truncs = nullptr) {
  return EnvRecords{{rewards, masks, ep_reward, ep_len, (FinishedRing*)finished}, truncs};
}
static EnvRecords env_records_of(const paac_env_records* rec) {
  return env_records_of(rec->rewards, rec->masks, rec->ep_reward, rec->ep_len, rec->finished, rec->truncs);
}

// A stateful game by its PAAC_EVAL_* id: f(G{}, opt) with the game's trait and its one integer option -- bricks gets `option`
// (its single_life), the others 0.  Any other id is refused in the name of the entry `fn`.
template <class F>
static int with_game(const char* fn, int game, int option, F&& f) {
#ifdef PAAC_USER_GAME
  // a user-game library: the user's game (its option passed through, as bricks') beside the three
  PAAC_REQUIRE(game == PAAC_EVAL_CATCH || game == PAAC_EVAL_BRICKS || game == PAAC_EVAL_RALLY || game == PAAC_EVAL_USER,
               "%s: game %d is none of catch (%d), bricks (%d), rally (%d), the user game (%d)", fn, game, PAAC_EVAL_CATCH,
               PAAC_EVAL_BRICKS, PAAC_EVAL_RALLY, PAAC_EVAL_USER);
  if (game == PAAC_EVAL_USER) return f(UserGame{}, option);
#endif
  PAAC_REQUIRE(game == PAAC_EVAL_CATCH || game == PAAC_EVAL_BRICKS || game == PAAC_EVAL_RALLY,
               "%s: game %d is none of catch (%d), bricks (%d), rally (%d)", fn, game, PAAC_EVAL_CATCH, PAAC_EVAL_BRICKS,
               PAAC_EVAL_RALLY);
  if (game == PAAC_EVAL_CATCH) return f(CatchGame{}, 0);
  if (game == PAAC_EVAL_BRICKS) return f(BricksGame{}, option);
  return f(RallyGame{}, 0);
}

}  // namespace paac

using namespace paac;

// =============================================================================================
// C-ABI wrappers
extern "C" {

int paac_catch_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                     paac_stream_t stream) {
  return game_reset<CatchGame>("paac_catch_reset", seed, env_offset, N, state_out, stack_out, stream);
}

int paac_catch_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                    int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                    float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                    paac_stream_t stream) {
  return game_step<CatchGame>("paac_catch_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in, stack_out,
                              stack_out2, env_records_of(rewards_out, masks_out, ep_reward, ep_len, finished), 0, stream);
}

int paac_bricks_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                      paac_stream_t stream) {
  return game_reset<BricksGame>("paac_bricks_reset", seed, env_offset, N, state_out, stack_out, stream);
}

int paac_bricks_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                     int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                     float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished, int single_life,
                     paac_stream_t stream) {
  return game_step<BricksGame>("paac_bricks_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in, stack_out,
                               stack_out2, env_records_of(rewards_out, masks_out, ep_reward, ep_len, finished), single_life, stream);
}

int paac_rally_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                     paac_stream_t stream) {
  return game_reset<RallyGame>("paac_rally_reset", seed, env_offset, N, state_out, stack_out, stream);
}

int paac_rally_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                    int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                    float* rewards_out, float* masks_out, float* ep_reward, int32_t* ep_len, void* finished,
                    paac_stream_t stream) {
  return game_step<RallyGame>("paac_rally_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in, stack_out,
                              stack_out2, env_records_of(rewards_out, masks_out, ep_reward, ep_len, finished), 0, stream);
}

// Duel: rally against the learner itself, two rows per board (csrc/duel_dev.h).  The records come as paac_game_step's block.
int paac_duel_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                    paac_stream_t stream) {
  PAAC_REQUIRE(N >= 2 && N % 2 == 0, "paac_duel_reset: N=%d is not an even number of rows >= 2 (two rows per board)", N);
  return game_reset<DuelGame>("paac_duel_reset", seed, env_offset, N, state_out, stack_out, stream);
}

int paac_duel_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                   int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                   const paac_env_records* rec, paac_stream_t stream) {
  PAAC_REQUIRE(N >= 2 && N % 2 == 0, "paac_duel_step: N=%d is not an even number of rows >= 2 (two rows per board)", N);
  PAAC_REQUIRE(rec, "paac_duel_step: null records");
  return game_step<DuelGame>("paac_duel_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in, stack_out,
                             stack_out2, env_records_of(rec), 0, stream);
}

// The user's game (--emulator user --device_game): the same launchers on the user's trait; the stock library has none.
int paac_user_game_info(int* words, int* actions, int* max_steps) {
#ifdef PAAC_USER_GAME
  if (words) *words = UserGame::kWords;
  if (actions) *actions = UserGame::kActions;
  if (max_steps) *max_steps = UserGame::kMaxSteps;
  return 1;
#else
  if (words) *words = 0;
  if (actions) *actions = 0;
  if (max_steps) *max_steps = 0;
  return 0;
#endif
}

int paac_user_game_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                         paac_stream_t stream) {
#ifdef PAAC_USER_GAME
  return game_reset<UserGame>("paac_user_game_reset", seed, env_offset, N, state_out, stack_out, stream);
#else
  PAAC_REQUIRE(false, "paac_user_game_reset: this library was built without a user game (--device_game builds one)");
  return -1;
#endif
}

int paac_user_game_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                        int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                        uint8_t* stack_out2, const paac_env_records* rec, int option, paac_stream_t stream) {
#ifdef PAAC_USER_GAME
  PAAC_REQUIRE(rec, "paac_user_game_step: null records");
  return game_step<UserGame>("paac_user_game_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in,
                             stack_out, stack_out2, env_records_of(rec), option, stream);
#else
  PAAC_REQUIRE(false, "paac_user_game_step: this library was built without a user game (--device_game builds one)");
  return -1;
#endif
}

// paac_<game>_step by the game's id, with the records as one block -- the truncation plane among them.
int paac_game_step(int game, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                   int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out, uint8_t* stack_out2,
                   const paac_env_records* rec, int option, paac_stream_t stream) {
  return with_game("paac_game_step", game, option, [&](auto g, int opt) {
    PAAC_REQUIRE(rec, "paac_game_step: null records");
    return game_step<decltype(g)>("paac_game_step", seed, env_offset, N, actions, state_in, state_out, state_out2, stack_in,
                                  stack_out, stack_out2, env_records_of(rec), opt, stream);
  });
}

// Sticky actions (spec: paac_amd/sticky.py): paac_game_step / paac_duel_step / paac_eval_step with the sticky arguments
// behind their lists -- the plain entries' refusals, then sticky_check's, then the kernels' sticky forms.
int paac_game_step_sticky(int game, uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                          int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                          uint8_t* stack_out2, const paac_env_records* rec, int option, const paac_sticky* sticky,
                          paac_stream_t stream) {
  return with_game("paac_game_step_sticky", game, option, [&](auto g, int opt) {
    PAAC_REQUIRE(rec, "paac_game_step_sticky: null records");
    return game_step_sticky<decltype(g)>("paac_game_step_sticky", seed, env_offset, N, actions, state_in, state_out, state_out2,
                                         stack_in, stack_out, stack_out2, env_records_of(rec), opt, sticky, stream);
  });
}

int paac_duel_step_sticky(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const int32_t* state_in,
                          int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                          uint8_t* stack_out2, const paac_env_records* rec, const paac_sticky* sticky, paac_stream_t stream) {
  PAAC_REQUIRE(N >= 2 && N % 2 == 0, "paac_duel_step_sticky: N=%d is not an even number of rows >= 2 (two rows per board)", N);
  PAAC_REQUIRE(rec, "paac_duel_step_sticky: null records");
  return game_step_sticky<DuelGame>("paac_duel_step_sticky", seed, env_offset, N, actions, state_in, state_out, state_out2,
                                    stack_in, stack_out, stack_out2, env_records_of(rec), 0, sticky, stream);
}

int paac_eval_step_sticky(int game, const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops,
                          const uint64_t* step_base_dev, uint64_t step_offset, uint64_t env_seed, uint32_t env_offset,
                          const int32_t* state_in, int32_t* state_out, const uint8_t* stack_in, uint8_t* stack_out,
                          int32_t* actions_out, float* score, int32_t* length, int32_t* done, int32_t* alive, float p,
                          const int32_t* prev_in, int32_t* prev_out, paac_stream_t stream) {
  return with_game("paac_eval_step_sticky", game, 0, [&](auto g, int) {
    PAAC_REQUIRE(N > 0, "paac_eval_step_sticky: N=%d", N);
    PAAC_REQUIRE(A >= 2 && A <= 32, "paac_eval_step_sticky: A=%d outside [2, 32]", A);
    PAAC_REQUIRE(noops >= 0, "paac_eval_step_sticky: noops=%d is negative", noops);
    PAAC_REQUIRE(probs && state_in && state_out && stack_in && stack_out && actions_out && score && length && done && alive,
                 "paac_eval_step_sticky: bad arguments");
    PAAC_REQUIRE(state_in != state_out && stack_in != stack_out,
                 "paac_eval_step_sticky: the step cannot run in place (every band workgroup of an environment reads state_in)");
    if (int rc = sticky_check("paac_eval_step_sticky", p, prev_in, prev_out, nullptr)) return rc;
    const StickyAlive tail = {alive, p, prev_in, prev_out};
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
    launch_k(eval_step_kernel<decltype(g), true>, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, probs, A, greedy, eval_seed,
             noops, step_base_dev, step_offset, env_seed, env_offset, N, state_in, state_out, (const uint32_t*)stack_in,
             (uint32_t*)stack_out, actions_out, score, length, done, tail);
    PAAC_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

int paac_eval_step(int game, const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops,
                   const uint64_t* step_base_dev, uint64_t step_offset, uint64_t env_seed, uint32_t env_offset,
                   const int32_t* state_in, int32_t* state_out, const uint8_t* stack_in, uint8_t* stack_out, int32_t* actions_out,
                   float* score, int32_t* length, int32_t* done, int32_t* alive, paac_stream_t stream) {
  // (evaluation plays whole episodes: no option reaches the kernel)
  return with_game("paac_eval_step", game, 0, [&](auto g, int) {
    PAAC_REQUIRE(N > 0, "paac_eval_step: N=%d", N);
    PAAC_REQUIRE(A >= 2 && A <= 32, "paac_eval_step: A=%d outside [2, 32]", A);
    PAAC_REQUIRE(noops >= 0, "paac_eval_step: noops=%d is negative", noops);
    PAAC_REQUIRE(probs && state_in && state_out && stack_in && stack_out && actions_out && score && length && done && alive,
                 "paac_eval_step: bad arguments");
    PAAC_REQUIRE(state_in != state_out && stack_in != stack_out,
                 "paac_eval_step: the step cannot run in place (every band workgroup of an environment reads state_in)");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
    launch_k(eval_step_kernel<decltype(g)>, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, probs, A, greedy, eval_seed, noops,
             step_base_dev, step_offset, env_seed, env_offset, N, state_in, state_out, (const uint32_t*)stack_in,
             (uint32_t*)stack_out, actions_out, score, length, done, alive);
    PAAC_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

// One step of a head-to-head match on N / 2 duel boards (spec: paac_amd/match.py).  An entry of its own: the paired game has
// no PAAC_EVAL_* id.
int paac_match_step(const float* probs, int N, int A, int greedy, uint64_t eval_seed, int noops, const uint64_t* step_base_dev,
                    uint64_t step_offset, uint64_t env_seed, uint32_t env_offset, const int32_t* state_in, int32_t* state_out,
                    const uint8_t* stack_in, uint8_t* stack_out, int32_t* actions_out, float* score, int32_t* length,
                    int32_t* done, int32_t* alive, paac_stream_t stream) {
  PAAC_REQUIRE(N >= 2 && N % 2 == 0, "paac_match_step: N=%d is not an even number of rows >= 2 (two rows per board)", N);
  PAAC_REQUIRE(A == kMatchActions, "paac_match_step: A=%d is not the 6 actions of the duel board", A);
  PAAC_REQUIRE(noops >= 0, "paac_match_step: noops=%d is negative", noops);
  PAAC_REQUIRE(probs, "paac_match_step: null probs");
  PAAC_REQUIRE(state_in && state_out, "paac_match_step: null state_in / state_out");
  PAAC_REQUIRE(stack_in && stack_out, "paac_match_step: null stack_in / stack_out");
  PAAC_REQUIRE(actions_out, "paac_match_step: null actions_out");
  PAAC_REQUIRE(score && length && done && alive, "paac_match_step: null score / length / done / alive");
  PAAC_REQUIRE(state_in != state_out && stack_in != stack_out,
               "paac_match_step: the step cannot run in place (every band workgroup of a row reads state_in)");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(g_prof_ctx, F_ENV_STEP, N, s);
  launch_k(match_step_kernel, dim3(N, PRE_BANDS), dim3(256), s, PROF_WHOLE, probs, greedy, eval_seed, noops, step_base_dev,
           step_offset, env_seed, env_offset, N, state_in, state_out, (const uint32_t*)stack_in, (uint32_t*)stack_out,
           actions_out, score, length, done, alive);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

// Duel against a pool of past selves (spec: paac_amd/duel_pool.py): N boards, the learner at the bottom of each, a ghost row
// of a frozen policy at the top.  Reset and step are ghost_step_kernel, as the games' are game_step_kernel.
int paac_duel_ghost_reset(uint64_t seed, uint32_t env_offset, int N, int32_t* state_out, uint8_t* stack_out,
                          uint8_t* ghost_stack_out, paac_stream_t stream) {
  PAAC_REQUIRE(N >= 1, "paac_duel_ghost_reset: N=%d boards: expected at least 1", N);
  PAAC_REQUIRE(state_out, "paac_duel_ghost_reset: null state_out");
  PAAC_REQUIRE(stack_out, "paac_duel_ghost_reset: null stack_out");
  PAAC_REQUIRE(ghost_stack_out, "paac_duel_ghost_reset: null ghost_stack_out");
  PAAC_REQUIRE(stack_out != ghost_stack_out, "paac_duel_ghost_reset: stack_out and ghost_stack_out are the same buffer");
  hipLaunchKernelGGL(ghost_step_kernel, dim3(2 * N, PRE_BANDS), dim3(256), 0, (hipStream_t)stream, seed, env_offset, N,
                     (const int32_t*)nullptr, (const float*)nullptr, (uint64_t)0, (const uint64_t*)nullptr, (uint64_t)0,
                     (const int32_t*)nullptr, state_out, (int32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)stack_out,
                     (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)ghost_stack_out, (uint32_t*)nullptr, EnvRecords{},
                     (int32_t*)nullptr);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

int paac_duel_ghost_step(uint64_t seed, uint32_t env_offset, int N, const int32_t* actions, const float* ghost_probs, int A,
                         uint64_t sampler_seed, const uint64_t* step_base_dev, uint64_t step_offset, const int32_t* state_in,
                         int32_t* state_out, int32_t* state_out2, const uint8_t* stack_in, uint8_t* stack_out,
                         uint8_t* stack_out2, const uint8_t* ghost_stack_in, uint8_t* ghost_stack_out,
                         uint8_t* ghost_stack_out2, const paac_env_records* rec, int32_t* ghost_actions_out,
                         paac_stream_t stream) {
  PAAC_REQUIRE(N >= 1, "paac_duel_ghost_step: N=%d boards: expected at least 1", N);
  PAAC_REQUIRE(A == kMatchActions, "paac_duel_ghost_step: A=%d is not the 6 actions of the duel board", A);
  PAAC_REQUIRE(actions, "paac_duel_ghost_step: null actions");
  PAAC_REQUIRE(ghost_probs, "paac_duel_ghost_step: null ghost_probs");
  PAAC_REQUIRE(state_in && state_out, "paac_duel_ghost_step: null state_in / state_out");
  PAAC_REQUIRE(stack_in && stack_out, "paac_duel_ghost_step: null stack_in / stack_out");
  PAAC_REQUIRE(ghost_stack_in && ghost_stack_out, "paac_duel_ghost_step: null ghost_stack_in / ghost_stack_out");
  PAAC_REQUIRE(rec, "paac_duel_ghost_step: null records");
  PAAC_REQUIRE(rec->rewards && rec->masks && rec->ep_reward && rec->ep_len,
               "paac_duel_ghost_step: null records rewards / masks / ep_reward / ep_len");
  PAAC_REQUIRE(ghost_actions_out, "paac_duel_ghost_step: null ghost_actions_out");
  PAAC_REQUIRE(state_in != state_out && state_in != state_out2,
               "paac_duel_ghost_step: state_in is state_out or state_out2: the step cannot run in place (every band workgroup "
               "of a board reads state_in)");
  PAAC_REQUIRE(stack_in != stack_out && stack_in != stack_out2,
               "paac_duel_ghost_step: stack_in is stack_out or stack_out2: the step cannot run in place");
  PAAC_REQUIRE(ghost_stack_in != ghost_stack_out && ghost_stack_in != ghost_stack_out2,
               "paac_duel_ghost_step: ghost_stack_in is ghost_stack_out or ghost_stack_out2: the step cannot run in place");
  PAAC_REQUIRE(stack_in != ghost_stack_out && stack_in != ghost_stack_out2 && ghost_stack_in != stack_out &&
               ghost_stack_in != stack_out2 && stack_out != ghost_stack_out,
               "paac_duel_ghost_step: the learner's and the ghost's stack buffers overlap");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(g_prof_ctx, F_ENV_STEP, 2 * N, s);
  launch_k(ghost_step_kernel, dim3(2 * N, PRE_BANDS), dim3(256), s, PROF_WHOLE, seed, env_offset, N, actions, ghost_probs,
           sampler_seed, step_base_dev, step_offset, state_in, state_out, state_out2, (const uint32_t*)stack_in,
           (uint32_t*)stack_out, (uint32_t*)stack_out2, (const uint32_t*)ghost_stack_in, (uint32_t*)ghost_stack_out,
           (uint32_t*)ghost_stack_out2, env_records_of(rec), ghost_actions_out);
  PAAC_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
