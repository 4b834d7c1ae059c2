"""Patrol: an 18-action game written OUTSIDE the package, compiled into the device loop by --emulator user --device_game.
A craft flies over a 14 x 14 board; four drones cross it in four lanes; the craft has one shot at a time, which flies sideways
in the direction the craft last moved in.  A drone shot is +1, a drone touched costs a life and -1.

This is the SPEC of the patrol environment and the specification module --device_game takes (paac_amd/user_game.py: the
attributes at the end of the constants below); the same numbers are produced
  * on the host by `PatrolEnvironment` (a BaseEnvironment plugin, numpy and pure Python; bound to the name `Environment`), and
  * on the device by paac_user_game_reset / paac_user_game_step of the library built from patrol_dev.h (trait PatrolGame).
Rally drives the 6-action paths; this game drives the 18-action ones -- the heads, both samplers and the evaluation's walk over
18 probabilities -- with ALE's full action set, every action of which differs in effect.

Spec (all hashing reuses lowbias32 and h = synth_key(seed, g, k) of paac_amd/synthetic.py unchanged; g = the global environment
env_offset + e, k = the episode index):
  board          14 x 14 cells of 6 x 6 pixels = 84 x 84; columns and rows 0..13, row 0 at the top
  actions        ALE's full set in ALE's order: 0 NOOP, 1 FIRE, 2 UP, 3 RIGHT, 4 LEFT, 5 DOWN, 6 UPRIGHT, 7 UPLEFT, 8 DOWNRIGHT,
                 9 DOWNLEFT, 10 UPFIRE, 11 RIGHTFIRE, 12 LEFTFIRE, 13 DOWNFIRE, 14 UPRIGHTFIRE, 15 UPLEFTFIRE, 16 DOWNRIGHTFIRE,
                 17 DOWNLEFTFIRE; each is (mx, my, fire) with mx, my in {-1, 0, +1}, UP is my = -1 (any other number: NOOP)
  constants      LANES = (2, 5, 8, 11), LIVES = 3, MAX_STEPS = 1000, SHOT_SPEED = 2, WAIT = 32
  state          per environment, int32: (px, py, face, lives, sx, sy, sd, steps, x0..x3, d0..d3, k).  The craft is at cell
                 (px, py); face in {-1, +1} is the sideways direction it last moved in.  One shot: sd = 0 means none (sx, sy then
                 mean nothing and stay what they were), otherwise it is at (sx, sy) flying in direction sd.  Drone i lives in row
                 LANES[i]: on the board at column x_i >= 0 flying in direction d_i, or waiting (x_i < 0): -x_i steps remain and
                 it will enter flying d_i.  k = the number of episodes this environment has started before the current one.
                 The device record is STATE_WORDS = 20: five 16-byte parts in that order, k followed by three zeros
  park(h, salt)  w = lowbias32(h ^ salt): x = -(1 + (w >> 1) % WAIT), d = +1 if w & 1 else -1
  episode start  px = lowbias32(h ^ 0x9A7E0001) % 14, py = lowbias32(h ^ 0x9A7E0002) % 14, face = +1, lives = 3, no shot
                 (sx = sy = sd = 0), steps = 0, drone i = park(h, 0x9A7E0010 + i)
  step(a)        in this order (h of the current episode, steps before its increment; every parking of drone i in the step
                 uses the salt 0x9A7E1000 + 16 * steps + i):
                   1. if mx != 0: face = mx.  px = clamp(px + mx, 0, 13), py = clamp(py + my, 0, 13)
                   2. fire and sd == 0: the shot appears at (px, py) with sd = face (it flies in 4. of this same step)
                   3. every drone on the board in the craft's cell is a hit and is parked
                   4. if sd != 0, up to SHOT_SPEED times: sx += sd; off the board: sd = 0, stop; a drone on the board at
                      (sx, sy): reward += 1, the drone is parked, sd = 0, stop
                   5. drones 0..3 in order.  Waiting: x_i += 1; still negative: done; else it enters at column 0 if d_i > 0, at
                      column 13 otherwise.  On the board: x_i += d_i; off the board: parked (escaped), done.  Then, entered or
                      moved: the shot live and in its cell: reward += 1, sd = 0, parked; else the craft in its cell: a hit,
                      parked.  (Kept on purpose: a drone parked with a wait of 1 in 3. or 4. enters again in this same step.)
                   6. any hit: lives -= 1 and reward -= 1, once per step: the reward is in {-1, 0, +1}
                   7. steps += 1; dead = lives == 0 or (single_life and hit); terminal if dead or steps == MAX_STEPS; truncated
                      if terminal and not dead; a terminal step starts episode k + 1 at once
  plane(state)   a pixel in cell (cy, cx) = 255 if the shot is live there; else the craft's cell is 128 with its two pixel
                 columns on the `face` side at 224 (one plane shows the facing); else 64 for a drone on the board; else 0
  observation    rally's rule: the previous stack shifted by one channel with the new plane as channel 3; at construction and
                 after a terminal step it is [0, 0, 0, plane of the new start state] -- the terminal position is never shown
  bookkeeping    as rally's: reward clipped to [-1, 1] (a no-op here), mask = 0 on terminal, ep_reward / ep_len totals, the
                 finished-episode ring
--single_life_episodes makes every hit end the episode; -g, --synthetic_terminal_p and --random_start do not apply.

Anchors, seed 3, (g, k) -> (px, py, x0..x3, d0..d3): (0, 0) -> (0, 11, -5, -30, -1, -27, -1, 1, -1, 1);
(1, 0) -> (13, 10, -7, -14, -5, -12, 1, 1, -1, -1); (2, 0) -> (9, 0, -11, -7, -12, -12, -1, -1, 1, 1);
(0, 1) -> (4, 4, -1, -31, -15, -1, 1, -1, -1, -1).
Scores, seed 3, environments 0..63 (rally.py's protocol).  The policies without skill over the first 16 episodes of each
environment (1024 episodes; uniform random drawn with random.Random(0).randrange(18), environment after environment), the two
reference policies over the first 4 episodes of each (256 episodes):
  uniform random   mean return -0.4717 (sum -483), std 2.160, lengths 31 to 779, mean 235.5, none at the step cap
  always NOOP      mean return -0.8438 (sum -864), std 1.349, mean length 738.2, 736 at the step cap (the starts in a safe row)
  always FIRE      mean return -0.0713 (sum -73), std 1.381, mean length 751.3, 736 at the step cap
  camper_action    mean return +54.9102 (sum +14057), std 3.835, every episode at the step cap
  hunter_action    mean return +109.9258 (sum +28141), std 7.379, every episode at the step cap
Chance, then "shoot what comes" (camper_action: one lane, turning and firing, a step aside when a drone comes too close), then
"go where the targets are" (hunter_action: the step that needs the vertical and diagonal actions).
"""
import numpy as np

from paac_amd.environment import BaseEnvironment
from paac_amd.synthetic import lowbias32_int, synth_key

CELLS = 14                 # board cells per side
CELL = 6                   # pixels per cell side
LANES = (2, 5, 8, 11)      # the drones' rows
LIVES = 3
MAX_STEPS = 1000
SHOT_SPEED = 2
WAIT = 32
SHOT, CRAFT, NOSE, DRONE = 255, 128, 224, 64   # pixel values
# (mx, my, fire) of ALE's 18 actions, in ALE's order
ACTIONS = ((0, 0, 0), (0, 0, 1), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, -1, 0), (-1, -1, 0), (1, 1, 0), (-1, 1, 0),
           (0, -1, 1), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (1, -1, 1), (-1, -1, 1), (1, 1, 1), (-1, 1, 1))
ACTION_OF = {m: a for a, m in enumerate(ACTIONS)}
NOOP, FIRE = 0, 1

# what --device_game reads (paac_amd/user_game.py)
NUM_ACTIONS = 18
STATE_WORDS = 20           # int32 words of a device state record: the 17 state words, then three zeros
MAX_EPISODE_STEPS = MAX_STEPS
TRUNCATES = True           # MAX_STEPS is a step cap: --bootstrap_truncated may bootstrap there
STEP_OPTION = "single_life"
DEVICE_HEADER = "patrol_dev.h"
DEVICE_TRAIT = "PatrolGame"


def park(h, salt):
    """-> (x, d) of a drone sent to wait: -x steps remain, it will enter flying d."""
    w = lowbias32_int(h ^ salt)
    return -(1 + (w >> 1) % WAIT), (1 if w & 1 else -1)


def start_state(seed, env, k):
    """-> the state episode k of global environment env starts from."""
    h = synth_key(seed, env, k)
    px = lowbias32_int(h ^ 0x9A7E0001) % CELLS
    py = lowbias32_int(h ^ 0x9A7E0002) % CELLS
    drones = [park(h, 0x9A7E0010 + i) for i in range(4)]
    return (px, py, 1, LIVES, 0, 0, 0, 0) + tuple(x for x, _ in drones) + tuple(d for _, d in drones) + (k,)


def step_state(seed, env, state, a, single_life=False):
    """One step of `state` under action a -> (state, reward, terminal).  The state returned is the one the next step starts
    from: after a terminal step that is the start state of episode k + 1 (the device record's rule)."""
    return step_state_truncated(seed, env, state, a, single_life)[:3]


def step_events(seed, env, state, a, single_life=False):
    """step_state_truncated with what happened on the step -> (state, reward, terminal, truncated, events): events is the set
    of the names "kill_flight", "kill_move", "hit_walk", "hit_move", "escape", "entry", "shot_off" (the tests' trace)."""
    px, py, face, lives, sx, sy, sd, steps = state[:8]
    x, d, k = list(state[8:12]), list(state[12:16]), state[16]
    h = synth_key(seed, env, k)
    mx, my, fire = ACTIONS[a] if 0 <= a < NUM_ACTIONS else ACTIONS[NOOP]
    events = set()
    reward, hit = 0.0, False

    def send(i):
        x[i], d[i] = park(h, 0x9A7E1000 + 16 * steps + i)

    if mx != 0:
        face = mx
    px = min(max(px + mx, 0), CELLS - 1)
    py = min(max(py + my, 0), CELLS - 1)
    if fire and sd == 0:
        sx, sy, sd = px, py, face
    for i in range(4):
        if x[i] >= 0 and x[i] == px and LANES[i] == py:
            hit = True
            events.add("hit_walk")
            send(i)
    if sd != 0:
        for _ in range(SHOT_SPEED):
            sx += sd
            if sx < 0 or sx > CELLS - 1:
                sd = 0
                events.add("shot_off")
                break
            struck = [i for i in range(4) if x[i] >= 0 and x[i] == sx and LANES[i] == sy]
            if struck:
                reward += 1.0
                events.add("kill_flight")
                send(struck[0])
                sd = 0
                break
    for i in range(4):
        if x[i] < 0:
            x[i] += 1
            if x[i] < 0:
                continue
            x[i] = 0 if d[i] > 0 else CELLS - 1
            events.add("entry")
        else:
            x[i] += d[i]
            if x[i] < 0 or x[i] > CELLS - 1:
                events.add("escape")
                send(i)
                continue
        if sd != 0 and x[i] == sx and LANES[i] == sy:
            reward += 1.0
            events.add("kill_move")
            sd = 0
            send(i)
        elif x[i] == px and LANES[i] == py:
            hit = True
            events.add("hit_move")
            send(i)
    if hit:
        lives -= 1
        reward -= 1.0
    steps += 1
    dead = lives == 0 or (bool(single_life) and hit)
    if dead or steps == MAX_STEPS:
        return start_state(seed, env, k + 1), reward, True, not dead, events
    return (px, py, face, lives, sx, sy, sd, steps) + tuple(x) + tuple(d) + (k,), reward, False, False, events


def step_state_truncated(seed, env, state, a, single_life=False):
    """step_state with the reason of a terminal step -> (state, reward, terminal, truncated): truncated = the step is terminal
    only because steps reached MAX_STEPS (no life was lost that ends the episode on it).  The cap is a time limit, not a
    property of the state: --bootstrap_truncated bootstraps the return there."""
    return step_events(seed, env, state, a, single_life)[:4]


def plane(state):
    px, py, face, _, sx, sy, sd = state[:7]
    out = np.zeros((84, 84), dtype=np.uint8)
    for i in range(4):
        if state[8 + i] >= 0:
            out[LANES[i] * CELL:(LANES[i] + 1) * CELL, state[8 + i] * CELL:(state[8 + i] + 1) * CELL] = DRONE
    out[py * CELL:(py + 1) * CELL, px * CELL:(px + 1) * CELL] = CRAFT
    nose = px * CELL + (CELL - 2 if face > 0 else 0)
    out[py * CELL:(py + 1) * CELL, nose:nose + 2] = NOSE
    if sd != 0:
        out[sy * CELL:(sy + 1) * CELL, sx * CELL:(sx + 1) * CELL] = SHOT
    return out


def state_words(state):
    """The device record of `state` (int32 [STATE_WORDS])."""
    return np.array(list(state) + [0] * (STATE_WORDS - len(state)), dtype=np.int32)


def _lane_action(state, i):
    """What both reference policies do about lane i: go to its row (never into a lane row whose drone is within 2 columns),
    keep off the edge columns, face the side the drone comes from, fire at it, and step out of the row when it comes too close
    from behind or while the shot is away."""
    px, py, face, _, sx, sy, sd = state[:7]
    x, d, row = state[8 + i], state[12 + i], LANES[i]
    centre = 1 if px < 3 else (-1 if px > 10 else 0)
    if py != row:
        my = 1 if row > py else -1
        if py + my in LANES:
            xj = state[8 + LANES.index(py + my)]
            if xj >= 0 and abs(xj - (px + centre)) <= 2:
                return ACTION_OF[(centre, 0, 0)]
        return ACTION_OF[(centre, my, 0)]
    out = ACTION_OF[(0, -1, 0)]
    if x < 0:
        want = -d                                          # it enters at column 0 flying right, or at 13 flying left
        if -x > 4 and centre:
            return ACTION_OF[(centre, 0, 0)]
        if face != want:
            return ACTION_OF[(want if 1 <= px + want <= CELLS - 2 else -want, 0, 0)]
        return NOOP
    dist = x - px
    side = 1 if dist > 0 else -1
    approaching = d == -side
    if face == side:
        if sd == 0:
            return FIRE
        if sy == py and sd == side and (x - sx) * side > 0:
            return NOOP                                    # the shot is between the two and cannot pass the drone
        return out if approaching and abs(dist) <= 3 else NOOP
    if not approaching:
        return ACTION_OF[(side, 0, 1)] if abs(dist) >= 2 else NOOP
    if abs(dist) >= 3 and sd == 0:
        return ACTION_OF[(side, 0, 1)]
    if abs(dist) >= 5:
        return ACTION_OF[(side, 0, 0)]
    return out


def camper_action(state):
    """Reference policy: go to row 5 and stay there, off the edge columns; turn with RIGHTFIRE / LEFTFIRE and fire at what
    enters; step out of the row when an approaching drone is within 2 cells."""
    return _lane_action(state, 1)


def hunter_action(state):
    """Reference policy: the camper's play in whichever lane has a reachable drone -- one on the board that will still be
    there when the craft arrives, else the one that enters soonest."""
    py = state[1]
    best, best_key = 0, None
    for i in range(4):
        x, d, rows = state[8 + i], state[12 + i], abs(LANES[i] - py)
        if x >= 0:
            left = (CELLS - 1 - x) if d > 0 else x
            key = (0, rows) if left >= rows + 2 else (2, rows)
        else:
            key = (1, max(-x, rows) + rows)
        if best_key is None or key < best_key:
            best, best_key = i, key
    return _lane_action(state, best)


class PatrolEnvironment(BaseEnvironment):
    def __init__(self, actor_id, seed=0, single_life=False):
        self.actor_id = int(actor_id)
        self.num_actions = NUM_ACTIONS
        self.seed = int(seed)
        self.single_life = bool(single_life)
        self.state = start_state(self.seed, self.actor_id, 0)
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.last_step_truncated = False       # the last next() ended its episode at the step cap alone (runners.py reads it)

    @property
    def k(self):
        return self.state[16]

    def state_words(self):
        """The device twin's state record of this environment (int32 [STATE_WORDS])."""
        return state_words(self.state)

    def get_initial_state(self):
        self.stack = np.zeros((84, 84, 4), dtype=np.uint8)
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack)

    def next(self, action):
        a = int(np.argmax(action))
        self.state, reward, terminal, self.last_step_truncated = step_state_truncated(self.seed, self.actor_id, self.state, a,
                                                                                       self.single_life)
        self.stack[..., :3] = self.stack[..., 1:]
        self.stack[..., 3] = plane(self.state)
        return np.copy(self.stack), reward, terminal

    def get_legal_actions(self):
        return np.arange(self.num_actions)

    def get_noop(self):
        return [1.0] + [0.0] * (NUM_ACTIONS - 1)


Environment = PatrolEnvironment
