"""What the learner's four bookkeeping kernels must compute, stated ONCE as a host model with a case table: azul_discounted_returns,
azul_discounted_returns_ring, azul_select_complete_samples and azul_select_episode_samples (include/azul_hip.h; the reference's loop is
nn_runner.py:59-76: whole episodes, q = reward + gamma * q backwards inside an episode).  The GPU test
(tests/test_gpu_training_ring.py) and the lockstep CPU emulation (tests/test_hostcheck_learner.py) build their inputs here and compare
through the compare_* functions below, so both ask the same; tests/test_training_ring_cases.py checks the model itself.

numpy only: no torch, no GPU, no ctypes.  The model is written from the header's contract, not from the kernels: per-game loops over
steps, no ballots, no chunks.  (The returns scans loop over time in Python and apply each float32 operation to all games at once -- an
elementwise numpy operation on float32 arrays rounds every element once, so each column is exactly the per-game loop
returns_column() spells out; the model test compares the two.)

The device library is compiled without contraction and without fast-math, so the float32 recurrence has ONE result and the model
demands the same bits.  returns_window_f64 (the fp64 twin and its running bound) is the plain high-precision statement of the same scan."""
import numpy as np

U23 = 2.0 ** -23                 # one rounding of the product + one of the sum (+ the reward's int -> float): 2 * 2^-24 per term
STEP_LIMIT = 0x7fff0000          # azul_select_episode_samples: largest steps_played
SENTINEL = -0x5A5A5A5B           # guard words behind index / scratch
NAN_BITS = 0x7fc00000            # quiet NaN; the low 16 bits carry a position pattern


# ---------------------------------------------------------------------------------------------------------------- the model
def returns_window(reward, done, gamma, carry):
    """azul_discounted_returns: float32, statement for statement.  reward int32 [T][N], done uint8 [T][N], carry float32 [N] or None
    (the return flowing in from the NEXT window; None = 0).  Returns (returns float32 [T][N], carry_out float32 [N])."""
    T, N = reward.shape
    g32 = np.float32(gamma)
    q = np.zeros(N, np.float32) if carry is None else np.array(carry, np.float32)
    out = np.zeros((T, N), np.float32)
    zero = np.float32(0)
    for t in range(T - 1, -1, -1):
        q = np.where(done[t] != 0, zero, q)                          # an episode end: nothing flows in from later steps
        prod = np.multiply(g32, q, dtype=np.float32)                 # one rounding
        q = np.add(reward[t].astype(np.float32), prod, dtype=np.float32)      # int -> float rounds, the sum rounds
        out[t] = q
    return out, q


def returns_column(reward, done, gamma, carry):
    """The same for ONE game with numpy float32 scalars: the literal per-game loop."""
    g32, q = np.float32(gamma), np.float32(0 if carry is None else carry)
    out = np.zeros(len(reward), np.float32)
    for t in range(len(reward) - 1, -1, -1):
        if done[t] != 0:
            q = np.float32(0)
        q = np.float32(np.float32(reward[t]) + np.float32(g32 * q))
        out[t] = q
    return out, q


def returns_window_f64(reward, done, gamma, carry):
    """The fp64 twin (gamma is the float32 the kernel gets) and the running bound of float32's distance from it:
    bound[t] = g * bound[t+1] + 2^-23 * (|r[t]| + g * |q64[t+1]|), nothing flowing in at an episode end (a carry is taken as exact)."""
    T, N = reward.shape
    g = float(np.float32(gamma))
    q = np.zeros(N, np.float64) if carry is None else np.array(carry, np.float64)
    b = np.zeros(N, np.float64)
    out, bound = np.zeros((T, N), np.float64), np.zeros((T, N), np.float64)
    for t in range(T - 1, -1, -1):
        end = done[t] != 0
        q, b = np.where(end, 0.0, q), np.where(end, 0.0, b)
        r = reward[t].astype(np.float64)
        b = g * b + U23 * (np.abs(r) + g * np.abs(q))
        q = r + g * q
        out[t], bound[t] = q, b
    return out, bound


def returns_ring(reward_ring, done_ring, returns_ring_in, gamma, ring_steps, steps_played, span):
    """azul_discounted_returns_ring: absolute step s lives in slot s % ring_steps; from the newest step steps_played - 1 back over `span`
    steps, nothing flowing into the newest step.  Returns the ring after the call: slots outside the span keep their bits."""
    out = np.array(returns_ring_in, np.float32, copy=True)
    g32, zero = np.float32(gamma), np.float32(0)
    q = np.zeros(reward_ring.shape[1], np.float32)
    for s in range(steps_played - 1, steps_played - 1 - span, -1):
        slot = s % ring_steps
        q = np.where(done_ring[slot] != 0, zero, q)
        q = np.add(reward_ring[slot].astype(np.float32), np.multiply(g32, q, dtype=np.float32), dtype=np.float32)
        out[slot] = q
    return out


def select_complete(done, action):
    """azul_select_complete_samples: per game the steps up to its last episode end that carry an action, as t * N + g, game by game."""
    T, N = done.shape
    index = []
    for g in range(N):
        d, a = done[:, g].tolist(), action[:, g].tolist()             # this game's column
        last = -1
        for t in range(T):
            if d[t] != 0:
                last = t
        for t in range(last + 1):
            if a[t] >= 0:
                index.append(t * N + g)
    return index, len(index)


def select_ring(done_ring, action_ring, T, D, steps_played, pending):
    """azul_select_episode_samples: the newest window is steps_played - T .. steps_played - 1; a game with an episode end in it hands out
    its steps from pending[g] up to the LAST such end, those still intact in the ring and carrying an action, as slot * N + g.  The
    oldest intact step: lo = steps_played - R + (1 if steps_played % R else 0), at least 0 (unless the newest window is the ring's last,
    the slot of step steps_played - R already holds the state after the window).  Steps before lo are dropped.
    Returns (index list, new pending [N] int64, dropped)."""
    R, N = T * D, done_ring.shape[1]
    lo = max(0, steps_played - R + (1 if steps_played % R else 0))
    index, dropped, new = [], 0, np.array(pending, np.int64)
    for g in range(N):
        d, a = done_ring[:, g].tolist(), action_ring[:, g].tolist()   # this game's column of the ring
        last = -1
        for s in range(steps_played - T, steps_played):
            if d[s % R] != 0:
                last = s
        if last < 0:
            continue
        start = max(int(pending[g]), lo)
        dropped += start - int(pending[g])
        for s in range(start, last + 1):
            if a[s % R] >= 0:
                index.append((s % R) * N + g)
        new[g] = last + 1
    return index, new, dropped


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def compare_returns(case_id, got, want, what="returns"):
    """Bit equality of two float32 arrays [T][N] or [N] (NaN patterns included); the message names the first cell that differs."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (case_id, what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    if len(bad):
        at = tuple(int(x) for x in bad[0])
        where = "step/slot %d game %d" % at if len(at) == 2 else "game %d" % at
        raise AssertionError("%s: %s differ in %d cells, first at %s: got %r (0x%08x) want %r (0x%08x)" % (
            case_id, what, len(bad), where, float(got[at]), int(_bits(got)[at]) & 0xffffffff, float(want[at]), int(_bits(want)[at]) & 0xffffffff))


def compare_index(case_id, got_index, got_count, want_index, n_games, what="index"):
    """index[:count] equals the model's list; the message names game and step (or ring slot) of the first difference."""
    want = np.asarray(want_index, np.int64)
    assert int(got_count) == len(want), "%s: %s count %d, model %d" % (case_id, what, int(got_count), len(want))
    got = np.asarray(got_index[:len(want)], np.int64)
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %s[%d] is %d (step/slot %d game %d), model %d (step/slot %d game %d); %d entries differ" % (
            case_id, what, i, got[i], got[i] // n_games, got[i] % n_games, want[i], want[i] // n_games, want[i] % n_games, len(bad)))


def compare_pending(case_id, got, want):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    bad = np.flatnonzero(got != want)
    if len(bad):
        g = int(bad[0])
        raise AssertionError("%s: pending of game %d is %d, model %d; %d games differ" % (case_id, g, got[g], want[g], len(bad)))


def compare_countf(case_id, countf, count):
    want = np.array([np.float32(count), np.float32(1.0) / np.float32(max(count, 1))], np.float32)
    assert _bits(countf).tolist() == _bits(want).tolist(), "%s: countf %r, want %r" % (case_id, list(map(float, countf)), want.tolist())


def compare_guard(case_id, tail, what):
    tail = np.asarray(tail)
    bad = np.flatnonzero(tail != SENTINEL)
    assert len(bad) == 0, "%s: %s written at %d words (first at +%d: %d)" % (case_id, what, len(bad), int(bad[0]), int(tail[bad[0]]))


def nan_pattern(shape, salt=0):
    """float32 NaNs whose low bits count the position: a slot that must stay untouched keeps exactly these bits."""
    n = int(np.prod(shape))
    bits = (NAN_BITS | ((np.arange(n, dtype=np.int64) * 7 + salt) & 0xffff)).astype(np.int32)
    return bits.view(np.float32).reshape(shape).copy()


def _done_values(rs, mask):
    """uint8 flags: 0 where mask is False, else 1, 2 or 3 (what the env writes: ended, nobody could move, move limit)."""
    return (mask * rs.randint(1, 4, size=mask.shape)).astype(np.uint8)


def _actions(rs, shape, p_none=0.06):
    return np.where(rs.rand(*shape) < p_none, -1, rs.randint(0, 180, size=shape)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- select_complete
# every N once, every T once, and (2500, 130); plus one lone game with the re-read path (its only column cannot hold every plant)
COMPLETE_SHAPES = [(1, 0), (63, 1), (1024, 64), (1025, 65), (2500, 130), (1, 130)]
# (in planting order: a chunk too small for all of them -- the lone game 1024 of N = 1025 -- gets the first, which carries samples)
COMPLETE_KINDS = ("end_last", "end64", "end63", "done123", "end_first", "all_none", "no_end")


class CompleteCase:
    """One window [T][N] for azul_select_complete_samples.  Planted columns (self.planted: kind -> games), at the first games of every
    chunk of 1024 games in COMPLETE_KINDS' order and mirrored at its last games, so the first and the last game of each chunk are planted:
      no_end     no episode end: contributes nothing
      end_first  the only end at t = 0: one step
      end_last   the only end at t = T - 1: the whole column
      end63      the last end exactly at t = 63: the last step the 64-bit action mask covers (needs T >= 64)
      end64      the last end exactly at t = 64: the first step behind it, the kernel reads the actions again (needs T >= 65)
      all_none   a finished episode whose actions are all -1: an end is found, nothing is kept
      done123    ends flagged 1, 2 and 3: any non-zero flag ends an episode (needs T >= 3)"""

    def __init__(self, N, T):
        self.N, self.T, self.id = N, T, "complete-N%d-T%d" % (N, T)

    def kinds(self):
        T = self.T
        need = {"no_end": 1, "end_first": 1, "end_last": 1, "end63": 64, "end64": 65, "all_none": 1, "done123": 3}
        return [k for k in COMPLETE_KINDS if T >= need[k]]

    def build(self):
        N, T = self.N, self.T
        rs = np.random.RandomState(1000 + 7 * N + T)
        done = _done_values(rs, rs.rand(T, N) < 0.03)
        action = _actions(rs, (T, N))
        kinds, planted = self.kinds(), {}
        if N == 1 and T > 64:
            kinds = ["end64"]
        for c0 in range(0, N, 1024):
            c1 = min(c0 + 1024, N) - 1
            size = c1 - c0 + 1
            spots = []
            for i, k in enumerate(kinds):
                spots.append((c0 + i, k))
                spots.append((c1 - i, k))
            taken = set()
            for g, k in spots:
                if g in taken or not (c0 <= g <= c1) or (len(taken) >= size):
                    continue
                taken.add(g)
                planted.setdefault(k, []).append(g)
                done[:, g] = 0
                if k == "end_first":
                    done[0, g] = 1
                elif k == "end_last":
                    done[T - 1, g] = 1
                elif k == "end63":
                    done[63, g] = 1
                    done[10, g] = 2
                elif k == "end64":
                    done[64, g] = 1
                    done[63, g] = 1
                elif k == "all_none":
                    done[T // 2, g] = 1
                    action[:, g] = -1
                elif k == "done123":
                    done[0, g], done[T // 2, g], done[T - 1, g] = 1, 2, 3
        self.planted = planted
        return done, action


COMPLETE_CASES = [CompleteCase(N, T) for N, T in COMPLETE_SHAPES]


# ---------------------------------------------------------------------------------------------------------------- select_ring
RING_SHAPES = [(1, 1, 1), (3, 8, 2), (5, 64, 2), (1023, 8, 3), (1029, 8, 3), (6, 65, 2), (7, 100, 3)]


class RingCase:
    """A sequence of windows on one ring [R = T * D][N] for azul_select_episode_samples, pending carried from call to call; at least
    3 D + 2 windows: the ring wraps three times and steps_played % R is both zero and not.  self.done / self.action are the ABSOLUTE
    history [windows * T][N]; ring_after(w) is the ring once window w has been played.  About 6 % of the actions are -1.  Planted games
    (self.roles: role -> games):
      edges    an end at the FIRST step of window k when k % 3 == 0, at the LAST step when k % 3 == 1, at both when k % 3 == 2 (the last
               game; for N = 1029 also games 1024 .. 1028: blocks 256 and 257 carry samples, so a block's base sums more than 256 blocks)
      long     (rings of more than 64 slots) episodes of exactly 64, 65, 70 and 100 steps, each alone in its window (filler episodes between
               them): 64 fills one ballot of the per-game step loop, the others need a second one; those of 64 and 65 steps are whole in the ring when they end
      outlive  an end every R + T // 2 + 1 steps: every episode outlives the ring, its oldest steps are dropped and counted
      never    no end at all: never contributes, pending stays
    The other games end a step with probability 0.14, every fifth of them with 0.02 (long random episodes: drops in short rings).
    `shift` > 0: the same sequence with m * R added to steps_played and to the first pending, m such that the LAST call's steps_played is
    the largest multiple of T not above 0x7fff0000 (the window count grows until that is a whole number of rings away): slots, indices,
    counts and drops must not change, pending moves by m * R."""

    def __init__(self, N, T, D, shifted=False, windows=None):
        self.N, self.T, self.D, self.R, self.shifted = N, T, D, T * D, shifted
        self.windows = 3 * D + 2 if windows is None else windows
        self.shift = 0
        if shifted:
            top = STEP_LIMIT // T                          # the last call's steps_played / T
            while (top - self.windows) % D:
                self.windows += 1
            self.shift = (top - self.windows) // D * self.R
        self.id = "ring-N%d-T%d-D%d%s" % (N, T, D, "-shifted" if shifted else "") + ("-w%d" % windows if windows else "")

    def build(self):
        N, T, D, R, W = self.N, self.T, self.D, self.R, self.windows
        rs = np.random.RandomState(2000 + N + 13 * T + 101 * D)
        S = W * T
        p_end = np.where(np.arange(N) % 5 == 0, 0.02, 0.14)
        done = _done_values(rs, rs.rand(S, N) < p_end)
        action = _actions(rs, (S, N))
        games = []
        for g in [N - 1, 0, 1, 2]:
            if 0 <= g < N and g not in games:
                games.append(g)
        names = ["edges"] + (["long"] if R > 64 else []) + ["outlive", "never"]
        roles = {k: [g] for k, g in zip(names, games)}
        if N == 1029:
            roles["edges"] += list(range(1024, 1028))
        for g in roles.get("edges", []):
            done[:, g] = 0
            for k in range(W):
                if T == 1:
                    done[k, g] = 0 if k % 3 == 1 else 1    # windows of one step: an episode of two steps now and then
                    continue
                if k % 3 in (0, 2):
                    done[k * T, g] = 1
                if k % 3 in (1, 2):
                    done[k * T + T - 1, g] = 2
        for g in roles.get("long", []):
            done[:, g] = 0
            s, i = -1, 0
            while s + (64, 65, 70, 100)[i % 4] < S:
                s += (64, 65, 70, 100)[i % 4]              # the episode of the wanted length ...
                i += 1
                done[s, g] = 1
                s = (s // T + 2) * T - 1                   # ... then a filler up to the last step of the NEXT window, so that no window
                if s < S:                                  # holds two ends (a game hands out up to its last end: the spans would merge)
                    done[s, g] = 1
        for g in roles.get("outlive", []):
            done[:, g] = 0
            done[R + T // 2::R + T // 2 + 1, g] = 3
        for g in roles.get("never", []):
            done[:, g] = 0
        self.roles, self.done, self.action = roles, done, action
        return self

    def steps_played(self, w):
        return (w + 1) * self.T + self.shift

    def first_pending(self):
        return np.full(self.N, self.shift, np.int64)

    def ring_after(self, w):
        """(done_ring, action_ring) [R][N] after windows 0 .. w: absolute step s in slot s % R (the shift is whole rings: the same slots)."""
        R, N = self.R, self.N
        dr, ar = np.zeros((R, N), np.uint8), np.zeros((R, N), np.int32)
        for s in range(max(0, (w + 1) * self.T - R), (w + 1) * self.T):
            dr[s % R], ar[s % R] = self.done[s], self.action[s]
        return dr, ar

    def expected(self):
        """The model over the whole sequence: per window (index list, pending after, dropped so far)."""
        out, pend, dropped = [], self.first_pending(), 0
        for w in range(self.windows):
            dr, ar = self.ring_after(w)
            index, pend, d = select_ring(dr, ar, self.T, self.D, self.steps_played(w), pend)
            dropped += d
            out.append((index, pend.copy(), dropped))
        return out


RING_CASES = [RingCase(*s) for s in RING_SHAPES]
SHIFT_CASES = [RingCase(1029, 8, 3, shifted=True), RingCase(6, 65, 2, shifted=True)]


# ---------------------------------------------------------------------------------------------------------------- returns_window
# (N, T, gamma, carry present): every N, every T, every gamma, both carries
WINDOW_SHAPES = [(1, 1, 0.99, False), (1, 200, 0.99, True), (255, 2, 0.0, True), (255, 33, 1.0, False), (256, 33, 0.99, True), (256, 2, 0.99, False),
                 (257, 200, 1.0, False), (257, 1, 1.0, True), (257, 33, 0.0, False), (1000, 33, 0.99, False), (1000, 200, 0.99, True)]
WINDOW_KINDS = ("end_last", "end_first", "no_end", "big", "pm200")


class WindowCase:
    """One window [T][N] for azul_discounted_returns.  Rewards are -9 .. 9, an end with probability 0.08.  Planted columns (self.planted:
    kind -> games; at games 0 .. 4 and mirrored at the last five; a lone game holds end_last when a carry flows in, else no_end):
      end_last   an end at t = T - 1: the carry flowing in (planted as 1e6) must not leak into the window
      end_first  the only end at t = 0: the carry flows through steps 1 .. T - 1 and stops there
      no_end     no end at all: the carry flows through the whole column into carry_out
      big        |reward| above 2^24, odd: the int -> float conversion rounds
      pm200      rewards of +-200"""

    def __init__(self, N, T, gamma, carry):
        self.N, self.T, self.gamma, self.has_carry = N, T, gamma, carry
        self.id = "window-N%d-T%d-g%s-%s" % (N, T, ("%g" % gamma).replace(".", "p"), "carry" if carry else "nocarry")

    def build(self):
        N, T = self.N, self.T
        rs = np.random.RandomState(3000 + N + 17 * T + (5 if self.has_carry else 0))
        reward = rs.randint(-9, 10, size=(T, N)).astype(np.int32)
        done = _done_values(rs, rs.rand(T, N) < 0.08)
        carry = (rs.randn(N) * 3).astype(np.float32) if self.has_carry else None
        planted = {}
        if N == 1:
            spots = [(0, "end_last" if self.has_carry else "no_end")]
        else:
            spots = [(i, k) for i, k in enumerate(WINDOW_KINDS)] + [(N - 1 - i, k) for i, k in enumerate(WINDOW_KINDS)]
        for g, k in spots:
            planted.setdefault(k, []).append(g)
            if k == "end_last":
                done[:, g] = 0
                done[T - 1, g] = 1
                if carry is not None:
                    carry[g] = np.float32(1e6)
            elif k == "end_first":
                done[:, g] = 0
                done[0, g] = 2
            elif k == "no_end":
                done[:, g] = 0
            elif k == "big":
                reward[:, g] = (rs.choice([-1, 1], T) * ((1 << 24) + 1 + 2 * rs.randint(0, 1 << 22, T))).astype(np.int32)
            elif k == "pm200":
                reward[:, g] = rs.choice([-200, 200], T)
        self.planted = planted
        return reward, done, carry


WINDOW_CASES = [WindowCase(*s) for s in WINDOW_SHAPES]


# ---------------------------------------------------------------------------------------------------------------- returns_ring
# (ring_steps, span, steps_played, N, gamma, window): the newest step steps_played - 1 sits in slot 0 ("first"), ring_steps - 1 ("last")
# or between ("middle"); window = T when the ring is whole windows of T steps and the span is the ring (the chained-windows comparison)
RETRING_SHAPES = [
    (1, 1, 7, 1, 0.99, None),                  # a ring of one slot
    (5, 1, 11, 63, 0.99, None),                # span 1, newest in slot 0
    (5, 5, 10, 64, 1.0, None),                 # span = ring, newest in the last slot
    (16, 15, 33, 65, 0.99, None),              # one short group of reads, newest in slot 0: the walk wraps at once
    (16, 16, 24, 64, 0.99, 8),                 # exactly one group, newest in the middle; two windows of 8
    (17, 17, 43, 63, 0.99, None),              # one group and one step, newest in the middle
    (17, 16, 35, 65, 0.0, None),               # one group, newest in slot 0
    (48, 17, 96, 1000, 0.99, None),            # newest in the last slot
    (48, 16, 49, 65, 0.99, None),              # newest in slot 0
    (48, 15, 68, 1, 0.99, None),               # newest in the middle
    (48, 48, 80, 1000, 0.99, 16),              # the whole ring, three windows of 16, newest window in the middle
    (48, 48, 2 ** 33 + 5, 1000, 0.99, None),   # a step clock beyond int32 (the entry reduces it on the host): newest in slot 36
]


class RetRingCase:
    """A ring [ring_steps][N] for azul_discounted_returns_ring.  The returns ring starts as a NaN pattern: slots outside the span keep it
    bit for bit.  Game 0 (N > 1: also the last game) has |reward| above 2^24; ends with probability 0.1, flags 1 .. 3."""

    def __init__(self, ring, span, played, N, gamma, window):
        self.ring, self.span, self.played, self.N, self.gamma, self.window = ring, span, played, N, gamma, window
        self.newest = (played - 1) % ring
        self.where = "first" if self.newest == 0 else ("last" if self.newest == ring - 1 else "middle")
        self.id = "retring-R%d-span%d-N%d-%s%s" % (ring, span, N, self.where if ring > 1 else "one", "-2p33" if played > 2 ** 31 else "")

    def build(self):
        R, N = self.ring, self.N
        rs = np.random.RandomState(4000 + 3 * R + 29 * self.span + N)
        reward = rs.randint(-9, 10, size=(R, N)).astype(np.int32)
        done = _done_values(rs, rs.rand(R, N) < 0.1)
        for g in {0, N - 1}:
            reward[:, g] = (rs.choice([-1, 1], R) * ((1 << 24) + 1 + 2 * rs.randint(0, 1 << 22, R))).astype(np.int32)
        return reward, done, nan_pattern((R, N), salt=R)

    def chronological(self, reward, done):
        """The span's steps oldest first, as plain [span][N] arrays (the ring unrolled)."""
        slots = [(self.played - self.span + i) % self.ring for i in range(self.span)]
        return reward[slots], done[slots], slots


RETRING_CASES = [RetRingCase(*s) for s in RETRING_SHAPES]
