"""What azul_lambda_returns_ring must compute -- the TD(lambda) return with critic bootstrap over a trajectory ring -- stated ONCE as a host
model with a case table, in the manner of tests/training_ring_cases.py.  The GPU test (tests/test_gpu_lambda_returns.py) and the lockstep
CPU emulation (tests/test_hostcheck_lambda_returns.py) build their inputs here and compare through compare_returns, so both ask the same;
tests/test_lambda_returns_model.py checks the model itself.

numpy only: no torch, no GPU, no ctypes.  The model is written from the header's contract (include/azul_hip.h), not from the kernel:

    oml = 1.0f - lambda
    v_next = tail ? tail[g] : 0.0f ;  q_next = v_next
    for s = steps_played - 1 down to steps_played - span:
        slot = s % ring_steps ;  r = (float)reward[slot][g] ;  v = value[slot][g]
        if done[slot][g] != 0:  q = r
        else:                   mix = fl(fl(oml * v_next) + fl(lambda * q_next)) ;  q = fl(r + fl(gamma * mix))
        returns[slot][g] = q ;  q_next = q ;  v_next = v

lambda_returns_ring loops over time in Python and applies each float32 operation to all games at once (an elementwise numpy operation on
float32 arrays rounds every element once, so each column is exactly the per-game loop lambda_returns_column spells out; the model test
compares the two).  The device library is compiled without contraction and without fast-math, so the recurrence has ONE float32 result
and the model demands the same bits.  lambda_returns_f64 is the plain high-precision statement with a running bound of float32's distance."""
import numpy as np

from tests.training_ring_cases import compare_returns, nan_pattern        # noqa: F401  (the tests compare through these)

U24 = 2.0 ** -24                 # float32's unit roundoff: fl(x) = x (1 + d), |d| <= U24


# ---------------------------------------------------------------------------------------------------------------- the model
def lambda_returns_ring(reward_ring, done_ring, value_ring, tail, returns_in, gamma, lam, ring_steps, steps_played, span):
    """The ring after the call.  reward int32 / done uint8 / value float32 [ring_steps][N], tail float32 [N] or None, returns_in float32
    [>= ring_steps][N]: slots outside the span (and any rows behind the ring) keep their bits."""
    f32 = np.float32
    out = np.array(returns_in, f32, copy=True)
    g32, l32 = f32(gamma), f32(lam)
    oml = f32(f32(1.0) - l32)                                            # one float32 subtraction
    N = reward_ring.shape[1]
    v_next = np.zeros(N, f32) if tail is None else np.array(tail, f32, copy=True)
    q = v_next.copy()
    for s in range(steps_played - 1, steps_played - 1 - span, -1):
        slot = s % ring_steps
        r = reward_ring[slot].astype(f32)
        mix = np.add(np.multiply(oml, v_next, dtype=f32), np.multiply(l32, q, dtype=f32), dtype=f32)
        q = np.where(done_ring[slot] != 0, r, np.add(r, np.multiply(g32, mix, dtype=f32), dtype=f32)).astype(f32)
        out[slot] = q
        v_next = np.asarray(value_ring[slot], f32)
    return out


def lambda_returns_column(reward, done, value, tail, returns_in, gamma, lam, ring_steps, steps_played, span):
    """The same for ONE game (1-d columns of the ring, tail a number or None) with numpy float32 scalars: the literal per-game loop."""
    f32 = np.float32
    out = np.array(returns_in, f32, copy=True)
    g32, l32 = f32(gamma), f32(lam)
    oml = f32(f32(1.0) - l32)
    v_next = f32(0.0) if tail is None else f32(tail)
    q_next = v_next
    for s in range(steps_played - 1, steps_played - 1 - span, -1):
        slot = s % ring_steps
        r, v = f32(reward[slot]), f32(value[slot])
        if done[slot] != 0:
            q = r
        else:
            mix = f32(f32(oml * v_next) + f32(l32 * q_next))
            q = f32(r + f32(g32 * mix))
        out[slot] = q
        q_next, v_next = q, v
    return out


def lambda_returns_f64(reward_ring, done_ring, value_ring, tail, gamma, lam, ring_steps, steps_played, span):
    """The fp64 twin -- gamma and lambda are the float32 numbers the kernel gets, 1 - lambda is exact in fp64 -- and the running bound of
    float32's distance from it.  With u = 2^-24, every float32 operation fl(x) = x (1 + d), |d| <= u, and E the bound of the step before:
        a = fl(oml32 * v):  oml32 = (1 - lambda)(1 + d), so  |a - (1 - lambda) v| <= Ea = 2u / (1 - 2u) * |(1 - lambda) v|
        b = fl(lambda * q32):               Eb = lambda E + u lambda (|q| + E)
        mix = fl(a + b):                    Em = Ea + Eb + u (|mix| + Ea + Eb)
        p = fl(gamma * mix):                Ep = gamma Em + u gamma (|mix| + Em)
        q = fl((float)r + p):               E' = Er + Ep + u (|r + gamma mix| + Er + Ep),   Er = u |r|  (the int -> float conversion)
    at an episode end q = (float)r: E' = Er.  The values and the tail are float32 inputs, exact.  Returns (returns, bound) [ring_steps][N],
    NaN outside the span."""
    R, N = reward_ring.shape
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    oml = 1.0 - l
    u, g2 = U24, 2 * U24 / (1 - 2 * U24)
    v_next = np.zeros(N, np.float64) if tail is None else np.array(tail, np.float64)
    q, E = v_next.copy(), np.zeros(N, np.float64)
    out, bound = np.full((R, N), np.nan), np.full((R, N), np.nan)
    for s in range(steps_played - 1, steps_played - 1 - span, -1):
        slot = s % ring_steps
        end = done_ring[slot] != 0
        r = reward_ring[slot].astype(np.float64)
        Er = u * np.abs(r)
        Ea = g2 * np.abs(oml * v_next)
        Eb = l * E + u * l * (np.abs(q) + E)
        mix = oml * v_next + l * q
        Em = Ea + Eb + u * (np.abs(mix) + Ea + Eb)
        Ep = g * Em + u * g * (np.abs(mix) + Em)
        full = r + g * mix
        Eq = Er + Ep + u * (np.abs(full) + Er + Ep)
        q, E = np.where(end, r, full), np.where(end, Er, Eq)
        out[slot], bound[slot] = q, E
        v_next = value_ring[slot].astype(np.float64)
    return out, bound


# ---------------------------------------------------------------------------------------------------------------- the cases
# planted columns, in planting order (games 0 .. 5 and, from N >= 12, mirrored at the last six; a lone game holds the case's `lone` kind)
KINDS = ("end_newest", "end_all", "no_end", "end_slot0", "end_last_slot", "big_value")
GUARD_ROWS = 1

# (ring_steps, span, steps_played, N, gamma, lambda, tail present, lone kind)
SHAPES = [
    (1, 1, 7, 1, 0.99, 0.5, True, "no_end"),                 # a ring of one slot: the tail alone feeds it
    (1, 1, 3, 1, 0.99, 0.95, False, "end_newest"),
    (5, 1, 11, 63, 1.0, 0.0, True, None),                    # span 1 in a longer ring, newest in slot 0
    (15, 15, 23, 63, 0.99, 0.95, True, None),                # span = ring, one short batch of loads, newest in the middle: the walk wraps
    (16, 16, 24, 64, 1.0, 1.0, False, None),                 # exactly one batch
    (17, 17, 43, 65, 0.99, 0.0, True, None),                 # one batch and one step
    (33, 33, 50, 257, 0.99, 0.5, False, None),               # two batches and one step, five workgroups
    (33, 33, 82, 64, 1.0, 0.95, True, None),
    (48, 15, 68, 1, 0.0, 0.95, True, "end_all"),             # the ring larger than the span, newest in the middle
    (48, 16, 49, 65, 0.99, 1.0, False, None),                # newest in slot 0: the walk wraps at once
    (48, 17, 96, 63, 1.0, 0.5, False, None),                 # newest in the last slot
    (48, 33, 60, 257, 0.99, 0.95, True, None),               # newest in the middle, the walk wraps through slot 0 and the last slot
    (16, 15, 33, 65, 0.0, 1.0, False, None),
    (20, 17, 2 ** 33 + 17, 64, 0.99, 0.95, False, None),     # a step clock beyond int32 (the entry reduces it on the host): newest in slot 8
    (17, 16, 35, 1, 0.99, 1.0, True, "no_end"),              # lambda = 1 with a tail: the Monte-Carlo return bootstrapped at the window's end
    (33, 17, 40, 1, 1.0, 0.0, False, "big_value"),
]


class Case:
    """A ring [ring_steps][N] for azul_lambda_returns_ring.  Rewards are -30 .. 30 (score differences), values N(0, 5) as float32, an end
    with probability 0.1 (flags 1 .. 3); the tail, when present, N(0, 5).  The returns ring starts as a NaN pattern with GUARD_ROWS rows
    behind it: slots outside the span and the guard keep it bit for bit.  Planted columns (self.planted: kind -> games):
      end_newest     an end at the newest step only: the tail (planted as 1e6) must not leak in
      end_all        an end at every step: returns = rewards
      no_end         no end: the tail flows through the whole span
      end_slot0      the only end in slot 0
      end_last_slot  the only end in slot ring_steps - 1
      big_value      values (and the tail) of magnitude up to 1e4, rewards -200 .. 200, no end"""

    def __init__(self, ring, span, played, N, gamma, lam, tail, lone):
        self.ring, self.span, self.played, self.N, self.gamma, self.lam, self.tail, self.lone = ring, span, played, N, gamma, lam, tail, lone
        self.newest = (played - 1) % ring
        self.where = "first" if self.newest == 0 else ("last" if self.newest == ring - 1 else "middle")
        self.wraps = span > self.newest + 1
        fmt = lambda x: ("%g" % x).replace(".", "p")
        self.id = "lam-R%d-span%d-N%d-%s-g%s-l%s-%s%s" % (ring, span, N, self.where if ring > 1 else "one", fmt(gamma), fmt(lam),
                                                        "tail" if tail else "notail", "-2p33" if played > 2 ** 31 else "")

    def plan(self):
        """kind -> games, from the shape alone."""
        N = self.N
        if N == 1:
            return {self.lone: [0]}
        spots = [(i, k) for i, k in enumerate(KINDS) if i < N]
        if N >= 2 * len(KINDS):
            spots += [(N - 1 - i, k) for i, k in enumerate(KINDS)]
        planted = {}
        for g, k in spots:
            planted.setdefault(k, []).append(g)
        return planted

    def build(self):
        """(reward, done, value, tail or None, returns_in [ring + GUARD_ROWS][N])"""
        R, N = self.ring, self.N
        rs = np.random.RandomState(7000 + 3 * R + 29 * self.span + N)
        reward = rs.randint(-30, 31, size=(R, N)).astype(np.int32)
        done = ((rs.rand(R, N) < 0.1) * rs.randint(1, 4, size=(R, N))).astype(np.uint8)
        value = (rs.randn(R, N) * 5).astype(np.float32)
        tail = (rs.randn(N) * 5).astype(np.float32) if self.tail else None
        self.planted = self.plan()
        for k, games in self.planted.items():
            for g in games:
                done[:, g] = 0
                if k == "end_newest":
                    done[self.newest, g] = 1
                    if tail is not None:
                        tail[g] = np.float32(1e6)
                elif k == "end_all":
                    done[:, g] = rs.randint(1, 4, size=R)
                elif k == "end_slot0":
                    done[0, g] = 2
                elif k == "end_last_slot":
                    done[R - 1, g] = 3
                elif k == "big_value":
                    value[:, g] = (rs.uniform(-1e4, 1e4, size=R)).astype(np.float32)
                    value[rs.randint(0, R), g] = np.float32(-1e4)
                    reward[:, g] = rs.randint(-200, 201, size=R)
                    if tail is not None:
                        tail[g] = np.float32(1e4)
        return reward, done, value, tail, nan_pattern((R + GUARD_ROWS, N), salt=R)

    def slots(self):
        """The span's slots, newest first."""
        return [(self.played - 1 - i) % self.ring for i in range(self.span)]


CASES = [Case(*s) for s in SHAPES]
