"""Crafted random() draws for the "Lid" factory draw (csrc/azul_selfplay2.hpp: deal_batch2; azul.py:79-89) -- test-only helpers.

The kernels decide a draw with the integer comparison  P_c * 2^53 <= K * T  and fall back to the literal fp64 code only when a multiple of
2^32 lies within the draw margin of K * T.  The draws where the integer answer differs from CPython's fp64 answer are far too rare for
self-play to meet, so the tests put them there: an MT19937 state whose next random() calls return chosen K / 2^53.

  * untemper / words_for_K: the two untempered state words that make random() return exactly K / 2^53;
  * cpython_colour / exact_colour / disagreements: CPython's random.choices arithmetic on Python floats, the exact integer answer, and the
    K near each threshold where the two differ;
  * plan_round: walks a round's draws (the depleted box, the refill from the lid) and writes a chosen K on each draw -- a disagreement K
    on the target draws, random K elsewhere -- into the words before and after a regeneration of the 624-word state; it checks itself
    against CPython's own random() and random.choices on the crafted state."""
import random
from bisect import bisect_right
from itertools import accumulate

import numpy as np

MARGIN = 8192                               # AZ_DRAW_MARGIN (csrc/azul_common.hpp)
TWO53 = 1 << 53
KMAX = TWO53 - 1
N, M = 624, 397
MATRIX_A, UPPER, LOWER = 0x9908B0DF, 0x80000000, 0x7FFFFFFF


def temper(y):
    y ^= y >> 11
    y ^= (y << 7) & 0x9D2C5680
    y ^= (y << 15) & 0xEFC60000
    return (y ^ (y >> 18)) & 0xFFFFFFFF


def untemper(w):
    """The state word y with temper(y) == w."""
    y = w ^ (w >> 18)
    y ^= (y << 15) & 0xEFC60000
    t = y
    for _ in range(4):                      # y ^= (y << 7) & B, 7 bits at a time
        t = y ^ ((t << 7) & 0x9D2C5680)
    y = t & 0xFFFFFFFF
    t = y
    for _ in range(2):                      # y ^= y >> 11
        t = y ^ (t >> 11)
    return t & 0xFFFFFFFF


def words_for_K(K):
    """random() = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 on the tempered words: the untempered pair giving K / 2^53."""
    assert 0 <= K <= KMAX
    return untemper((K >> 26) << 5), untemper((K & ((1 << 26) - 1)) << 6)


def twist_term(a, b):
    """What CPython's regeneration XORs onto old mt[i + 397] to make new mt[i] (i < 227) from old mt[i], mt[i + 1]."""
    y = (a & UPPER) | (b & LOWER)
    return (y >> 1) ^ (MATRIX_A if y & 1 else 0)


def cpython_colour(box, K):
    """random.choices(range(5), weights=[box_c / T ...]) with random() == K / 2^53, the way random.py computes it."""
    T = sum(box)
    cum = list(accumulate([b / T for b in box]))
    total = cum[-1] + 0.0
    return bisect_right(cum, (K * (1.0 / 9007199254740992.0)) * total, 0, 4)


def exact_colour(box, K):
    """#{c < 4 : P_c / T <= K / 2^53}, the exact answer (what the kernels' integer comparison computes)."""
    T = sum(box)
    return sum(P * TWO53 <= K * T for P in list(accumulate(box))[:4])


def in_window(K, T, margin=MARGIN):
    """deal_batch2's test: a multiple of 2^32 lies within `margin` of K * T (the sequential loop's form, u64 wrap included)."""
    KT = K * T
    return ((KT - margin) & (2 ** 64 - 1)) >> 32 != ((KT + margin) & (2 ** 64 - 1)) >> 32


def disagreements(box, span=None):
    """[(K, |K T - P_c 2^53|)] for every K with K T within `span` (default 22 T: beyond the 21.1 T bound) of a threshold P_c 2^53 at which
    CPython's fp64 answer differs from the exact one."""
    T = sum(box)
    span = 22 * T if span is None else span
    out = []
    for P in sorted(set(list(accumulate(box))[:4])):
        lo, hi = max(0, -((span - P * TWO53) // T)), min(KMAX, (P * TWO53 + span) // T)
        for K in range(lo, hi + 1):
            if cpython_colour(box, K) != exact_colour(box, K):
                out.append((K, abs(K * T - P * TWO53)))
    return out


class NoDisagreement(Exception):
    pass


def _put_word(mt, mt0, pos, j, w):
    """Stream word j from index `pos` (j + pos may pass 624): before the regeneration the state word itself, after it (new index
    i < 227) old mt[i + 397], which CPython XORs with a term of old mt[i], mt[i + 1] (unchanged here)."""
    s = pos + j
    if s < N:
        mt[s] = w
    else:
        i = s - N
        assert i < N - M and i + M < min(pos, N), "crafted words must lie in the first 227 words after the regeneration"
        mt[i + M] = w ^ twist_term(int(mt0[i]), int(mt0[i + 1]))


def plan_round(box, lid, mt, pos, ndraws, targets, seed=0, short_deal=False, skip=0):
    """Craft the words of one round's factory draw.

    box, lid: 5 tile counts each at the start of the draw; mt, pos: a 624-word state and its index (0 .. 624); the draw's first random()
    follows `skip` further 32-bit words (the moves before it in the same call);
    ndraws: 4 per display; targets: {t: K} -- K an integer, or None for "a disagreement K of the box this draw sees" (the first one at
    distance >= 2 that is not in the window of the undepleted total when t > 0; NoDisagreement when there is none).  The other draws
    get random K outside the window.

    Returns (mt', draws): the crafted state (pos unchanged) and one dict per draw: t, K, box (before the draw), T, colour (CPython's),
    exact, refilled (the box was refilled from the lid before this draw)."""
    rs = np.random.RandomState(seed)
    mt0 = np.asarray(mt, dtype=np.uint32)
    out = mt0.copy()
    box, lid = [int(x) for x in box], [int(x) for x in lid]
    T0 = sum(box)
    draws = []
    refilled = False
    for t in range(ndraws):
        if sum(box) == 0:
            box, lid, refilled = lid, [0] * 5, True
            T0 = sum(box)
            if T0 == 0:
                assert short_deal, "box and lid empty"
                break
        T = sum(box)
        if t in targets and targets[t] is not None:
            K = int(targets[t])
        elif t in targets:
            cand = [K for K, d in disagreements(box) if d >= 2 and (T == T0 or not in_window(K, T0))]
            if not cand:
                raise NoDisagreement((t, tuple(box)))
            K = cand[rs.randint(len(cand))]
        else:
            while True:
                K = (int(rs.randint(0, 1 << 27)) << 26) | int(rs.randint(0, 1 << 26))
                if not in_window(K, T):
                    break
        a, b = words_for_K(K)
        _put_word(out, mt0, pos, skip + 2 * t, a)
        _put_word(out, mt0, pos, skip + 2 * t + 1, b)
        col = cpython_colour(box, K)
        draws.append({"t": t, "K": K, "box": tuple(box), "T": T, "colour": col, "exact": exact_colour(box, K), "refilled": refilled})
        box[col] -= 1
    _self_check(out, pos, skip, draws)
    return out, draws


def _self_check(mt, pos, skip, draws):
    """CPython itself, on the crafted state: random() returns K / 2^53 for every draw, and random.choices gives the planned colours."""
    state = (3, tuple(int(x) for x in mt) + (int(pos),), None)
    r, c = random.Random(), random.Random()
    r.setstate(state)
    c.setstate(state)
    for _ in range(skip):
        r.getrandbits(32)
        c.getrandbits(32)
    for d in draws:
        assert r.random() == d["K"] / TWO53, d
        assert c.choices(range(5), weights=[b / d["T"] for b in d["box"]])[0] == d["colour"], d


def disagreeing(draws):
    """The draws whose exact answer differs from CPython's: the integer rule alone would get them wrong."""
    return [d for d in draws if d["colour"] != d["exact"]]


def _deal(box, lid, Ks, rule):
    """The displays (colour counts per four draws), box and lid a round's draws leave when `rule(box, K)` decides each one."""
    box, lid, cols = list(box), list(lid), []
    for K in Ks:
        if sum(box) == 0:
            box, lid = lid, [0] * 5
        c = rule(box, K)
        box[c] -= 1
        cols.append(c)
    disp = [tuple(np.bincount(cols[i:i + 4], minlength=5)) for i in range(0, len(cols), 4)]
    return disp, tuple(box), tuple(lid)


def integer_rule_differs(box, lid, draws):
    """The integer rule alone deals another round than CPython (a disagreement can be undone by a later one inside the same display:
    the colours of a display are counted, not ordered)."""
    Ks = [d["K"] for d in draws]
    return _deal(box, lid, Ks, exact_colour) != _deal(box, lid, Ks, cpython_colour)
