"""The arithmetic fact the "Lid" factory draw rests on (csrc/azul_selfplay2.hpp: deal_batch2, the comment above deal2), checked
against CPython's own random.choices arithmetic (random.py: accumulate of box_c / T, total = cum[-1] + 0.0, bisect_right(cum, random() *
total, 0, 4)) -- no device code involved:
  * wherever no multiple of 2^32 lies within AZ_DRAW_MARGIN = 8192 of K * T, the integer rule P_c * 2^53 <= K * T is CPython's answer --
    for every total T = 1 .. 255 (record_in_domain's limit), several boxes per total plus edge boxes and the depleted boxes of a round,
    every prefix P_c, every K with K * T within 3 * 8192 of P_c * 2^53, and K = 0, 1, 2^53 - 2, 2^53 - 1;
  * inside the window the two answers do differ (the fp64 fallback is needed), and never further than 21.1 * T from the threshold --
    the bound the comment argues, per total.
tests/test_hostcheck_deal_margins.py and tests/test_gpu_deal_margins.py feed the disagreement draws found here to the kernels."""
import random
from itertools import accumulate

import numpy as np

from tests import deal_craft as dc

SPAN = 3 * dc.MARGIN
EDGE_K = np.array([0, 1, dc.TWO53 - 2, dc.TWO53 - 1], dtype=np.int64)


def boxes_for(T, rs):
    """Four random boxes of total T plus the edge boxes that total T allows."""
    out = []
    for _ in range(4):
        cuts = np.sort(rs.randint(0, T + 1, size=4))
        out.append(tuple(int(x) for x in np.diff(np.concatenate([[0], cuts, [T]]))))
    for c in range(5):                                    # a single colour
        out.append(tuple(T if i == c else 0 for i in range(5)))
    if T >= 2:                                            # zero-count colours between non-zero ones
        out.append((T // 2, 0, 0, 0, T - T // 2))
        out.append((0, T - T // 2, 0, T // 2, 0))
    if T == 100:
        out.append((20, 20, 20, 20, 20))
    if T == 255:
        out += [(51, 51, 51, 51, 51), (1, 1, 1, 1, 251), (251, 1, 1, 1, 1), (127, 0, 128, 0, 0)]
    return out


def depleted_boxes(rs, count=60):
    """The boxes a round's draws leave behind: P_c - n_c(t) over T0 - t for t <= 36 (the nine-display deal), from random starting boxes."""
    out = []
    for _ in range(count):
        T0 = int(rs.randint(37, 256))
        cuts = np.sort(rs.randint(0, T0 + 1, size=4))
        box = [int(x) for x in np.diff(np.concatenate([[0], cuts, [T0]]))]
        for _t in range(36):
            c = int(rs.choice(5, p=np.array(box) / sum(box)))
            box[c] -= 1
            out.append(tuple(box))
    return out


def sweep_box(box):
    """(K array, distance to the nearest threshold, CPython's colour, exact colour, in-window flag) for every K within SPAN of a threshold."""
    T = sum(box)
    cum = list(accumulate([b / T for b in box]))
    total = cum[-1] + 0.0
    Ps = sorted(set(list(accumulate(box))[:4]))
    ks = [EDGE_K]
    for P in Ps:
        lo, hi = max(0, -((SPAN - P * dc.TWO53) // T)), min(dc.KMAX, (P * dc.TWO53 + SPAN) // T)
        ks.append(np.arange(lo, hi + 1, dtype=np.int64))
    K = np.unique(np.concatenate(ks))
    KT = K * T                                            # < 2^61
    x = (K.astype(np.float64) * (1.0 / 9007199254740992.0)) * total    # random() * total, both roundings as CPython does them
    cpy = np.searchsorted(np.array(cum[:4]), x, side="right")          # bisect_right(cum, x, 0, 4)
    thr = np.array([P * dc.TWO53 for P in list(accumulate(box))[:4]], dtype=np.int64)
    exact = (thr[None, :] <= KT[:, None]).sum(axis=1)
    dist = np.abs(KT[:, None] - np.array([P * dc.TWO53 for P in Ps], dtype=np.int64)[None, :]).min(axis=1)
    u = KT.astype(np.uint64)
    m = np.uint64(dc.MARGIN)
    with np.errstate(over="ignore"):
        window = ((u - m) >> np.uint64(32)) != ((u + m) >> np.uint64(32))          # the sequential loop's test (u64 wrap below the margin)
        lo = (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        risky = (lo + np.uint32(dc.MARGIN)) < np.uint32(2 * dc.MARGIN)             # the fixed point's half-ballot test on the low word
    assert np.array_equal(window, risky), box
    return K, dist, cpy, exact, window


def test_untemper_and_crafted_words_reproduce_cpython_random():
    rs = random.Random(7)
    for _ in range(20000):
        y = rs.getrandbits(32)
        assert dc.untemper(dc.temper(y)) == y
    r = random.Random()
    for K in [0, 1, dc.TWO53 - 2, dc.TWO53 - 1] + [rs.getrandbits(53) for _ in range(300)]:
        pos = rs.randrange(0, 623)
        mt = [rs.getrandbits(32) for _ in range(624)]
        mt[pos], mt[pos + 1] = dc.words_for_K(K)
        r.setstate((3, tuple(mt) + (pos,), None))
        assert r.random() == K / dc.TWO53


def test_literal_fp64_rule_is_random_choices():
    """The fp64 model used below is random.choices itself: a few hundred draws on crafted states, near thresholds and anywhere."""
    rs = np.random.RandomState(3)
    r = random.Random()
    n = 0
    for T in list(range(1, 30)) + [99, 100, 101, 200, 254, 255]:
        for box in boxes_for(T, rs)[:4]:
            Ks = [K for K, _ in dc.disagreements(box)][:4] + [int(rs.randint(0, 1 << 30)) << 23 | int(rs.randint(0, 1 << 23)) for _ in range(3)]
            for K in Ks:
                mt = [int(x) for x in rs.randint(0, 2 ** 32, size=624, dtype=np.uint64)]
                mt[100], mt[101] = dc.words_for_K(K)
                r.setstate((3, tuple(mt) + (100,), None))
                assert r.choices(range(5), weights=[b / T for b in box])[0] == dc.cpython_colour(box, K), (box, K)
                n += 1
    assert n > 300


def test_integer_rule_equals_cpython_outside_the_window_and_the_window_is_needed():
    rs = np.random.RandomState(11)
    worst = np.zeros(256, np.int64)
    checked = outside = inside_disagree = 0
    sets = [(T, boxes_for(T, rs)) for T in range(1, 256)]
    dep = {}
    for b in depleted_boxes(rs):
        dep.setdefault(sum(b), []).append(b)
    for T, boxes in sets + sorted(dep.items()):
        for box in boxes:
            K, dist, cpy, exact, window = sweep_box(box)
            bad = cpy != exact
            assert not (bad & ~window).any(), (box, K[bad & ~window][:5])
            checked += K.size
            outside += int((~window).sum())
            inside_disagree += int(bad.sum())
            if bad.any():
                worst[T] = max(worst[T], int(dist[bad].max()))
    Ts = np.arange(256)
    assert (worst <= 21.1 * Ts).all(), [(int(t), int(worst[t])) for t in Ts[worst > 21.1 * Ts]]
    print("\nfactory draw: %d decisions, %d outside the window (0 disagreements), %d disagreements inside it" % (checked, outside, inside_disagree))
    print("worst disagreement distance |K T - P_c 2^53| per total T (bound 21.1 T; 0: none found):")
    for t0 in range(1, 256, 16):
        print("  " + " ".join("%3d:%4d" % (t, worst[t]) for t in range(t0, min(t0 + 16, 256))))
    print("maximum %d at T = %d (21.1 T = %.0f)" % (worst.max(), worst.argmax(), 21.1 * worst.argmax()))
    assert checked > 3_000_000 and outside > 0
    assert inside_disagree > 0                            # the fallback is needed
    assert 0 < worst.max() <= 21.1 * 255 < dc.MARGIN


def test_edge_K_decide_like_cpython():
    """K = 0 and K = 2^53 - 1 on every box of every total: the window test wraps below the margin (K T < 8192) and the answers agree."""
    rs = np.random.RandomState(2)
    for T in range(1, 256):
        for box in boxes_for(T, rs):
            for K in (0, 1, dc.TWO53 - 2, dc.TWO53 - 1):
                assert dc.cpython_colour(box, K) == dc.exact_colour(box, K), (box, K)
            assert dc.in_window(0, T) and dc.in_window(1, T)
