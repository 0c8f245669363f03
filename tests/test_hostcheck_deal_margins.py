"""The factory draw's window check under the lockstep emulation (tests/hostcheck/simt, the UNMODIFIED product headers), fed the draws where
the integer rule P_c * 2^53 <= K * T is wrong (tests/deal_craft.py): CPython's answer must come out all the same, through every place the
window check lives in csrc/azul_selfplay2.hpp (deal_batch2) -- the low-word test of the fixed point, the depleted totals T0 - t, the half
ballot of the two games of a wave, the lane that owns draw t, the batch after a lid refill, the words after an MT19937 regeneration, and
K * T below the margin (the sequential loop's wrap).  Three emulations: the rule kernel (azul_op_kernel: new_round), the P-player kernel
(azul_x_op_kernel: 3 / 4 players with 2P + 1 displays, a 32 + 4 split deal) and the benchmarked self-play loop (azul_selfplay2_kernel at a
round boundary).  Each run is compared with the oracle -- record bytes (box, lid, displays), all 624 MT words and the index.

Negative control: the same crafted draws with a draw margin of 1 (the emulation accepts it; the ABI refuses it) are decided by the integer
rule alone and must come out DIFFERENT from the oracle on every case that carries a disagreement draw -- the craft reaches the draws the
fallback exists for."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import deal_craft as dc
from tests.hostcheck import hostcheck as hc
from tests.test_hostcheck_selfplay2 import check_case, load, run_case

OL = oz.lib()


def _rng(mt, pos):
    r = oz.Rng()
    OL.oz_rng_set(C.byref(r), np.ascontiguousarray(mt, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), int(pos))
    return r


def _plan(box, lid, mt, pos, ndraws, targets, seed=0, skip=0, control=True):
    """deal_craft.plan_round, refused (NoDisagreement) unless the integer rule alone deals another round: the negative control's premise."""
    mt, draws = dc.plan_round(box, lid, mt, pos, ndraws, targets, seed=seed, skip=skip)
    if control and not dc.integer_rule_differs(box, lid, draws):
        raise dc.NoDisagreement("the integer rule's errors cancel")
    return mt, draws


def _find(make, tries=400):
    """make(seed) -> a planned case, or NoDisagreement: the first seed that plans."""
    for seed in range(tries):
        try:
            return make(seed)
        except dc.NoDisagreement:
            continue
    raise AssertionError("no box with the wanted disagreement draws in %d tries" % tries)


def _random_box(rs, lo, hi):
    T = int(rs.randint(lo, hi + 1))
    cuts = np.sort(rs.randint(0, T + 1, size=4))
    return [int(x) for x in np.diff(np.concatenate([[0], cuts, [T]]))]


# ---- the case catalogue of one round's factory draw: (name, box, lid, pos, targets) -------------------------------------------------
def catalogue(ndraws):
    """ndraws = 20 (two players, five displays), 28 or 36 (3 / 4 players, 2P + 1 displays)."""
    last = ndraws - 1
    specs = [("a_first", (20, 255), {0: None}), ("a_middle", (20, 255), {ndraws // 2 - 1: None}), ("a_last_lane", (20, 255), {min(last, 19): None}),
             ("b_depleted_total", (20, 60), {last: None})]
    if ndraws > 32:
        specs += [("g_second_batch", (36, 120), {33: None}), ("g_display5", (36, 120), {21: None})]
    elif ndraws > 20:
        specs += [("g_display6", (28, 120), {25: None})]
    cases = []
    for name, (lo, hi), targets in specs:
        def make(seed, lo=lo, hi=hi, targets=targets, name=name):
            rs = np.random.RandomState(1000 * len(cases) + seed)
            box = _random_box(rs, max(lo, ndraws), hi)
            lid = _random_box(rs, 0, 40)
            mt = rs.randint(0, 2 ** 32, size=624, dtype=np.uint64).astype(np.uint32)
            pos = int(rs.randint(0, 624 - 2 * ndraws))
            return (name, box, lid, pos) + _plan(box, lid, mt, pos, ndraws, targets, seed=seed)
        cases.append(_find(make))

    # c: fewer tiles in the box than the round draws: one batch of T draws, the refill from the lid, a second batch
    def make_refill(seed):
        rs = np.random.RandomState(5000 + seed)
        box = _random_box(rs, 6, min(ndraws - 3, 30))
        T = sum(box)
        lid = _random_box(rs, ndraws - T + 20, 120)
        mt = rs.randint(0, 2 ** 32, size=624, dtype=np.uint64).astype(np.uint32)
        pos = int(rs.randint(0, 624 - 2 * ndraws))
        return ("c_refill", box, lid, pos) + _plan(box, lid, mt, pos, ndraws, {T // 2: None, T + 1: None}, seed=seed)
    cases.append(_find(make_refill))

    # e: the round's words straddle the regeneration (CPython's index 586 .. 623 when the round starts): a disagreement on the draw whose
    # words hold (odd index: straddle) the first words of the new state, and on the last draw
    for pos in range(624 - 2 * 20, 624):
        def make_twist(seed, pos=pos):
            rs = np.random.RandomState(7000 + 100 * pos + seed)
            box = _random_box(rs, max(ndraws, 20), 200)
            lid = _random_box(rs, 0, 40)
            mt = rs.randint(0, 2 ** 32, size=624, dtype=np.uint64).astype(np.uint32)
            return ("e_twist_%d" % pos, box, lid, pos) + _plan(box, lid, mt, pos, ndraws, {(624 - pos) // 2: None, last: None}, seed=seed)
        cases.append(_find(make_twist))

    # f: K = 0 and K = 2^53 - 1 (K * T below the margin: the window test wraps); no disagreement there, just the answer
    rs = np.random.RandomState(77)
    box, lid = [30, 0, 25, 20, 25], [3, 4, 5, 6, 7]
    mt = rs.randint(0, 2 ** 32, size=624, dtype=np.uint64).astype(np.uint32)
    targets = {0: 0, 1: dc.KMAX, 5: 1, 6: dc.KMAX - 1, last - 1: 0, last: dc.KMAX}
    cases.append(("f_edge_K", box, lid, 100) + dc.plan_round(box, lid, mt, 100, ndraws, targets, seed=1))
    for name, box, lid, pos, mt, draws in cases:
        assert name.startswith("f_") or dc.disagreeing(draws), name
        if name.startswith("c_"):
            assert any(d["refilled"] for d in dc.disagreeing(draws)) and any(not d["refilled"] for d in dc.disagreeing(draws))
        if name.startswith("b_"):
            d = dc.disagreeing(draws)[-1]
            assert d["t"] > 0 and not dc.in_window(d["K"], sum(box)) and sum(box) != d["T"]
    return cases


# ---- the rule kernel: new_round on one record --------------------------------------------------------------------------------------------
def _two_player_record(box, lid, seed=41):
    rec = oz.Stream(seed).advance(1 + seed % 7)["rec_after"][-1].copy()
    rec["box"], rec["lid"] = box, lid
    return rec


def rule_kernel_new_round(rec, mt, pos, margin=0):
    e = hc.EmuBackend(oz.FIRST_RANDOM, oz.POOL_LID)
    e.put(rec)
    e.mt[:] = mt
    e.pos[0] = pos
    st = e._op("new_round", margin=margin)["status"]
    return st, e.rec.tobytes(), e.mt.copy(), int(e.pos[0])


def oracle_new_round(rec, mt, pos):
    q, r = oz.unpack(rec, oz.POOL_LID, oz.FIRST_RANDOM), _rng(mt, pos)
    st = OL.oz_new_round(C.byref(q.game), C.byref(r))
    return st, oz.pack(q).tobytes(), np.ctypeslib.as_array(r.mt).copy(), int(r.idx)


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.fixture(scope="module")
def cat20():
    return catalogue(20)


def test_rule_kernel_new_round_on_crafted_draws_equals_the_oracle(cat20):
    for name, box, lid, pos, mt, draws in cat20:
        rec = _two_player_record(box, lid)
        want = oracle_new_round(rec, mt, pos)
        assert want[0] == 0, name
        got = rule_kernel_new_round(rec, mt, pos)
        assert _same(got, want), name
        disp = np.frombuffer(want[1], np.uint8)[:25].reshape(5, 5)
        for d in range(5):                                  # the planned colours are the oracle's: the craft hit the draws it aimed at
            assert list(disp[d]) == list(np.bincount([x["colour"] for x in draws[4 * d:4 * d + 4]], minlength=5)), name


def test_rule_kernel_negative_control_margin_one_differs_on_the_disagreement_draws(cat20):
    differ = 0
    for name, box, lid, pos, mt, draws in cat20:
        rec = _two_player_record(box, lid)
        got, want = rule_kernel_new_round(rec, mt, pos, margin=1), oracle_new_round(rec, mt, pos)
        if name.startswith("f_"):
            assert _same(got, want), name                   # no disagreement on the edge K: the integer rule is right there
        else:
            assert got[1] != want[1], name                  # the integer rule alone deals another colour
            differ += 1
    assert differ >= 40


# ---- the P-player kernel: 3 / 4 players, 2P + 1 displays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("players", [3, 4])
def test_rules_x_new_round_on_crafted_draws_equals_the_oracle(players):
    ext = hc.EXT_DISPLAYS_2P1
    D = 2 * players + 1
    cases = catalogue(4 * D)
    s = oz.StreamX(60 + players, players, oz.FIRST_RANDOM, oz.POOL_LID, ext)
    s.advance(3)
    base = s.record().copy()
    for name, box, lid, pos, mt, draws in cases:
        rec = base.copy()
        rec["box"], rec["lid"] = box, lid
        g, r = oz.unpack_np(rec, oz.POOL_LID, ext), _rng(mt, pos)
        assert OL.oz_new_round(C.byref(g), C.byref(r)) == 0, name
        want = oz.pack_np(g).tobytes()
        for margin in (0, 1):
            raw = np.frombuffer(rec.tobytes(), np.uint8).copy()
            emt, epos = mt.copy(), np.array([pos], np.uint32)
            out = hc.x_op(raw, players, oz.FIRST_RANDOM, oz.POOL_LID, ext, "new_round", 0, emt, epos, margin=margin)
            assert out["status"] == 0, name
            same = raw.tobytes() == want and np.array_equal(emt, np.ctypeslib.as_array(r.mt)) and int(epos[0]) == r.idx
            if margin == 0 or name.startswith("f_"):
                assert same, (name, margin)
            else:
                assert raw.tobytes() != want, name           # negative control: the integer rule alone deals another colour
        if name.startswith("g_second"):
            assert dc.disagreeing(draws)[-1]["t"] >= 32


# ---- the benchmarked self-play loop at a round boundary ----------------------------------------------------------------------------------
def _clone(s):
    c = oz.Stream.__new__(oz.Stream)
    c.q, c.r = oz.Runner.from_buffer_copy(s.q), oz.Rng.from_buffer_copy(s.r)
    c.stuck, c.episodes, c.stats_sum = C.c_uint64(s.stuck.value), C.c_uint64(s.episodes.value), s.stats_sum.copy()
    return c


def _probe(s):
    """If the stream's next move ends a round (and not the game): (words of that move before its factory draw, box, lid the draw starts
    from, displays after it); else None."""
    c = _clone(s)
    w0, rec0 = c.r.words, c.record().copy()
    c.advance(1, want_records=False)
    rec1 = c.record()
    if int(rec1["turn_counter"]) != int(rec0["turn_counter"]) + 1 or c.episodes.value != s.episodes.value or c.stuck.value != s.stuck.value:
        return None
    drawn = rec1["displays"].sum(axis=0).astype(int)
    lid = rec1["lid"].astype(int) + rec1["box"].astype(int) + drawn - rec0["box"].astype(int)     # the lid after count_score
    return int(c.r.words - w0) - 40, [int(x) for x in rec0["box"]], [int(x) for x in lid], rec1["displays"].copy()


def craft_at_boundary(s, targets, want_box=None, draw_pos=None, max_moves=2000):
    """Advance oracle stream `s` to the move before a round's factory draw that can carry `targets` (want_box(box, lid) filters the
    rounds; a tuple (box, lid) replaces them), optionally moving CPython's index so that the draw starts at `draw_pos`, and write the crafted words into its state.
    Returns the planned draws."""
    for _ in range(max_moves):
        p = _probe(s)
        if p is not None and (want_box is None or isinstance(want_box, tuple) or want_box(p[1], p[2])):
            if isinstance(want_box, tuple):                 # another box and lid at the round's end (the state is the record)
                np.ctypeslib.as_array(s.q.game.box)[:], np.ctypeslib.as_array(s.q.game.lid)[:] = want_box
                p = _probe(s)
            if draw_pos is not None:
                s.r.idx = draw_pos - p[0]
                p = _probe(s)
                assert p is not None
            skip, box, lid, _ = p
            mt = None
            for seed in range(30):                         # other random draws before a target: other depleted boxes at it
                try:
                    mt, draws = _plan(box, lid, np.ctypeslib.as_array(s.r.mt), int(s.r.idx), 20, targets, seed=seed, skip=skip,
                                      control=any(v is None for v in targets.values()))
                    break
                except dc.NoDisagreement:
                    continue
            if mt is not None:
                np.ctypeslib.as_array(s.r.mt)[:] = mt
                disp = _probe(s)[3]
                for d in range(5):                          # the oracle deals the planned colours: the offset and the refill are right
                    assert list(disp[d]) == list(np.bincount([x["colour"] for x in draws[4 * d:4 * d + 4]], minlength=5))
                return draws
        s.advance(1, want_records=False)
    raise AssertionError("no round boundary that carries the targets")


SELFPLAY_RUNS = {
    # name: per game (targets, want_box, draw_pos); two games per wave
    "a_b_lanes": [({0: None}, None, None), ({9: None}, None, None), ({19: None}, None, None), ({14: None}, lambda b, l: sum(b) < 60, None)],
    "c_refill": [({2: None, 16: None}, ([3, 0, 4, 2, 3], [14, 20, 9, 11, 17]), None), ({}, None, None),
                 ({5: None, 19: None}, ([1, 4, 0, 6, 6], [1, 2, 30, 2, 1]), None), ({8: None}, ([2, 2, 2, 0, 1], [40, 40, 40, 40, 40]), None)],
    "d_half_ballot": [({7: None}, None, None), ({}, None, None), ({}, None, None), ({11: None}, None, None), ({2: None}, None, None),
                      ({16: None}, None, None)],
    "e_regeneration": [({19: None}, None, 586), ({(624 - 601) // 2: None}, None, 601), ({0: None}, None, 622), ({1: None}, None, 623)],
    "f_edge_K": [({0: 0, 1: dc.KMAX, 18: 1, 19: dc.KMAX - 1}, None, None), ({3: dc.KMAX, 4: 0}, None, None)],
}
SEED0 = {"a_b_lanes": 2100, "c_refill": 2200, "d_half_ballot": 2300, "e_regeneration": 2400, "f_edge_K": 2500}


def _prepare(run, planned):
    def prepare(streams):
        planned.clear()
        for s, (targets, want_box, draw_pos) in zip(streams, SELFPLAY_RUNS[run]):
            planned.append(craft_at_boundary(s, targets, want_box, draw_pos))
            s.episodes.value, s.stuck.value, s.stats_sum[:] = 0, 0, 0.0     # the kernel's counters start from zero
    return prepare


@pytest.mark.parametrize("run", sorted(SELFPLAY_RUNS))
def test_selfplay_loop_deals_crafted_draws_like_the_oracle(run):
    """Every game of the run ends a round on its first move; the crafted draw decides the new round's displays.  Outputs, records, all MT
    words + index, counters: the oracle's.  Then the negative control (margin 1): exactly the games that carry a disagreement draw differ."""
    L = load()
    n, planned = len(SELFPLAY_RUNS[run]), []
    check_case(L, 0, 1, n=n, T=6, variant=3, seed0=SEED0[run], prepare=_prepare(run, planned))
    carries = [bool(dc.disagreeing(d)) for d in planned]
    assert carries == [bool(t) and not run.startswith("f_") for t, _, _ in SELFPLAY_RUNS[run]]
    if run == "c_refill":
        assert {d["refilled"] for g in planned for d in dc.disagreeing(g)} == {False, True}
    streams, state, mt, pos, *_ = run_case(L, 0, 1, n=n, T=6, variant=3, seed0=SEED0[run], margin=1, prepare=_prepare(run, []))
    for g, s in enumerate(streams):
        s.advance(6, want_records=False)
        assert (state[g].tobytes() != s.record().tobytes()) == carries[g], (run, g)
