"""The host model of the returns scans and episode selectors (tests/training_ring_cases.py) is worth trusting BEFORE a kernel is compared
with it -- numpy alone, no GPU, no emulation: the float32 scan stays inside the running bound of its fp64 twin, the ring scan is the
window scan chained through the carry, a ring sequence hands out every step exactly once, the single-window selector is the ring
selector with one window, the shifted clock changes nothing but the clock, and every planted edge is really in its case."""
import numpy as np
import pytest

from tests import training_ring_cases as M

ids = lambda cases: [c.id for c in cases]


# ---------------------------------------------------------------------------------------------------------------- the scans
@pytest.mark.parametrize("case", M.WINDOW_CASES, ids=ids(M.WINDOW_CASES))
def test_float32_window_scan_lies_within_the_running_bound_of_its_fp64_twin(case):
    reward, done, carry = case.build()
    got, carry_out = M.returns_window(reward, done, case.gamma, carry)
    q64, bound = M.returns_window_f64(reward, done, case.gamma, carry)
    err = np.abs(got.astype(np.float64) - q64)
    assert (err <= bound).all(), (case.id, float((err - bound).max()))
    assert np.array_equal(carry_out.view(np.int32), got[0].view(np.int32))         # what flows out is the first step's return
    # the literal per-game loop on the planted columns and a few others: the same bits as the all-games-at-once form
    cols = sorted({g for gs in case.planted.values() for g in gs} | {case.N // 2, case.N // 3})
    for g in cols:
        col, c_out = M.returns_column(reward[:, g], done[:, g], case.gamma, None if carry is None else carry[g])
        M.compare_returns(case.id, got[:, g], col, "column %d" % g)
        assert np.float32(c_out).view(np.int32) == carry_out[g].view(np.int32)
    # the planted edges are there and do what they are planted for
    T = case.T
    for g in case.planted.get("end_last", []):
        assert done[T - 1, g] != 0 and np.flatnonzero(done[:, g]).tolist() == [T - 1]
        if carry is not None:                                   # the 1e6 flowing in is cut: the last step's return is its reward
            assert carry[g] == np.float32(1e6) and got[T - 1, g] == np.float32(reward[T - 1, g])
    for g in case.planted.get("end_first", []):
        assert np.flatnonzero(done[:, g]).tolist() == [0]
    for g in case.planted.get("no_end", []):
        assert not done[:, g].any()
        if carry is not None and case.gamma != 0:
            assert carry_out[g] != M.returns_window(reward, done, case.gamma, None)[1][g]          # the carry reaches carry_out
    for g in case.planted.get("big", []):
        assert (np.abs(reward[:, g]) > (1 << 24)).all() and (reward[:, g].astype(np.float32).astype(np.int64) != reward[:, g]).all()
    for g in case.planted.get("pm200", []):
        assert set(np.abs(reward[:, g]).tolist()) == {200}
    if case.N > 1:
        assert sorted(case.planted) == sorted(M.WINDOW_KINDS) and all(0 in gs or case.N - 1 in gs or len(gs) == 2 for gs in case.planted.values())


def test_the_window_table_covers_what_it_promises():
    shapes = M.WINDOW_SHAPES
    assert {s[0] for s in shapes} == {1, 255, 256, 257, 1000} and {s[1] for s in shapes} == {1, 2, 33, 200}
    assert {s[2] for s in shapes} == {0.0, 0.99, 1.0} and {s[3] for s in shapes} == {False, True}
    shapes = M.RETRING_SHAPES
    assert {s[0] for s in shapes} == {1, 5, 16, 17, 48} and {s[3] for s in shapes} == {1, 63, 64, 65, 1000}
    assert {1, 15, 16, 17} <= {s[1] for s in shapes} and all(any(s[0] == r and s[1] == r for s in shapes) for r in (1, 5, 16, 17, 48))
    assert {c.where for c in M.RETRING_CASES if c.ring > 1} == {"first", "last", "middle"}
    assert any(s[2] == 2 ** 33 + 5 for s in shapes)
    assert len({c.id for c in M.WINDOW_CASES + M.RETRING_CASES + M.COMPLETE_CASES + M.RING_CASES + M.SHIFT_CASES}) == \
        len(M.WINDOW_CASES + M.RETRING_CASES + M.COMPLETE_CASES + M.RING_CASES + M.SHIFT_CASES)
    assert [(c.N, c.T) for c in M.COMPLETE_CASES][:5] == [(1, 0), (63, 1), (1024, 64), (1025, 65), (2500, 130)]
    assert [(c.N, c.T, c.D) for c in M.RING_CASES] == [(1, 1, 1), (3, 8, 2), (5, 64, 2), (1023, 8, 3), (1029, 8, 3), (6, 65, 2), (7, 100, 3)]


@pytest.mark.parametrize("case", M.RETRING_CASES, ids=ids(M.RETRING_CASES))
def test_ring_scan_is_the_window_scan_chained_through_the_carry(case):
    reward, done, ret_in = case.build()
    got = M.returns_ring(reward, done, ret_in, case.gamma, case.ring, case.played, case.span)
    r, d, slots = case.chronological(reward, done)
    assert slots[-1] == case.newest and len(set(slots)) == case.span
    # window by window, newest first; windows of the case's own T when it has one, else of 1, 2, 3, ... steps
    want = np.zeros((case.span, case.N), np.float32)
    carry, hi, k = np.zeros(case.N, np.float32), case.span, 1
    while hi > 0:
        lo = max(0, hi - (case.window or k))
        want[lo:hi], carry = M.returns_window(r[lo:hi], d[lo:hi], case.gamma, carry)
        hi, k = lo, k + 1
    M.compare_returns(case.id, got[slots], want, "ring scan vs chained windows")
    q64, bound = M.returns_window_f64(r, d, case.gamma, None)
    assert (np.abs(got[slots].astype(np.float64) - q64) <= bound).all()
    outside = [s for s in range(case.ring) if s not in slots]
    M.compare_returns(case.id, got[outside], ret_in[outside], "slots outside the span")
    assert np.isnan(ret_in).all() and len(outside) == case.ring - case.span
    assert (np.abs(reward[:, 0]) > (1 << 24)).all()


# ---------------------------------------------------------------------------------------------------------------- the selectors
@pytest.mark.parametrize("case", M.COMPLETE_CASES, ids=ids(M.COMPLETE_CASES))
def test_single_window_selector_and_its_planted_columns(case):
    done, action = case.build()
    N, T = case.N, case.T
    index, count = M.select_complete(done, action)
    assert count == len(index) == len(set(index))
    games = [i % N for i in index]
    assert games == sorted(games) and all(a < b for a, b in zip(index, index[1:]) if a % N == b % N)      # game by game, steps ascending
    keep = (np.cumsum(done[::-1] != 0, axis=0)[::-1] > 0) & (action >= 0)                                  # vectorised restatement
    assert sorted(index) == np.flatnonzero(keep.reshape(-1)).tolist()
    if T > 0:
        # the ring selector with one window of T steps on the same arrays: the same list
        ix, pend, dropped = M.select_ring(done, action, T, 1, T, np.zeros(N, np.int64))
        assert ix == index and dropped == 0
    else:
        assert count == 0
    # every planted kind that T allows is there, in the first and the last game of every chunk of 1024
    last = np.array([np.flatnonzero(done[:, g])[-1] if done[:, g].any() else -1 for g in range(N)])
    per_game = np.bincount(np.array(games, np.int64), minlength=N) if index else np.zeros(N, np.int64)
    if N > 1:
        assert sorted(case.planted) == sorted(case.kinds())
        planted = {g for gs in case.planted.values() for g in gs}
        for c0 in range(0, N, 1024):
            assert c0 in planted and min(c0 + 1024, N) - 1 in planted
            size = min(c0 + 1024, N) - c0
            here = {k: sum(1 for g in case.planted[k] if c0 <= g < c0 + 1024) for k in case.kinds()}
            assert sum(here.values()) == min(size, 2 * len(here)), (c0, here)
            assert size < 2 * len(here) or set(here.values()) == {2}, (c0, here)
            assert here[case.kinds()[0]] >= 1 and per_game[c0] > 0                          # every chunk carries samples in its first game
    for g in case.planted.get("no_end", []):
        assert last[g] == -1 and per_game[g] == 0
    for g in case.planted.get("end_first", []):
        assert last[g] == 0 and (done[:, g] != 0).sum() == 1
    for g in case.planted.get("end_last", []):
        assert last[g] == T - 1 and (done[:, g] != 0).sum() == 1
    for g in case.planted.get("end63", []):
        assert last[g] == 63
    for g in case.planted.get("end64", []):
        assert last[g] == 64
    for g in case.planted.get("all_none", []):
        assert last[g] >= 0 and per_game[g] == 0 and (action[:, g] == -1).all()
    for g in case.planted.get("done123", []):
        assert set(done[:, g].tolist()) == {0, 1, 2, 3}
    if T >= 65 and N > 1:
        assert case.planted["end63"] and case.planted["end64"]
    if N > 1024:
        assert any(i % N >= 1024 for i in index) and any(i % N < 1024 for i in index)


def _walk(case):
    """A ring sequence through the model, checked against the ABSOLUTE history: what was handed out, what was dropped."""
    case.build()
    N, T, R = case.N, case.T, case.R
    seen, dropped_steps, pend = set(), set(), case.first_pending()
    spans, mods, results = {g: [] for g in range(N)}, set(), case.expected()
    for w, (index, new, dropped) in enumerate(results):
        s_end = case.steps_played(w)
        mods.add(s_end % R != 0)
        games = [i % N for i in index]
        assert games == sorted(games), (case.id, w)                                         # game by game
        prev = None
        for i in index:
            slot, g = divmod(i, N)
            s = s_end - 1 - ((s_end - 1 - slot) % R)                                        # the newest absolute step living in that slot
            assert prev is None or prev[0] != g or prev[1] < s, (case.id, w, g, s)          # steps ascending
            prev = (g, s)
            assert (g, s) not in seen, "%s: game %d step %d handed out twice" % (case.id, g, s)
            seen.add((g, s))
            assert case.action[s - case.shift, g] >= 0
        for g in np.flatnonzero(new != pend):
            spans[g].append((int(pend[g]), int(new[g]) - 1, s_end))
        pend = new
    dropped_total = results[-1][2]
    # what should have been handed out: every action-carrying step up to each game's last end -- minus the steps that had left the ring
    want, n_dropped = set(), 0
    for g in range(N):
        ends = np.flatnonzero(case.done[:, g])
        for p0, last, s_end in spans[g]:
            lo = max(0, s_end - R + (1 if s_end % R else 0))
            for s in range(p0, last + 1):
                if s < lo:
                    n_dropped += 1
                elif case.action[s - case.shift, g] >= 0:
                    want.add((g, s))
        covered = sum(last - p0 + 1 for p0, last, _ in spans[g])
        assert covered == (ends[-1] + 1 if len(ends) else 0), (case.id, g)                  # the spans tile 0 .. the last end
        assert int(pend[g]) - case.shift == covered
    assert seen == want and n_dropped == dropped_total
    return spans, mods, results


@pytest.mark.parametrize("case", M.RING_CASES, ids=ids(M.RING_CASES))
def test_ring_sequence_hands_out_every_step_exactly_once(case):
    spans, mods, results = _walk(case)
    N, T, D, R = case.N, case.T, case.D, case.R
    assert case.windows >= 3 * D + 2 and (mods == {True, False} or D == 1)
    assert results[-1][2] > 0 or N < 3 and D > 1                                            # drops occur (a lone game on one slot: below)
    roles = case.roles
    for g in roles["edges"]:
        ends = np.flatnonzero(case.done[:, g])
        assert any(e % T == 0 for e in ends) and any(e % T == T - 1 for e in ends)
        assert len(spans[g]) == case.windows or T == 1                                      # samples in every window
    for g in roles.get("long", []):
        lens = [last - p0 + 1 for p0, last, _ in spans[g]]
        assert {64, 65, 70} <= set(lens), lens                                              # one full ballot, and a second one
        for p0, last, s_end in spans[g]:
            assert last - p0 + 1 not in (64, 65) or p0 >= s_end - R + (1 if s_end % R else 0)     # ... all of it still in the ring
    for g in roles.get("outlive", []):
        assert spans[g] and all(last - p0 + 1 > R for p0, last, _ in spans[g])
    for g in roles.get("never", []):
        assert not spans[g] and not case.done[:, g].any()
    if R > 64:
        assert roles.get("long")
    if N >= 3:
        assert set(roles) >= {"edges", "outlive", "never"}
    assert abs(float((case.action < 0).mean()) - 0.06) < 0.03 or case.action.size < 200
    if N == 1029:
        sampled = {i % N for index, _, _ in results for i in index}
        assert {1024, 1025, 1026, 1027, 1028} <= sampled and min(sampled) < 4               # blocks 256 and 257, and block 0


def test_a_lone_game_on_a_ring_of_one_slot_drops_what_it_cannot_hold():
    case = M.RING_CASES[0]
    spans, mods, results = _walk(case)
    assert (case.N, case.R) == (1, 1) and results[-1][2] > 0 and sum(len(ix) for ix, _, _ in results) > 0


@pytest.mark.parametrize("case", M.SHIFT_CASES, ids=ids(M.SHIFT_CASES))
def test_a_clock_shifted_by_whole_rings_changes_nothing_but_the_clock(case):
    _walk(case)
    plain = M.RingCase(case.N, case.T, case.D, windows=case.windows).build()
    assert np.array_equal(plain.done, case.done) and np.array_equal(plain.action, case.action)
    assert case.shift % case.R == 0 and case.shift > 0
    last = case.steps_played(case.windows - 1)
    assert last % case.T == 0 and last <= M.STEP_LIMIT < last + case.T                     # the largest multiple of T the entry accepts
    for (ia, pa, da), (ib, pb, db) in zip(plain.expected(), case.expected()):
        assert ia == ib and da == db and np.array_equal(pa + case.shift, pb)


# ---------------------------------------------------------------------------------------------------------------- the comparisons object
def test_the_shared_comparisons_object_to_a_perturbed_result():
    want = [5, 9, 12]
    M.compare_index("x", np.array([5, 9, 12, 77]), 3, want, 4)
    with pytest.raises(AssertionError, match="game 2"):
        M.compare_index("x", np.array([5, 10, 12]), 3, want, 4)
    with pytest.raises(AssertionError, match="count"):
        M.compare_index("x", np.array([5, 9, 12]), 2, want, 4)
    a = M.nan_pattern((3, 4))
    M.compare_returns("x", a, a.copy())
    b = a.copy()
    b.view(np.int32)[2, 1] ^= 1                                  # another NaN: equal as floats never, equal as bits only when untouched
    with pytest.raises(AssertionError, match="step/slot 2 game 1"):
        M.compare_returns("x", b, a)
    with pytest.raises(AssertionError, match="game 3"):
        M.compare_pending("x", [0, 0, 0, 8], [0, 0, 0, 9])
    M.compare_countf("x", np.array([3, np.float32(1) / np.float32(3)], np.float32), 3)
    M.compare_countf("x", np.array([0, 1], np.float32), 0)
    with pytest.raises(AssertionError):
        M.compare_countf("x", np.array([3, 0.3333], np.float32), 3)
    M.compare_guard("x", np.full(64, M.SENTINEL, np.int32), "index guard")
    with pytest.raises(AssertionError, match=r"\+7"):
        g = np.full(64, M.SENTINEL, np.int32)
        g[7] = 0
        M.compare_guard("x", g, "index guard")
