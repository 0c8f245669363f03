"""The host model of azul_lambda_returns_ring (tests/lambda_returns_cases.py) checked against itself: the array form equals the literal
per-game loop, float32 stays within the running bound of the fp64 twin, lambda = 1 is the Monte-Carlo scan of
tests/training_ring_cases.py bit for bit, lambda = 0 is r + gamma * V_next, and the case table holds every class the kernel's tests rely
on.  No GPU, no library."""
import numpy as np
import pytest

from tests import lambda_returns_cases as M
from tests import training_ring_cases as RC

ids = [c.id for c in M.CASES]


def _model(case, built, lam=None, tail="case"):
    reward, done, value, t, ret_in = built
    return M.lambda_returns_ring(reward, done, value, t if tail == "case" else tail, ret_in, case.gamma, case.lam if lam is None else lam,
                                 case.ring, case.played, case.span)


def test_the_table_holds_every_class():
    C = M.CASES
    assert {c.N for c in C} >= {1, 63, 64, 65, 257}
    assert {c.span for c in C} >= {1, 15, 16, 17, 33}
    assert {c.lam for c in C} >= {0.0, 0.5, 0.95, 1.0} and {c.gamma for c in C} >= {0.0, 0.99, 1.0}
    assert {c.tail for c in C} == {True, False}
    assert any(c.ring == c.span and c.ring > 1 for c in C) and any(c.ring > c.span for c in C)
    assert any(c.ring > c.span and c.where == "middle" and c.wraps for c in C)
    assert any(c.ring == c.span and c.where == "middle" and c.wraps for c in C)
    assert {c.where for c in C if c.ring > 1} == {"first", "middle", "last"}
    assert any(c.played % c.ring for c in C) and any(c.played > 2 ** 31 for c in C)
    assert any(c.lam == 1.0 and not c.tail for c in C) and any(c.lam == 1.0 and c.tail for c in C)
    kinds = set()
    for c in C:
        reward, done, value, tail, ret_in = c.build()
        kinds |= set(c.planted)
        assert ret_in.shape == (c.ring + M.GUARD_ROWS, c.N) and np.isnan(ret_in).all()
        assert reward.min() < 0 and sorted(c.slots()) == sorted(set(c.slots())) and len(c.slots()) == c.span
        for k, games in c.planted.items():
            for g in games:
                d = done[:, g]
                want = {"end_newest": [c.newest], "end_all": list(range(c.ring)), "no_end": [], "end_slot0": [0], "end_last_slot": [c.ring - 1],
                        "big_value": []}[k]
                assert np.flatnonzero(d).tolist() == want, (c.id, k, g)
                if k == "big_value":
                    assert np.abs(value[:, g]).max() == 1e4 and np.abs(value[:, g]).max() <= 1e4
    assert kinds == set(M.KINDS)
    # somewhere an end really sits inside the span at slot 0 and at the last slot
    assert any(0 in c.slots() and "end_slot0" in c.plan() for c in C) and any(c.ring - 1 in c.slots() and "end_last_slot" in c.plan() for c in C)


@pytest.mark.parametrize("case", M.CASES, ids=ids)
def test_column_twin_equals_the_array_form(case):
    built = case.build()
    reward, done, value, tail, ret_in = built
    got = _model(case, built)
    games = sorted({0, case.N - 1, case.N // 2} | {g for gs in case.planted.values() for g in gs})
    for g in games:
        col = M.lambda_returns_column(reward[:, g], done[:, g], value[:, g], None if tail is None else tail[g], ret_in[:, g], case.gamma,
                                      case.lam, case.ring, case.played, case.span)
        M.compare_returns("%s game %d" % (case.id, g), got[:, g], col)


@pytest.mark.parametrize("case", M.CASES, ids=ids)
def test_guard_rows_and_slots_outside_the_span_keep_their_bits(case):
    built = case.build()
    got, ret_in = _model(case, built), built[4]
    keep = np.ones(case.ring + M.GUARD_ROWS, bool)
    keep[case.slots()] = False
    M.compare_returns(case.id, got[keep], ret_in[keep], "the untouched rows")
    assert np.isfinite(got[~keep]).all()


@pytest.mark.parametrize("case", M.CASES, ids=ids)
def test_float32_stays_within_the_fp64_bound(case):
    built = case.build()
    reward, done, value, tail, _ = built
    got = _model(case, built)[:case.ring].astype(np.float64)
    q64, bound = M.lambda_returns_f64(reward, done, value, tail, case.gamma, case.lam, case.ring, case.played, case.span)
    s = case.slots()
    err = np.abs(got[s] - q64[s])
    assert (err <= bound[s]).all(), (case.id, float((err - bound[s]).max()))
    # (the bound itself says something: |q| <= (span + 1) * top, top the largest magnitude that entered, and a few roundings of it per step)
    top = max(np.abs(value).max(), np.abs(reward).max(), 0.0 if tail is None else np.abs(tail).max())
    assert (bound[s] <= 8 * M.U24 * case.span * (case.span + 1) * top).all()


@pytest.mark.parametrize("case", M.CASES, ids=ids)
def test_lambda_one_is_the_monte_carlo_scan_bit_for_bit(case):
    built = case.build()
    reward, done, value, tail, ret_in = built
    got = _model(case, built, lam=1.0, tail=None)
    want = RC.returns_ring(reward, done, ret_in, case.gamma, case.ring, case.played, case.span)
    M.compare_returns(case.id, got, want)


@pytest.mark.parametrize("case", M.CASES, ids=ids)
def test_lambda_zero_is_the_one_step_target(case):
    built = case.build()
    reward, done, value, tail, ret_in = built
    got = _model(case, built, lam=0.0)
    g32 = np.float32(case.gamma)
    for i, slot in enumerate(case.slots()):
        v_next = (np.zeros(case.N, np.float32) if tail is None else tail) if i == 0 else value[case.slots()[i - 1]]
        r = reward[slot].astype(np.float32)
        want = np.where(done[slot] != 0, r, np.add(r, np.multiply(g32, v_next, dtype=np.float32), dtype=np.float32))
        M.compare_returns("%s slot %d" % (case.id, slot), got[slot], want)
