"""The policy head's draws pinned to an independent host reference (tests/policy_draw_ref.py): Philox4x32-10 against the Random123 known
answers, and azul_policy_head_kernel / azul_policy_head_n_kernel<180 | 240 | 300> (csrc/azul_policy.hpp: policy_head_rows, compiled
UNMODIFIED under the lane emulation of tests/hostcheck) against the float64 masked softmax and np.random.choice's inverse CDF, on the rows
where heads go wrong and at the extreme uniforms u = 0 and u = 1 - k 2^-24.

Tolerances (policy_draw_ref.draw_delta / logp_tol): u = 2^-24 is the f32 unit round-off.  A weight e_j = __expf(z_j) is off by a relative
2|z_j| u + 2u (v_exp_f32 evaluates 2^(z log2 e): rounding the product moves the exponent by |z| log2(e) u, a relative |z| u, the constant
log2 e as much again, plus 1 ulp of v_exp_f32); every partial sum of the inverse CDF, the row_shr scan and the butterfly sum S is a sum of
non-negative terms with at most k = (legal actions of the fullest lane) + 4 DPP steps inexact additions (adding an illegal action's 0 is
exact), so each carries k u; the lane prefix's subtraction and the target u S round once each.  The crossing test therefore sits within
delta = (1 + 2^-4) u (sum_j (2|z_j| + 2) w_j / S + 2k + 2)  of the exact CDF: a draw closer than delta to a boundary is excused, and must
still pick one of the two actions beside it.  logp and the entropy term add __logf's error (2 ulp of log S, 2^-21 absolute near S = 1) and
the (NPL + 4) u sum |z| of zsum.  On the existing tests' regime (randn x 3 logits, 30 % legal) these bounds are tighter than their
atol 2e-5, rtol 1e-5 (asserted below)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import policy_draw_ref as R
from tests.hostcheck import hostcheck


# (seed, counter, id_base): nonzero high key words (the opponent key sample_seed ^ 0x4F50504F4E454E54), counters across the 2^32 carry and
# the net-opponent paths' 2^64 - 1, a nonzero id_base
KEYS = [(0x5EED, 0, 0), (0x5EED ^ 0x4F50504F4E454E54, 2 ** 32 - 1, 4096), (0x0123456789ABCDEF, 2 ** 32 + 1, 0xFFFFFF00),
        ((0x5EED ^ 0x4F50504F4E454E54) + 1, 2 ** 64 - 1, 77)]

# ids whose uniform at seed 0x5EED (the default sample_seed), counter 7 is 0 or 1 - k 2^-24 (found by a scan of 2^25 ids; re-asserted below)
EXTREME_IDS = {0: [174611, 2193503], 1: [2703464, 12026210], 2: [18417450], 3: [9156337], 4: [5654025]}


def _lib():
    L = C.CDLL(hostcheck.build("libsimt_learner.so"))
    L.sl_head.restype = C.c_longlong
    L.sl_head.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sl_head_n.restype = C.c_longlong
    L.sl_head_n.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sl_buffer_oob.restype = C.c_ulonglong
    return L


@pytest.fixture(scope="module")
def L():
    return _lib()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def emulated_head(L, entry, logits, mask, seed, counter, id_base):
    """azul_policy_head (entry "head", 180 actions) or azul_policy_head_n (entry "head_n") under emulation."""
    logits, mask = np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(mask, np.uint8)
    n, na = logits.shape
    a, lp, en = np.full(n, -9, np.int32), np.full(n, 9, np.float32), np.full(n, 9, np.float32)
    oob0 = L.sl_buffer_oob()
    if entry == "head":
        assert na == 180
        ops = L.sl_head(n, _p(logits), _p(mask), seed, counter, id_base, _p(a), _p(lp), _p(en))
    else:
        ops = L.sl_head_n(n, na, _p(logits), _p(mask), seed, counter, id_base, _p(a), _p(lp), _p(en))
    assert ops > 0 and L.sl_buffer_oob() == oob0
    return a, lp, en


def test_philox_known_answers():
    """Random123's known-answer vectors for Philox4x32-10 (ctr / key -> out)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, out in kat:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == out
    # vectorised: the same answers broadcast over arrays, and the kernels' word layout (counter lo / hi, id, "AZUL"; seed lo / hi)
    words = R.philox4x32_10((np.array([0, 0xFFFFFFFF], np.uint64), np.array([0, 0xFFFFFFFF], np.uint64), np.array([0, 0xFFFFFFFF], np.uint64),
                             np.array([0, 0xFFFFFFFF], np.uint64)), (np.array([0, 0xFFFFFFFF], np.uint64), np.array([0, 0xFFFFFFFF], np.uint64)))
    assert [int(w) for w in words[0]] == [0x6627E8D5, 0x408F276D]
    seed, counter, game = 0x299F31D0A4093822, 0x85A308D3243F6A88, 0x13198A2E
    assert int(R.philox4x32_10((0x243F6A88, 0x85A308D3, game, R.AZUL_WORD), (0xA4093822, 0x299F31D0))[0]) == int(R.policy_word(seed, counter, game))


def test_the_extreme_uniform_ids_are_what_they_claim():
    for k, ids in EXTREME_IDS.items():
        u = R.policy_uniform(0x5EED, 7, np.array(ids))
        assert (u == (0.0 if k == 0 else 1.0 - k * 2.0 ** -24)).all(), (k, ids, u)


@pytest.mark.parametrize("entry,na", [("head", 180), ("head_n", 180), ("head_n", 240), ("head_n", 300)])
def test_emulated_head_matches_the_float64_reference(L, entry, na):
    """Every input family at every key: the action equals the float64 inverse CDF outside delta of a boundary, logp / entropy within the
    per-row bounds; argmax mode (seed AZUL_POLICY_ARGMAX) equals the first maximum on every row."""
    compared = excused = 0
    for ki, (seed, counter, id_base) in enumerate(KEYS):
        for name, (lg, mk) in R.input_families(na, 256, 100 * na + ki).items():
            ref = R.head(lg, mk, seed, counter, id_base)
            a, lp, en = emulated_head(L, entry, lg, mk, seed, counter, id_base)
            c, e = R.compare(ref, a, lp, en)
            compared, excused = compared + c, excused + e
            if name == "peaked":                              # the bounds are no looser than the existing atol 2e-5, rtol 1e-5 here
                lpt, ent_t = R.logp_tol(ref["z"], ref["w"], ref["mask"], ref["npl"])
                ok = ref["mask"].any(axis=1)
                assert (lpt[ok] <= 2e-5 + 1e-5 * np.abs(ref["logp_all"][ok, np.maximum(a[ok], 0)])).all()
                assert (ent_t[ok] <= 2e-5 + 1e-5 * np.abs(ref["entropy"][ok])).all()
            if name == "edges":                               # a single legal action: always that one, log p = 0
                assert np.array_equal(a, mk.argmax(axis=1)) and (lp == 0).all() and (en == 0).all()
        lg, mk = R.input_families(na, 64, 7 + ki)["peaked"]
        ref = R.head(lg, mk, R.ARGMAX, counter, id_base)
        a, lp, en = emulated_head(L, entry, lg, mk, R.ARGMAX, counter, id_base)
        assert R.compare(ref, a, lp, en) == (int(mk.any(axis=1).sum()), 0)
    assert compared >= 4000 and excused <= compared // 1000, (compared, excused)


@pytest.mark.parametrize("entry,na", [("head", 180), ("head_n", 240), ("head_n", 300)])
def test_equal_logits_pin_the_uniform(L, entry, na):
    """All actions legal with equal logits: every weight is 1 and every sum exact, so the draw is floor(na u) of the f32 target u * na --
    7 to 8 bits of each row's uniform, pinned row by row (and equal to the float64 floor(na u) except where u * na rounds up to an integer)."""
    n = 1024
    lg, mk = np.full((n, na), 0.375, np.float32), np.ones((n, na), np.uint8)
    for seed, counter, id_base in KEYS:
        u = R.policy_uniform(seed, counter, (np.arange(n) + id_base) & 0xFFFFFFFF)
        a, lp, en = emulated_head(L, entry, lg, mk, seed, counter, id_base)
        want32 = np.floor(np.float32(u.astype(np.float32) * np.float32(na)).astype(np.float64)).astype(np.int64)
        assert np.array_equal(a, want32)
        assert (np.floor(u * na).astype(np.int64) != want32).sum() <= n // 1000
        assert np.allclose(lp, -np.log(na), atol=2e-6) and np.allclose(en, np.log(na), atol=2e-6)


def _zero_weight_case(L, entry, na, k, where, rows):
    lg, mk, zero, other = R.zero_weight_rows(na, rows, 1000 * na + 10 * k + (where == "first"), where)
    got = np.zeros(rows, np.int64)
    ids = EXTREME_IDS[k]
    lps = np.zeros(rows)
    for r in range(rows):                                       # the id sets u: one row per launch, id_base = the found id
        a, lp, en = emulated_head(L, entry, lg[r:r + 1], mk[r:r + 1], 0x5EED, 7, ids[r % len(ids)])
        got[r], lps[r] = a[0], lp[0]
    return got, zero, other, lps


@pytest.mark.parametrize("entry,na", [("head", 180), ("head_n", 180), ("head_n", 240), ("head_n", 300)])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_u_just_below_one_never_draws_a_zero_weight_action(L, entry, na, k):
    """u = 1 - k 2^-24 with the last legal action at zero f32 weight: the kernel's target u S can land at or past its last cumulative sum
    (the sums are the same numbers added in another order), and its round-off fallback must then take the last legal action of POSITIVE
    weight -- what np.random.choice on the f32 softmax and the float64 reference both draw -- never the zero-weight one."""
    got, zero, other, lps = _zero_weight_case(L, entry, na, k, "last", 256)
    assert not (got == zero).any(), "rows %s drew an action of probability 0" % np.flatnonzero(got == zero)[:8].tolist()
    assert np.array_equal(got, other)
    assert (lps > -30).all()


@pytest.mark.parametrize("entry,na", [("head", 180), ("head_n", 240), ("head_n", 300)])
def test_u_zero_skips_a_leading_zero_weight_action(L, entry, na):
    """u = 0 with the first legal action at zero f32 weight: target 0 is not below its cumulative sum 0, so the draw is the first legal
    action of positive weight (np.random.choice's searchsorted(0, side="right") on the f32 softmax)."""
    got, zero, other, lps = _zero_weight_case(L, entry, na, 0, "first", 128)
    assert not (got == zero).any() and np.array_equal(got, other)


def test_a_wrong_stream_is_told_apart(L):
    """Negative control: the same comparison against a reference fed a subtly wrong uniform (game id + 1; counter words swapped) fails on
    most rows -- the comparison can tell the kernel's stream from a near miss."""
    na, n = 240, 512
    lg, mk = R.input_families(na, n, 3)["flat"]
    seed, counter, id_base = 0x5EED ^ 0x4F50504F4E454E54, 2 ** 32 + 5, 4096
    a, lp, en = emulated_head(L, "head_n", lg, mk, seed, counter, id_base)
    R.compare(R.head(lg, mk, seed, counter, id_base), a, lp, en)
    swapped = ((counter & 0xFFFFFFFF) << 32) | (counter >> 32)
    for wrong in (R.head(lg, mk, seed, counter, id_base + 1), R.head(lg, mk, seed, swapped, id_base)):
        ok = mk.any(axis=1)
        assert (a[ok] != wrong["action"][ok]).mean() > 0.9
        with pytest.raises(AssertionError):
            R.compare(wrong, a, lp, en)
