"""azul_x_score_moves_kernel on CPU: csrc/azul_x_kernels.hpp (on azx::score_moves_body_x of azul_rules_x.hpp, UNMODIFIED) compiled by g++ and
run under the lockstep 64-lane emulation (tests/hostcheck/simt_mp_score_moves.cpp) for the five instantiations (P, D) = (2, 5), (3, 5),
(3, 7), (4, 5), (4, 9) on the shared states of tests/mp_score_moves_model.py (three oracle streams, arbitrary in-domain records, a game
before its first round), against that model: the whole [n][num_actions] table and `best` for every perspective in batches of 1, 2, 3 and
33 records (odd counts leave the last wave one game; neighbours of a wave hold different masks), an `active` mask with holes (inactive rows
keep a canary), each output optional, and records, MT19937 words and indices and counters byte-identical before and after.  The `-m gpu`
tests repeat it on the real kernel (tests/test_gpu_mp_score_moves.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import mp_score_moves_model as mm
from tests.hostcheck import hostcheck as hc

CANARY = 0x5EED5EED
SIZES = (1, 2, 3, 33)
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(hc.build("libsimt_mp_score_moves.so"))
        _lib.shx_score_moves.restype = C.c_longlong
        _lib.shx_score_moves.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p] * 3
    return _lib


def run(shape, recs, persp, active=None, want_scores=True, want_best=True):
    P, ext, pool, first = shape
    n, NA = len(recs), mm.num_actions(shape)
    rs = np.random.RandomState(n + 31 * P)
    book = {"state": np.ascontiguousarray(recs, np.uint8).copy(), "mt": rs.randint(0, 2 ** 32, size=(n, 624), dtype=np.uint64).astype(np.uint32),
            "pos": rs.randint(0, 625, size=n).astype(np.uint32), "episodes": rs.randint(0, 99, size=n).astype(np.uint64),
            "stuck": rs.randint(0, 99, size=n).astype(np.uint32), "stat_sum": rs.rand(n, 10)}
    keep = {k: v.copy() for k, v in book.items()}
    scores = np.full((n, NA), CANARY, np.int32) if want_scores else None
    best = np.full(n, CANARY, np.int32) if want_best else None
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    xpool = 2 if ext & oz.EXT_FINITE_BAG else (1 if pool == oz.POOL_LID else 0)
    ops = lib().shx_score_moves(n, P, mm.displays(shape), hc.ptr(book["state"]), hc.ptr(book["mt"]), hc.ptr(book["pos"]), hc.ptr(book["episodes"]),
                                hc.ptr(book["stuck"]), hc.ptr(book["stat_sum"]), first, xpool, int(bool(ext & oz.EXT_END_BONUS)),
                                int(bool(ext & oz.EXT_SHORT_DEAL)), persp, hc.ptr(act), hc.ptr(scores), hc.ptr(best))
    assert ops >= 0                                                      # (0: every game of the launch was inactive)
    for k in book:
        assert book[k].tobytes() == keep[k].tobytes(), "the kernel wrote to the batch's %s" % k
    return scores, best


def windows(n_states):
    """(start, size) of consecutive windows over the shared states, sizes 1, 2, 3, 33 in turn."""
    i, k, out = 0, 0, []
    while i < n_states:
        n = min(SIZES[k % 4], n_states - i)
        out.append((i, n))
        i, k = i + n, k + 1
    return out


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=[mm.shape_id(s) for s in mm.SHAPES])
def test_table_and_best_equal_the_model_for_every_perspective(i):
    shape = mm.SHAPES[i]
    recs = mm.states(i)
    wins = windows(len(recs))
    assert {n for _, n in wins} >= set(SIZES)
    for persp in mm.perspectives(shape):
        tabs, best = mm.tables(i, persp)
        for lo, n in wins:
            s, b = run(shape, recs[lo:lo + n], persp)
            assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]), (persp, lo, n)
            assert np.array_equal(b, best[lo:lo + n]), (persp, lo, n)


def test_a_nine_display_state_whose_best_move_is_256_or_above():
    i = len(mm.SHAPES) - 1
    shape = mm.SHAPES[i]
    assert mm.num_actions(shape) == 300
    tabs, best = mm.tables(i, mm.PERSP_MOVER)
    high = np.flatnonzero(best >= 256)
    assert len(high) >= 3
    for g in high[:6]:
        s, b = run(shape, mm.states(i)[g:g + 1], mm.PERSP_MOVER)
        assert int(b[0]) == int(best[g]) >= 256 and np.array_equal(s[0].astype(np.int64), tabs[g])


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=[mm.shape_id(s) for s in mm.SHAPES])
@pytest.mark.parametrize("n,holes", [(1, [0]), (2, [1]), (3, [0, 2]), (33, [1, 2, 6, 32]), (33, [0] + list(range(3, 31)))])
def test_inactive_rows_keep_the_canary_and_each_output_is_optional(i, n, holes):
    shape = mm.SHAPES[i]
    recs = mm.states(i)[40:40 + n]
    tabs, best = mm.tables(i, mm.PERSP_MOVER)
    tabs, best = tabs[40:40 + n], best[40:40 + n]
    active = np.ones(n, np.uint8)
    active[holes] = 0
    on = active != 0
    for want_scores, want_best in ((True, True), (True, False), (False, True)):
        s, b = run(shape, recs, mm.PERSP_MOVER, active, want_scores, want_best)
        if want_scores:
            assert np.array_equal(s[on].astype(np.int64), tabs[on]) and (s[~on] == CANARY).all()
        if want_best:
            assert np.array_equal(b[on], best[on]) and (b[~on] == CANARY).all()
