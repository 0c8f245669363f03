"""azul_score_moves_kernel on CPU: csrc/azul_selfplay_kernels.hpp (on azul_ops2.hpp -> azul_env2.hpp -> azul_selfplay2.hpp, all UNMODIFIED) compiled by g++ and
run under the lockstep 64-lane emulation (tests/hostcheck/simt_score_moves.cpp) on the 360 states of three oracle streams, against the
host model (tests/score_moves_model.py): the whole [n][180] table and `best` in batches of 1, 2, 3 and 7 records (odd counts leave the
last wave one game), both pools, the three perspectives, an `active` mask with holes (inactive rows keep a canary), record bytes unchanged.
The `-m gpu` tests repeat it on the real kernel (tests/test_gpu_score_moves.py)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import score_moves_model as sm
from tests.hostcheck import hostcheck as hc

CANARY = 0x5EED5EED
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(hc.build("libsimt_score_moves.so"))
        _lib.shs_score_moves.restype = C.c_int
        _lib.shs_score_moves.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
    return _lib


def run(recs, pool, persp, active=None, want_scores=True, want_best=True):
    n = len(recs)
    buf = np.ascontiguousarray(recs, np.uint8).copy()
    keep = buf.copy()
    scores = np.full((n, 180), CANARY, np.int32) if want_scores else None
    best = np.full(n, CANARY, np.int32) if want_best else None
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    assert lib().shs_score_moves(n, hc.ptr(buf), pool, persp, hc.ptr(act), hc.ptr(scores), hc.ptr(best)) == 0
    assert np.array_equal(buf, keep), "the kernel wrote to a record"
    return scores, best


@pytest.mark.parametrize("persp", [0, 1, sm.PERSP_CURRENT])
@pytest.mark.parametrize("pool", [oz.POOL_LID, oz.POOL_RANDOM])
def test_table_and_best_equal_the_model_on_every_stream_state(pool, persp):
    recs = sm.stream_states()[0]
    tabs, best = sm.stream_tables(persp)
    i = 0
    sizes = [1, 2, 3, 7]
    k = 0
    while i < len(recs):
        n = min(sizes[k % 4], len(recs) - i)
        k += 1
        s, b = run(recs[i:i + n], pool, persp)
        assert np.array_equal(s.astype(np.int64), tabs[i:i + n]), (i, n)
        assert np.array_equal(b, best[i:i + n]), (i, n)
        i += n
    assert k >= 4


@pytest.mark.parametrize("n,holes", [(1, [0]), (2, [1]), (3, [0, 2]), (7, [1, 2, 6]), (7, [0, 3, 4, 5])])
def test_inactive_rows_keep_the_canary_and_each_output_is_optional(n, holes):
    recs = sm.stream_states()[0][40:40 + n]
    tabs, best = sm.stream_tables(sm.PERSP_CURRENT)
    tabs, best = tabs[40:40 + n], best[40:40 + n]
    active = np.ones(n, np.uint8)
    active[holes] = 0
    on = active != 0
    for want_scores, want_best in ((True, True), (True, False), (False, True)):
        s, b = run(recs, oz.POOL_LID, sm.PERSP_CURRENT, active, want_scores, want_best)
        if want_scores:
            assert np.array_equal(s[on].astype(np.int64), tabs[on]) and (s[~on] == CANARY).all()
        if want_best:
            assert np.array_equal(b[on], best[on]) and (b[~on] == CANARY).all()
