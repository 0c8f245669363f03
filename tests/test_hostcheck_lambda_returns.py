"""azul_lambda_returns_ring_kernel (csrc/azul_selfplay_kernels.hpp), UNMODIFIED, under the lockstep lane emulation
(tests/hostcheck/simt_lambda_returns.cpp) on the case table of tests/lambda_returns_cases.py: bit-equal to the host model of the header's
contract, the guard rows behind the ring and the slots outside the span untouched, the inputs unchanged.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import lambda_returns_cases as M
from tests import training_ring_cases as RC
from tests.hostcheck import hostcheck
from tests.hostcheck.hostcheck import ptr

_lib = None


def load():
    global _lib
    if _lib is None:
        L = C.CDLL(hostcheck.build(os.environ.get("AZUL_SIMT_LAMBDA_RETURNS_LIB", "libsimt_lambda_returns.so")))
        L.slr_lambda_returns_ring.restype = C.c_longlong
        L.slr_lambda_returns_ring.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_int, C.c_longlong, C.c_int, C.c_int]
        L.slr_buffer_oob.restype = C.c_ulonglong
        _lib = L
    return _lib


def _run(case, built, lam=None, use_tail=True):
    reward, done, value, tail, ret_in = built
    keep = [a.copy() for a in (reward, done, value)] + [None if tail is None else tail.copy()]
    out = ret_in.copy()
    t = tail if use_tail else None
    assert load().slr_lambda_returns_ring(ptr(reward), ptr(done), ptr(value), ptr(t), ptr(out), np.float32(case.gamma),
                                          np.float32(case.lam if lam is None else lam), case.ring, case.played, case.span, case.N) > 0
    assert load().slr_buffer_oob() == 0
    for a, b in zip((reward, done, value, tail), keep):
        assert b is None or np.array_equal(a, b), case.id                # the inputs are read, never written
    return out


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_lambda_returns_ring_kernel_under_emulation_on_the_case_table(case):
    built = case.build()
    reward, done, value, tail, ret_in = built
    want = M.lambda_returns_ring(reward, done, value, tail, ret_in, case.gamma, case.lam, case.ring, case.played, case.span)
    got = _run(case, built)
    M.compare_returns(case.id, got, want)                                # the ring, the slots outside the span and the guard rows at once
    untouched = np.ones(len(got), bool)
    untouched[case.slots()] = False
    M.compare_returns(case.id, got[untouched], ret_in[untouched], "the rows outside the span and behind the ring")
    assert np.isfinite(got[~untouched]).all()


@pytest.mark.parametrize("case", [c for c in M.CASES if c.N > 1], ids=[c.id for c in M.CASES if c.N > 1])
def test_lambda_one_without_a_tail_is_the_monte_carlo_scan(case):
    """The contract's first property on the kernel itself: lambda == 1, nothing flowing in, finite values -> azul_discounted_returns_ring's
    bits (its model: tests/training_ring_cases.returns_ring)."""
    built = case.build()
    reward, done, value, tail, ret_in = built
    got = _run(case, built, lam=1.0, use_tail=False)
    M.compare_returns(case.id, got, RC.returns_ring(reward, done, ret_in, case.gamma, case.ring, case.played, case.span))
