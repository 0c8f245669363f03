"""The PPO instantiations (OBJ = 1) of the gradient kernels on the CPU: csrc/azul_learner.hpp compiles unmodified under the lockstep
64-lane emulation (tests/hostcheck/simt_ppo.cpp), and azul_a2c_grad_kernel<1> (reference shape) and azul_a2c_grad_n_kernel<260, 300, 1>
(p4_d9) give, per element, the float64 restatement of tests/ppo_grad_ref.py within K_case 2^-24 N on n = M + 1 (one and two parts),
clip-all-four, one-legal-random and index-perm-count=M-1; the recomputed logp[a] lands at the sample's launch position only, and the
emulation's out-of-range buffer counter does not move.  Measured: 5 s (reference shape) + 6 s (p4_d9) for five launches each,
the build of the shim included."""
import ctypes as C

import numpy as np
import pytest

from tests import ppo_grad_ref as R
from tests.hostcheck import hostcheck
from tests.hostcheck.hostcheck import ptr

SENTINEL = np.float32(777.0)
_L = None


def _lib():
    global _L
    if _L is None:
        L = C.CDLL(hostcheck.build("libsimt_ppo.so"))
        L.sp_gradients.restype = C.c_longlong
        L.sp_gradients.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6 + [C.c_float] * 3 + [C.c_void_p, C.c_float] + [C.c_void_p] * 12
        L.sp_buffer_oob.restype = C.c_ulonglong
        _L = L
    return _L


def _run(L, shape, c):
    IN, A = shape
    total = R.flat_size(IN, A) + 4
    assert L.sp_flat_size(IN, A) == total - 4
    w = c["w"]
    w2a = np.ascontiguousarray(w["w2a_t"].T)
    M = R.samples_per_pass(IN, A)
    parts = min(c["parts"], (c["n"] + M - 1) // M)             # (the host entry launches min(tiles, workspace_parts) parts)
    partial, grad = np.zeros((parts, total), np.float32), np.full(total, np.nan, np.float32)
    logp = np.full(c["n"], SENTINEL, np.float32)
    n_dev = inv_dev = None
    inv_host = c["inv_n"] if c["inv_n"] is not None else 1.0 / max(c["n"], 1)
    if c["index"] is not None:
        assert int(c["index"].min()) >= 0 and int(c["index"].max()) < c["obs"].shape[0]
        n_dev, inv_dev, inv_host = np.array([c["count"]], np.int32), np.array([1.0 / max(c["count"], 1)], np.float32), 1.0
    oob0 = L.sp_buffer_oob()
    ops = L.sp_gradients(IN, A, c["n"], parts, ptr(c["obs"]), ptr(c["mask"]), ptr(c["action"]), ptr(c["q"]), ptr(c["old_logp"]), ptr(c["adv"]),
                         c["eps"], c["cv"], c["ce"], ptr(c["index"]), inv_host, ptr(n_dev), ptr(inv_dev), ptr(w["w1t"]), ptr(w["b1"]), ptr(w["w2c"]),
                         ptr(w["b2c"]), ptr(w["w2a_t"]), ptr(w["b2a"]), ptr(w2a), ptr(partial), ptr(grad), ptr(logp))
    assert ops > 0 and L.sp_buffer_oob() == oob0
    return grad, logp


@pytest.mark.parametrize("shape_name", ["ref", "p4_d9"])
def test_ppo_head_under_emulation_on_the_case_table(shape_name):
    L = _lib()
    shape = R.SHAPES[shape_name]
    size = R.flat_size(*shape)
    for name in R.EMULATION_CASES:
        c = R.build(shape_name, name)
        ref = R.reference(shape, c["w"], *R.call_args(c))
        K = R.k_case(R.yardstick(shape, c))
        assert K * R.ULP <= 1e-3
        got, logp = _run(L, shape, c)
        worst, zeros_ok = R.normalised_error(got[:size], ref["flat"], ref["N"])
        print("NORMALISED %s %s worst %.2f K_case %.1f" % (shape_name, name, worst, K))
        assert np.isfinite(got).all() and zeros_ok, name
        assert worst <= K, (name, worst, K)
        assert got[R.offsets(*shape)["pad"][0]] == 0.0 and got[size + 3] == ref["sums"][3], name
        tol = 2e-5 * float(np.abs(ref["sums"][:3]).max()) + 1e-6
        assert (np.abs(got[size:size + 3] - ref["sums"][:3]) <= tol).all(), (name, got[size:size + 3], ref["sums"])
        have = np.zeros(c["n"], bool)
        have[:len(ref["logp"])] = np.isfinite(ref["logp"])
        assert (logp[~have] == SENTINEL).all(), name           # positions without a sample are not written
        assert np.abs(logp[have] - ref["logp"][np.isfinite(ref["logp"])]).max() <= 2e-5, name
