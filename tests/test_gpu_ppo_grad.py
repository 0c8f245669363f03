"""GPU: azul_ppo_gradients (the OBJ = 1 instantiations of the five gradient kernels of csrc/azul_learner.hpp) through the C ABI on the
case table of tests/ppo_grad_ref.py: every flat element against the float64 restatement within K_case 2^-24 N (K_case from the
case's f32 yardstick, measured on the CPU), elements with N == 0 exactly 0.0, the pad float, the exact count, the three sums and the
recomputed logp[a] within 2e-5, bit-identical repeats, and content of rows without a sample that cannot change a bit.  Every index is
checked against the arrays on the host before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ppo_grad_ref as R

pytestmark = pytest.mark.gpu

PARAMS = R.all_params()
SENTINEL = np.float32(777.0)
_cache = {}


def _buffers(shape_name):
    if shape_name not in _cache:
        _cache.clear()
        total = R.flat_size(*R.SHAPES[shape_name]) + 4
        _cache[shape_name] = (torch.empty(3 * total, device="cuda"), total)
    return _cache[shape_name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Launcher:
    def __init__(self, shape_name, c):
        from azul_deep_reinforcement_learning_amd import _lib as L
        self.L, self.c = L, c
        self.IN, self.A = R.SHAPES[shape_name]
        self.ws, self.total = _buffers(shape_name)
        self.w = {k: _dev(v) for k, v in c["w"].items()}
        self.w["w2a"] = _dev(c["w"]["w2a_t"].T)                # actor_linear2.weight as PyTorch stores it
        self.index = None if c["index"] is None else _dev(c["index"])
        if c["index"] is not None:
            self.n_dev = torch.tensor([c["count"]], dtype=torch.int32, device="cuda")
            self.inv_dev = torch.tensor([1.0 / max(c["count"], 1)], dtype=torch.float32, device="cuda")

    def __call__(self, eps=None, **over):
        c, L = dict(self.c, **over), self.L
        rows, n = c["obs"].shape[0], c["n"]
        # nothing may reach out of range: shapes, types and every index are checked here, on the host
        assert c["obs"].shape == (rows, self.IN) and c["obs"].dtype == np.float32 and c["mask"].shape == (rows, self.A) and c["mask"].dtype == np.uint8
        assert c["action"].shape == (rows,) and c["action"].dtype == np.int32
        for k in ("q", "old_logp", "adv"):
            assert c[k].shape == (rows,) and c[k].dtype == np.float32, k
        assert 1 <= c["parts"] <= 3 and n >= 0
        if c["index"] is None:
            assert n == rows
        else:
            assert c["index"].dtype == np.int32 and len(c["index"]) == n and 0 <= c["count"] <= n
            assert int(c["index"].min()) >= 0 and int(c["index"].max()) < rows
        d = [_dev(c[k]) for k in ("obs", "mask", "action", "q", "old_logp", "adv")]
        grad = torch.full((self.total,), float("nan"), device="cuda")
        logp = torch.full((max(n, 1),), float(SENTINEL), device="cuda")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        w, f32 = self.w, C.c_float
        counted = c["index"] is not None
        inv_host = 1.0 if counted else (c["inv_n"] if c["inv_n"] is not None else 1.0 / max(n, 1))
        L.check(L.lib.azul_ppo_gradients(*[p(t) for t in d], n, f32(inv_host), f32(c["eps"] if eps is None else eps), f32(c["cv"]), f32(c["ce"]),
                                         p(w["w1t"]), p(w["b1"]), p(w["w2c"]), p(w["b2c"]), p(w["w2a_t"]), p(w["b2a"]), p(w["w2a"]), self.IN, 180,
                                         self.A, p(self.ws), c["parts"], p(grad), p(self.index), p(self.n_dev) if counted else None,
                                         p(self.inv_dev) if counted else None, p(logp), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return grad.cpu().numpy(), logp.cpu().numpy()[:n]


def _compare(tag, got, logp, shape, c, ref, K):
    IN, A = shape
    size = R.flat_size(IN, A)
    assert np.isfinite(got).all(), tag
    worst, zeros_ok = R.normalised_error(got[:size], ref["flat"], ref["N"])
    print("NORMALISED %s worst %.2f K_case %.1f" % (tag, worst, K))
    assert zeros_ok, "%s: an element without a single non-zero term is not exactly 0.0" % tag
    assert worst <= K, "%s: normalised error %.1f above K_case %.1f" % (tag, worst, K)
    assert got[R.offsets(IN, A)["pad"][0]] == 0.0, tag
    assert got[size + 3] == ref["sums"][3], (tag, got[size + 3], ref["sums"][3])
    tol = 2e-5 * float(np.abs(ref["sums"][:3]).max()) + 1e-6
    assert (np.abs(got[size:size + 3] - ref["sums"][:3]) <= tol).all(), (tag, got[size:size + 3], ref["sums"][:3])
    have = np.zeros(c["n"], bool)
    have[:len(ref["logp"])] = np.isfinite(ref["logp"])
    assert (logp[~have] == SENTINEL).all(), "%s: a position without a sample was written" % tag
    if have.any():
        err = float(np.abs(logp[have] - ref["logp"][np.isfinite(ref["logp"])]).max())
        print("LOGP %s worst %.3g" % (tag, err))
        assert err <= 2e-5, (tag, err)


def _other_content(rs, c, dead):
    """Other finite observations, actions, returns, old log-probabilities and advantages in the rows that carry no sample."""
    out = {k: c[k].copy() for k in ("obs", "action", "q", "old_logp", "adv")}
    out["obs"][dead] = rs.randint(0, 9, size=(len(dead), c["obs"].shape[1])).astype(np.float32) - 3.0
    out["action"][dead] = rs.randint(0, c["mask"].shape[1], len(dead)).astype(np.int32)
    out["q"][dead] = (rs.randn(len(dead)) * 50).astype(np.float32)
    out["old_logp"][dead] = (-rs.rand(len(dead)) * 9).astype(np.float32)
    out["adv"][dead] = (rs.randn(len(dead)) * 50).astype(np.float32)
    return out


@pytest.mark.parametrize("shape_name,case_name", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_ppo_gradients_per_element_on_the_case_table(shape_name, case_name):
    shape = IN, A = R.SHAPES[shape_name]
    c = R.build(shape_name, case_name)
    ref = R.reference(shape, c["w"], *R.call_args(c))
    K = R.k_case(R.yardstick(shape, c))
    assert K * R.ULP <= 1e-3
    run = Launcher(shape_name, c)
    got, logp = run()
    tag = "%s %s" % (shape_name, case_name)
    _compare(tag, got, logp, shape, c, ref, K)
    # the same call twice: the same bits
    got2, logp2 = run()
    assert np.array_equal(got, got2) and np.array_equal(logp, logp2)
    # dead content: rows without a legal action, and on the index path every row the first `count` entries do not name
    used, _, _ = R._used(c["mask"], c["index"], c["count"])
    dead = np.setdiff1d(np.arange(c["obs"].shape[0]), used)
    if len(dead):
        got3, logp3 = run(**_other_content(np.random.RandomState(5), c, dead))
        assert np.array_equal(got, got3) and np.array_equal(logp, logp3), "content of rows that carry no sample reached the result"
    if c["meta"].get("adv_zero"):                              # the actor part of rows with Adv == 0.0 is exactly zero (c_e = 0 here)
        assert (got[:R.flat_size(IN, A)][R.actor_elements(IN, A)] == 0.0).all() and got[R.flat_size(IN, A)] == 0.0
    if c["meta"].get("no_value"):                              # c_v = 0: dw2c, db2c and the critic half of dw1t / db1
        assert (got[:R.flat_size(IN, A)][R.critic_elements(IN, A)] == 0.0).all()
    if c["meta"].get("ratio_one"):
        # the first epoch of PPO is the plain policy gradient, at the bit level: with the launch's own logp[a] fed back as old_log_prob the
        # ratio is exactly 1.0, and (c_e = 0) the result equals, bit for bit, a launch in which nothing can ever be clipped
        assert c["ce"] == 0.0
        fed = logp.astype(np.float32).copy()
        assert (fed != SENTINEL).all()
        at_one, logp_b = run(old_logp=fed)
        unclipped, logp_c = run(old_logp=fed, eps=1e30)
        assert np.array_equal(logp_b, logp) and np.array_equal(logp_c, logp)
        assert np.array_equal(at_one, unclipped)
        size = R.flat_size(IN, A)
        adv64 = c["adv"].astype(np.float64)                    # ... and sum L_pi = -sum Adv there
        assert abs(at_one[size] + adv64.sum()) <= 2e-5 * np.abs(adv64).sum() + 1e-6
