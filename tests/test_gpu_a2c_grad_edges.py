"""GPU: the five instantiations of azul_a2c_gradients (csrc/azul_learner.hpp: azul_a2c_grad_kernel for (136, 180, 180),
azul_a2c_grad_n_kernel<IN, A> for the four wide shapes), called through the C ABI so that workspace_parts can be 1, 2, 3 and 256,
on the case table of tests/a2c_grad_ref.py: every flat element against the float64 reference within K_case 2^-24 N (N: the element's
sum of absolute terms; K_case = max(64, 8 x the case's f32 yardstick), measured on the CPU, never on the kernel), elements with
N == 0 exactly 0.0, and the exact properties -- the pad float, the sample count, bit-identical repeats, and content of rows that
carry no sample (no legal action, or past the device count) that cannot change a bit of the result.
Every index is checked against the arrays on the host before a launch: no input can reach out of range."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import a2c_grad_ref as R

pytestmark = pytest.mark.gpu

PARAMS = R.all_params()
_cache = {}


def _buffers(shape_name):
    """Per shape: workspace for 256 parts and the gradient buffer (allocated once)."""
    if shape_name not in _cache:
        _cache.clear()
        total = R.flat_size(*R.SHAPES[shape_name]) + 4
        _cache[shape_name] = (torch.empty(256 * total, device="cuda"), total)
    return _cache[shape_name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Launcher:
    def __init__(self, shape_name, c):
        from azul_deep_reinforcement_learning_amd import _lib as L
        self.L, self.c = L, c
        self.IN, self.A = R.SHAPES[shape_name]
        self.ws, self.total = _buffers(shape_name)
        w = c["w"]
        self.w = {k: _dev(v) for k, v in w.items()}
        self.w["w2a"] = _dev(w["w2a_t"].T)                    # actor_linear2.weight as PyTorch stores it
        self.index = None if c["index"] is None else _dev(c["index"])
        if c["index"] is not None:
            self.n_dev = torch.tensor([c["count"]], dtype=torch.int32, device="cuda")
            self.inv_dev = torch.tensor([1.0 / max(c["count"], 1)], dtype=torch.float32, device="cuda")

    def __call__(self, obs=None, mask=None, action=None, q=None):
        c, L = self.c, self.L
        obs, mask = c["obs"] if obs is None else obs, c["mask"] if mask is None else mask
        action, q = c["action"] if action is None else action, c["q"] if q is None else q
        rows, n = obs.shape[0], c["n"]
        # nothing may reach out of range: shapes, types and every index are checked here, on the host
        assert obs.shape == (rows, self.IN) and obs.dtype == np.float32 and mask.shape == (rows, self.A) and mask.dtype == np.uint8
        assert action.shape == (rows,) and action.dtype == np.int32 and q.shape == (rows,) and q.dtype == np.float32
        assert 1 <= c["parts"] <= 256 and n >= 0
        if c["index"] is None:
            assert n == rows
        else:
            assert c["index"].dtype == np.int32 and len(c["index"]) == n and 0 <= c["count"] <= n
            assert int(c["index"].min()) >= 0 and int(c["index"].max()) < rows
        d = [_dev(obs), _dev(mask), _dev(action), _dev(q)]
        grad = torch.full((self.total,), float("nan"), device="cuda")
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        w = self.w
        inv_host = 1.0 if c["index"] is not None else (c["inv_n"] if c["inv_n"] is not None else 1.0 / max(n, 1))
        L.check(L.lib.azul_a2c_gradients(p(d[0]), p(d[1]), p(d[2]), p(d[3]), n, C.c_float(inv_host), p(w["w1t"]), p(w["b1"]), p(w["w2c"]),
                                         p(w["b2c"]), p(w["w2a_t"]), p(w["b2a"]), p(w["w2a"]), self.IN, 180, self.A, p(self.ws), c["parts"],
                                         p(grad), p(self.index), p(self.n_dev) if c["index"] is not None else None,
                                         p(self.inv_dev) if c["index"] is not None else None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return grad.cpu().numpy()


def _compare(tag, got, shape, c, ref, K):
    """The per-element bound and the exact properties of one result against one reference."""
    IN, A = shape
    flat, sums, N, _ = ref
    size = R.flat_size(IN, A)
    assert np.isfinite(got).all(), tag
    worst, zeros_ok = R.normalised_error(got[:size], flat, N)
    print("NORMALISED %s worst %.2f K_case %.1f" % (tag, worst, K))
    assert zeros_ok, "%s: an element without a single non-zero term is not exactly 0.0" % tag
    assert worst <= K, "%s: normalised error %.1f above K_case %.1f" % (tag, worst, K)
    o = R.offsets(IN, A)
    assert got[o["pad"][0]] == 0.0, tag
    assert got[size + 3] == sums[3], (tag, got[size + 3], sums[3])
    # columns of dw2a_t / db2a of actions that are legal in no sample used
    used, _ = R._used(c["mask"] if "mask_used" not in c else c["mask_used"], c["index"], c["count"])
    never = ~((c["mask"] if "mask_used" not in c else c["mask_used"])[used] != 0).any(axis=0) if len(used) else np.ones(A, bool)
    assert (got[o["w2a_t"][0]:o["b2a"][0]].reshape(180, A)[:, never] == 0.0).all() and (got[o["b2a"][0]:size][never] == 0.0).all(), tag
    # the three logged sums: the 2e-5 of the existing learner tests, taken on the largest of them (adv ~ 0 makes the actor sum pure noise)
    tol = 2e-5 * float(np.abs(sums[:3]).max()) + 1e-6
    assert (np.abs(got[size:size + 3] - sums[:3]) <= tol).all(), (tag, got[size:size + 3], sums[:3])


def _other_content(rs, c, rows_dead):
    """Other finite observations, actions and returns in the rows that carry no sample."""
    obs, action, q = c["obs"].copy(), c["action"].copy(), c["q"].copy()
    A = c["mask"].shape[1]
    obs[rows_dead] = rs.randint(0, 9, size=(len(rows_dead), obs.shape[1])).astype(np.float32) - 3.0
    action[rows_dead] = rs.randint(0, A, len(rows_dead)).astype(np.int32)
    q[rows_dead] = (rs.randn(len(rows_dead)) * 50).astype(np.float32)
    return obs, action, q


@pytest.mark.parametrize("shape_name,case_name", [p for p in PARAMS if p[1] != "sweep"], ids=["%s-%s" % p for p in PARAMS if p[1] != "sweep"])
def test_gradients_per_element_at_the_edges(shape_name, case_name):
    shape = R.SHAPES[shape_name]
    c = R.build(shape_name, case_name)
    ref = R.reference(shape, c["w"], *R.call_args(c))
    K = R.k_case(R.yardstick(shape, c))
    assert K * R.ULP <= 1e-3
    run = Launcher(shape_name, c)
    got = run()
    _compare("%s %s" % (shape_name, case_name), got, shape, c, ref, K)
    if c["index"] is not None and c["count"] == 0:
        assert (got == 0.0).all()
    # the same call twice: the same bits
    assert np.array_equal(got, run())
    # dead content: rows without a legal action, and on the index path every row the first `count` entries do not name
    rows = c["obs"].shape[0]
    used, _ = R._used(c["mask"], c["index"], c["count"])
    dead = np.setdiff1d(np.arange(rows), used)
    if len(dead):
        obs, action, q = _other_content(np.random.RandomState(5), c, dead)
        assert np.array_equal(got, run(obs=obs, action=action, q=q)), "content of rows that carry no sample reached the result"


@pytest.mark.parametrize("shape_name", list(R.SHAPES))
def test_position_sweep_every_row_alone(shape_name):
    """n = 2M + 1 on two parts (workgroup 0 makes two passes): launch k has a legal action in row k only and must give the reference of
    sample k alone, scaled by 1 / n -- a row that is dropped, doubled or routed to another MFMA row is an O(1) error in every role."""
    shape = R.SHAPES[shape_name]
    c = R.build(shape_name, "sweep")
    n = c["n"]
    run = Launcher(shape_name, c)
    for k in range(n):
        one = dict(c, obs=c["obs"][k:k + 1], mask=c["mask"][k:k + 1], action=c["action"][k:k + 1], q=c["q"][k:k + 1], inv_n=1.0 / n)
        ref = R.reference(shape, c["w"], *R.call_args(one))
        K = R.k_case(R.yardstick(shape, one))
        assert K * R.ULP <= 1e-3
        mk = R.sweep_mask(c, k)
        got = run(mask=mk)
        _compare("%s sweep row %d" % (shape_name, k), got, shape, dict(c, mask_used=mk), ref, K)
        if k == R.samples_per_pass(*shape):                  # dead content, once: every other row rewritten
            dead = np.setdiff1d(np.arange(n), [k])
            obs, action, q = _other_content(np.random.RandomState(6), c, dead)
            assert np.array_equal(got, run(obs=obs, mask=mk, action=action, q=q))
