"""The wide-shape A2C kernels on CPU: azul_a2c_grad_n_kernel<IN, A> (csrc/azul_learner.hpp: three workgroup roles per part, gradient
tiles in registers), azul_a2c_reduce_n_kernel and azul_a2c_apply_n_kernel on their layouts, compiled UNMODIFIED by g++ and run as workgroups of emulated wavefronts
(tests/hostcheck/simt) -- gradients and loss sums against float64 autograd of the reference's loss (agent.py:39-62) for p3_d5 and
p4_d9 with several passes per part, a ragged last tile and rows without a legal action; Adam against torch.optim.Adam."""
import ctypes as C

import numpy as np
import torch

from tests.hostcheck import hostcheck


def load():
    L = C.CDLL(hostcheck.build("libsimt_learner_n.so"))
    L.sln_gradients.restype = C.c_longlong
    L.sln_gradients.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 9
    L.sln_gradients_dev.restype = C.c_longlong
    L.sln_gradients_dev.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 11
    L.sln_adam.restype = C.c_longlong
    L.sln_adam.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_float] * 4 + [C.c_int] + [C.c_void_p] * 8
    L.sln_flat_size.restype = C.c_int
    L.sln_buffer_oob.restype = C.c_ulonglong
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _weights(rs, IN, A):
    w = {"w1t": rs.randn(IN, 360) * 0.06, "b1": rs.randn(360) * 0.05, "w2c": rs.randn(180) * 0.1, "b2c": rs.randn(1) * 0.1,
         "w2a_t": rs.randn(180, A) * 0.1, "b2a": rs.randn(A) * 0.05}
    w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}
    w["w2a"] = np.ascontiguousarray(w["w2a_t"].T)                       # actor_linear2.weight as PyTorch stores it
    return w


def _offsets(IN, A):
    b1 = IN * 360
    return {"w1t": (0, (IN, 360)), "b1": (b1, (360,)), "w2c": (b1 + 360, (180,)), "b2c": (b1 + 540, (1,)), "w2a_t": (b1 + 542, (180, A)),
            "b2a": (b1 + 542 + 180 * A, (A,))}


def _check_gradients(IN, A, n, parts, seed):
    L = load()
    rs = np.random.RandomState(seed)
    w = _weights(rs, IN, A)
    obs = rs.randint(0, 6, size=(n, IN)).astype(np.float32)
    mask = rs.rand(n, A) < 0.2
    act = rs.randint(0, A, n).astype(np.int32)
    mask[np.arange(n), act] = True
    mask[3] = False                                                     # rows without a legal action carry no sample
    mask[n - 1] = False
    q = (rs.randn(n) * 5).astype(np.float32)
    mask = np.ascontiguousarray(mask.astype(np.uint8))
    size = L.sln_flat_size(IN, A)
    assert size == IN * 360 + 542 + 181 * A
    partial = np.zeros((parts, size + 4), np.float32)
    grad = np.zeros(size + 4, np.float32)
    L.sln_gradients(IN, A, n, parts, ptr(obs), ptr(mask), ptr(act), ptr(q), None, C.c_float(1.0 / n), ptr(w["w1t"]), ptr(w["b1"]),
                    ptr(w["w2c"]), ptr(w["b2c"]), ptr(w["w2a_t"]), ptr(w["b2a"]), ptr(w["w2a"]), ptr(partial), ptr(grad))
    assert L.sln_buffer_oob() == 0
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items() if k != "w2a"}
    keep = torch.tensor(mask.astype(bool)).any(1)
    x = torch.tensor(obs, dtype=torch.float64)[keep]
    legal = torch.tensor(mask.astype(bool))[keep]
    h = torch.relu(x @ t["w1t"] + t["b1"])
    v = h[:, :180] @ t["w2c"] + t["b2c"]
    lp = torch.log_softmax((h[:, 180:] @ t["w2a_t"] + t["b2a"]).masked_fill(~legal, float("-inf")), 1)
    lpa = lp.gather(1, torch.tensor(act).long()[keep].unsqueeze(1)).squeeze(1)
    ent = -(torch.where(legal, lp, torch.zeros_like(lp)).sum(1) / legal.sum(1))
    adv = torch.tensor(q, dtype=torch.float64)[keep] - v
    la, lc, le = (-lpa * adv).sum(), (adv ** 2).sum(), ent.sum()
    ((la + 0.5 * lc + 0.1 * le) / n).backward()
    for k, (o, shape) in _offsets(IN, A).items():
        got = grad[o:o + int(np.prod(shape))].reshape(shape)
        ref = t[k].grad.numpy()
        scale = np.abs(ref).max()
        assert np.abs(ref - got).max() <= 2e-5 * scale + 1e-7, k        # test_hostcheck_learner.py's tolerance
    assert grad[size - 181 * A - 1] == 0.0                              # the pad float
    sums = grad[size:]
    assert int(sums[3]) == int(keep.sum())
    for want, got in zip((la, lc, le), sums[:3]):
        assert np.isclose(float(want), float(got), rtol=2e-5, atol=1e-4)


def test_wide_gradients_p3_d5_under_emulation_match_autograd():
    _check_gradients(188, 180, 83, 2, 11)            # 6 tiles over 2 parts: three passes each, a ragged last tile of 3 samples


def test_wide_gradients_p4_d9_under_emulation_match_autograd():
    _check_gradients(260, 300, 70, 2, 12)            # 5 tiles: passes of 3 and 2, last tile of 6 samples


def _run_edge_case(L, IN, A, c, mask=None):
    size = L.sln_flat_size(IN, A)
    w = c["w"]
    w2a = np.ascontiguousarray(w["w2a_t"].T)
    parts = min(c["parts"], (c["n"] + 15) // 16)                        # (the host entry launches min(tiles, workspace_parts) parts)
    partial, grad = np.zeros((parts, size + 4), np.float32), np.full(size + 4, np.nan, np.float32)
    mask = c["mask"] if mask is None else mask
    n_dev = inv_dev = None
    inv_host = c["inv_n"] if c["inv_n"] is not None else 1.0 / max(c["n"], 1)
    if c["index"] is not None:
        assert int(c["index"].min()) >= 0 and int(c["index"].max()) < c["obs"].shape[0]
        n_dev, inv_dev, inv_host = np.array([c["count"]], np.int32), np.array([1.0 / max(c["count"], 1)], np.float32), 1.0
    L.sln_gradients_dev(IN, A, c["n"], parts, ptr(c["obs"]), ptr(mask), ptr(c["action"]), ptr(c["q"]), ptr(c["index"]), C.c_float(inv_host),
                        ptr(n_dev), ptr(inv_dev), ptr(w["w1t"]), ptr(w["b1"]), ptr(w["w2c"]), ptr(w["b2c"]), ptr(w["w2a_t"]), ptr(w["b2a"]),
                        ptr(w2a), ptr(partial), ptr(grad))
    assert L.sln_buffer_oob() == 0
    return grad


def test_wide_gradients_p4_d9_under_emulation_on_the_edge_case_table():
    """p4_d9 on a subset of the case table of tests/a2c_grad_ref.py, through the per-element comparison of
    tests/test_gpu_a2c_grad_edges.py: the position sweep's rows 0, M - 1, M and 2M, n = M + 1 on one and two parts, one legal action,
    only the last action legal, and a device count that ends inside a tile.  Measured: 19 s."""
    from tests import a2c_grad_ref as R
    L = load()
    shape = IN, A = R.SHAPES["p4_d9"]
    size = R.flat_size(IN, A)

    def check(tag, got, c, ref):
        flat, sums, N, _ = ref
        K = R.k_case(R.yardstick(shape, c))
        worst, zeros_ok = R.normalised_error(got[:size], flat, N)
        assert np.isfinite(got).all() and zeros_ok, tag
        assert worst <= K, (tag, worst, K)
        assert got[R.offsets(IN, A)["pad"][0]] == 0.0 and got[size + 3] == sums[3], tag

    for name in R.EMULATION_CASES:
        c = R.build("p4_d9", name)
        check(name, _run_edge_case(L, IN, A, c), c, R.reference(shape, c["w"], *R.call_args(c)))
    c = R.build("p4_d9", "sweep")
    for k in R.emulation_sweep_rows(IN, A):
        one = dict(c, obs=c["obs"][k:k + 1], mask=c["mask"][k:k + 1], action=c["action"][k:k + 1], q=c["q"][k:k + 1], inv_n=1.0 / c["n"])
        check("sweep row %d" % k, _run_edge_case(L, IN, A, c, R.sweep_mask(c, k)), one, R.reference(shape, c["w"], *R.call_args(one)))


def test_wide_adam_under_emulation_matches_torch_adam():
    L = load()
    IN, A = 188, 180
    rs = np.random.RandomState(5)
    size = L.sln_flat_size(IN, A)
    flat = (rs.randn(size) * 0.05).astype(np.float32)
    flat[IN * 360 + 541] = 0.0
    m, v = np.zeros(size, np.float32), np.zeros(size, np.float32)
    mods = {"c1w": np.zeros((180, IN), np.float32), "c1b": np.zeros(180, np.float32), "c2w": np.zeros((1, 180), np.float32),
            "c2b": np.zeros(1, np.float32), "a1w": np.zeros((180, IN), np.float32), "a1b": np.zeros(180, np.float32),
            "a2w": np.zeros((A, 180), np.float32), "a2b": np.zeros(A, np.float32)}
    param = torch.tensor(flat.copy(), requires_grad=True)
    opt = torch.optim.Adam([param], lr=3e-4)
    for step in range(1, 4):
        g = (rs.randn(size + 4) * 1e-3).astype(np.float32)
        g[IN * 360 + 541] = 0.0
        L.sln_adam(IN, A, ptr(g), ptr(flat), ptr(m), ptr(v), 3e-4, 0.9, 0.999, 1e-8, step, *[ptr(mods[k]) for k in mods])
        param.grad = torch.tensor(g[:size])
        opt.step()
        assert np.abs(flat - param.detach().numpy()).max() <= 2e-6
    o = _offsets(IN, A)
    w1t = flat[:IN * 360].reshape(IN, 360)
    assert np.array_equal(mods["c1w"], w1t[:, :180].T) and np.array_equal(mods["a1w"], w1t[:, 180:].T)
    assert np.array_equal(mods["a2w"], flat[o["w2a_t"][0]:o["b2a"][0]].reshape(180, A).T)
    assert np.array_equal(mods["a2b"], flat[o["b2a"][0]:]) and mods["c2b"][0] == flat[o["b2c"][0]]
