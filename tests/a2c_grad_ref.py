"""An independent float64 restatement of the A2C gradient (the loss of agent.py:39-62 in the closed form at the top of
csrc/azul_learner.hpp) and the table of edge cases that tests/test_gpu_a2c_grad_edges.py, tests/test_a2c_grad_ref.py and the two
emulation files run through azul_a2c_gradients.  Plain numpy on the CPU: no project code is imported here.

    X1 = [x | 1]  [n][IN+1]        W1 = [w1t ; b1]  [IN+1][360]       pre = X1 W1,  H = relu(pre)
    v  = H[:, :180] w2c + b2c      H1 = [H[:, 180:] | 1]  [n][181]    logits = H1 [w2a_t ; b2a]
    logp = masked log-softmax      adv = q - v                        p = softmax over the legal actions
    dL/dv       = (logp[a] - adv) inv_n
    g_j         = -adv [j == a] - 0.1 / |legal|   (legal j),  G = sum_j g_j = -adv - 0.1
    dLogits_j   = (g_j - p_j G) inv_n             (legal j; 0 otherwise)
    dZ [n][360] = [ dv w2c^T | dLogits w2a_t^T ] * (pre > 0)
    dW1 = X1^T dZ (row IN: db1)    dw2c = H[:, :180]^T dv    db2c = sum dv    dW2 = H1^T dLogits (row 180: db2a)

Rows without a legal action carry no sample.  Flat layout (azul_a2c_flat_size): dw1t | db1 | dw2c | db2c | pad | dw2a_t | db2a.

Next to the gradient, `reference` returns N, the "sum of absolute terms" of every element: the same backward pass with every matrix
product taken on absolute values and the non-cancelling magnitudes (|g_j| + p_j |G|) inv_n for dLogits and (|logp[a]| + |adv|) inv_n
for dL/dv.  An element that is small because its terms cancel is then held to the size of its terms, not to its own size."""
import collections

import numpy as np

SHAPES = collections.OrderedDict([("ref", (136, 180)), ("p3_d5", (188, 180)), ("p4_d5", (240, 180)), ("p3_d7", (198, 240)),
                                  ("p4_d9", (260, 300))])
HID = 180
QUANT = 1024.0         # first-layer weights and biases are multiples of 1 / QUANT: with integer observations every pre-activation is
                       # a sum of fewer than 2^24 such steps, EXACT in f32 in any summation order (so is relu h; see make_weights)
MARGIN = 2.0 / QUANT   # every sample used keeps |pre-activation| >= MARGIN (0.00195; the floor asked for is 1e-3)
ULP = 2.0 ** -24
POISON_ROW = 0         # device-count cases: row 0 of the arrays is NaN; every index entry past the count points at it


def samples_per_pass(IN, A):
    return 32 if (IN, A) == (136, 180) else 16


def flat_size(IN, A):
    return IN * 360 + 542 + 181 * A


def offsets(IN, A):
    b1 = IN * 360
    return {"w1t": (0, (IN, 360)), "b1": (b1, (360,)), "w2c": (b1 + 360, (HID,)), "b2c": (b1 + 540, (1,)), "pad": (b1 + 541, (1,)),
            "w2a_t": (b1 + 542, (HID, A)), "b2a": (b1 + 542 + HID * A, (A,))}


def _used(mask, index, count):
    """Source rows of the samples a call uses, in order: index[:count] (or every row), without the rows that have no legal action."""
    if index is not None:
        cnt = len(index) if count is None else int(count)
        rows = np.asarray(index[:cnt], dtype=np.int64)
    else:
        cnt = mask.shape[0] if count is None else int(count)
        rows = np.arange(cnt, dtype=np.int64)
    live = (mask[rows] != 0).any(axis=1) if len(rows) else np.zeros(0, bool)
    return rows[live], cnt


def _evaluate(dt, shape, w, obs, mask, action, q, index, count, inv_n):
    IN, A = shape
    rows, cnt = _used(mask, index, count)
    inv_n = dt(1.0 / max(cnt, 1) if inv_n is None else inv_n)
    n = len(rows)
    x = obs[rows].astype(dt)
    legal = mask[rows] != 0
    act = np.asarray(action)[rows].astype(np.int64)
    qv = np.asarray(q)[rows].astype(dt)
    one = np.ones((n, 1), dt)
    X1 = np.concatenate([x, one], axis=1)
    W1 = np.concatenate([w["w1t"].astype(dt), w["b1"].astype(dt)[None]], axis=0)
    w2c, w2a_t = w["w2c"].astype(dt), w["w2a_t"].astype(dt)
    pre = X1 @ W1
    on = pre > 0
    H = np.where(on, pre, dt(0))
    v = H[:, :HID] @ w2c + w["b2c"].astype(dt)[0]
    H1 = np.concatenate([H[:, HID:], one], axis=1)
    logits = H1 @ np.concatenate([w2a_t, w["b2a"].astype(dt)[None]], axis=0)
    assert legal[np.arange(n), act].all(), "the chosen action of a used sample must be legal"
    m = np.where(legal, logits, -np.inf).max(axis=1, keepdims=True) if n else np.zeros((0, 1), dt)
    z = np.where(legal, logits - m, dt(0))
    e = np.where(legal, np.exp(z), dt(0))
    S = e.sum(axis=1, keepdims=True)
    logS = np.log(S)
    p = e / S
    cntl = legal.sum(axis=1).astype(dt)
    logp_a = (z - logS)[np.arange(n), act]
    adv = qv - v
    hot = np.zeros((n, A), dt)
    hot[np.arange(n), act] = 1
    g = np.where(legal, -adv[:, None] * hot - dt(0.1) / cntl[:, None], dt(0))
    G = -adv - dt(0.1)
    dlog = np.where(legal, (g - p * G[:, None]) * inv_n, dt(0))
    dv = (logp_a - adv) * inv_n
    dZ = np.concatenate([dv[:, None] * w2c[None], dlog @ w2a_t.T], axis=1) * on
    dW1, dW2 = X1.T @ dZ, H1.T @ dlog
    flat = np.zeros(flat_size(IN, A), dt)
    o = offsets(IN, A)

    def put(vec, dW1_, dw2c_, db2c_, dW2_):
        vec[:o["b1"][0] + 360] = dW1_.reshape(-1)
        vec[o["w2c"][0]:o["w2c"][0] + HID] = dw2c_
        vec[o["b2c"][0]] = db2c_
        vec[o["w2a_t"][0]:] = dW2_.reshape(-1)

    put(flat, dW1, H[:, :HID].T @ dv, dv.sum(), dW2)
    ent = -(np.where(legal, z - logS, dt(0)).sum(axis=1) / cntl)
    sums = np.array([(-logp_a * adv).sum(), (adv * adv).sum(), ent.sum(), n], dt)
    # the sum of absolute terms
    Nlog = np.where(legal, (np.abs(g) + p * np.abs(G)[:, None]) * inv_n, dt(0))
    Ndv = (np.abs(logp_a) + np.abs(adv)) * inv_n
    NdZ = np.concatenate([Ndv[:, None] * np.abs(w2c)[None], Nlog @ np.abs(w2a_t).T], axis=1) * on
    N = np.zeros(flat_size(IN, A), dt)
    put(N, np.abs(X1).T @ NdZ, H[:, :HID].T @ Ndv, Ndv.sum(), H1.T @ Nlog)
    margin = float(np.abs(pre).min()) if n else float("inf")
    return flat, sums, N, margin


def reference(shape, weights, obs, mask, action, q, index=None, count=None, inv_n=None):
    """(flat gradient, the four sums, N, min |pre-activation| over the samples used), all float64.  shape = (IN, A)."""
    return _evaluate(np.float64, shape, weights, obs, mask, action, q, index, count, inv_n)


def reference_f32(shape, weights, obs, mask, action, q, index=None, count=None, inv_n=None):
    """The same formulas in numpy float32: the yardstick of the tolerance (what plain f32 arithmetic loses), not a second reference."""
    with np.errstate(all="ignore"):
        return _evaluate(np.float32, shape, weights, obs, mask, action, q, index, count, inv_n)


def normalised_error(got, flat, N):
    """max |got - ref| / (2^-24 N) over the elements with N > 0, and whether every element with N == 0 is exactly 0.0."""
    got = np.asarray(got, np.float64)
    pos = N > 0
    worst = float((np.abs(got[pos] - flat[pos]) / (ULP * N[pos])).max()) if pos.any() else 0.0
    return worst, bool((got[~pos] == 0.0).all())


def yardstick(shape, c, **over):
    """The case's f32 yardstick: the normalised error of reference_f32 against reference (CPU only, never the kernel)."""
    a = call_args(c, **over)
    flat, _, N, _ = reference(shape, c["w"], *a)
    f32 = reference_f32(shape, c["w"], *a)[0]
    return normalised_error(f32, flat, N)[0]


def k_case(y):
    return max(64.0, 8.0 * y)


def call_args(c, mask=None):
    return (c["obs"], c["mask"] if mask is None else mask, c["action"], c["q"], c["index"], c["count"], c["inv_n"])


def sweep_mask(c, k):
    """Position sweep: the mask of launch k -- row k keeps its legal set, every other row has no legal action."""
    m = np.zeros_like(c["mask"])
    m[k] = c["mask"][k]
    return m


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def make_weights(IN, A, seed):
    rs = np.random.RandomState(seed)
    w = {"w1t": rs.randn(IN, 360) * 0.06, "b1": rs.randn(360) * 0.05, "w2c": rs.randn(HID) * 0.1, "b2c": rs.randn(1) * 0.1,
         "w2a_t": rs.randn(HID, A) * 0.1, "b2a": rs.randn(A) * 0.05}
    # The hidden layer is made exact: w1t and b1 on a grid of 1 / QUANT, observations small integers.  Otherwise a hidden unit close to
    # the kink carries the f32 rounding of a 136..260-term sum relative to its own small size (about 1e-6 / |h|, thousands of ulps at
    # |h| = 1e-3) into every dW2a_t element it feeds, and no per-element bound below 1e-3 could hold for an f32 evaluation at all.
    # A wrong row, column or k-step of the layer-1 GEMM still moves h by O(1); only its rounding is taken out of the comparison.
    for k in ("w1t", "b1"):
        w[k] = np.round(w[k] * QUANT) / QUANT
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def pre64(w, obs):
    return obs.astype(np.float64) @ w["w1t"].astype(np.float64) + w["b1"].astype(np.float64)


def forward64(w, obs):
    h = np.maximum(pre64(w, obs), 0.0)
    v = h[:, :HID] @ w["w2c"].astype(np.float64) + float(w["b2c"][0])
    return v, h[:, HID:] @ w["w2a_t"].astype(np.float64) + w["b2a"].astype(np.float64)


def clear_rows(w, IN, n, rs):
    """n observation rows (small integers, like the game's counts) whose 360 pre-activations all stay MARGIN away from the ReLU
    kink: spare rows are drawn and the first n clear ones kept, so n is exact and nothing is filtered at test time."""
    out = np.zeros((0, IN), np.float32)
    while len(out) < n:
        cand = rs.randint(0, 6, size=(max(64, 16 * n), IN)).astype(np.float32)
        ok = (np.abs(pre64(w, cand)) >= MARGIN).all(axis=1)
        out = np.concatenate([out, cand[ok]])
    return np.ascontiguousarray(out[:n])


def random_mask(rs, n, A, p=0.2):
    m = rs.rand(n, A) < p
    act = rs.randint(0, A, n).astype(np.int32)
    m[np.arange(n), act] = True
    return m.astype(np.uint8), act


def _case(w, obs, mask, action, q, parts, index=None, count=None, n=None, inv_n=None, **meta):
    return {"w": w, "obs": np.ascontiguousarray(obs, np.float32), "mask": np.ascontiguousarray(mask, np.uint8),
            "action": np.ascontiguousarray(action, np.int32), "q": np.ascontiguousarray(q, np.float32), "parts": int(parts),
            "index": None if index is None else np.ascontiguousarray(index, np.int32), "count": count,
            "n": int(obs.shape[0] if n is None else n), "inv_n": inv_n, "meta": meta}


def _plain(IN, A, n, seed, parts, p=0.2):
    rs = np.random.RandomState(seed)
    w = make_weights(IN, A, 1000 + IN + A)
    obs = clear_rows(w, IN, n, rs)
    mask, act = random_mask(rs, n, A, p)
    return rs, w, obs, mask, act, returns_for(rs, w, obs)


def returns_for(rs, w, obs):
    """Returns 1 to 6 away from the value, either side: adv = q - v is itself a difference, and where it happens to come out near 0
    (or near -0.1, where G vanishes) its f32 rounding is large beside the magnitudes N is built from.  The adv-zero case goes there on
    purpose, with few legal actions; every other case stays clear of it."""
    n = obs.shape[0]
    away = np.where(rs.rand(n) < 0.5, -1.0, 1.0) * (1.0 + 5.0 * rs.rand(n))
    return (forward64(w, np.nan_to_num(obs))[0] + away).astype(np.float32)


def b_sweep(IN, A):
    M = samples_per_pass(IN, A)
    rs, w, obs, mask, act, q = _plain(IN, A, 2 * M + 1, 11, 2)
    return _case(w, obs, mask, act, q, 2, sweep=True)


def b_size(mult, add, parts):
    def build(IN, A):
        n = mult * samples_per_pass(IN, A) + add
        rs, w, obs, mask, act, q = _plain(IN, A, n, 20 + n, parts)
        return _case(w, obs, mask, act, q, parts)
    return build


def b_long(IN, A):
    rs, w, obs, mask, act, q = _plain(IN, A, 16 * 3 * 8 + 5, 31, 3)
    return _case(w, obs, mask, act, q, 3)


def _edge(fn, seed):
    """A softmax / mask edge at n = M + 1 on two parts: fn(rs, d) edits the dict of arrays in place."""
    def build(IN, A):
        M = samples_per_pass(IN, A)
        rs, w, obs, mask, act, q = _plain(IN, A, M + 1, seed, 2)
        d = {"w": {k: v.copy() for k, v in w.items()}, "obs": obs, "mask": mask, "action": act, "q": q, "meta": {}, "IN": IN, "A": A, "M": M}
        fn(rs, d)
        if d.get("redraw"):                                  # the first layer changed: draw the rows again for the new weights
            d["obs"] = clear_rows(d["w"], IN, M + 1, rs)
        if d.get("redraw"):
            d["q"] = returns_for(rs, d["w"], d["obs"])
        if "q_fn" in d:
            d["q"] = d["q_fn"](d)
        return _case(d["w"], d["obs"], d["mask"], d["action"], d["q"], 2, **d["meta"])
    return build


def _one_legal(where):
    def fn(rs, d):
        n, A = d["mask"].shape
        col = {"first": np.zeros(n, int), "last": np.full(n, A - 1), "random": rs.randint(0, A, n)}[where]
        d["mask"][:] = 0
        d["mask"][np.arange(n), col] = 1
        d["action"] = col.astype(np.int32)
    return fn


def _all_legal(rs, d):
    d["mask"][:] = 1


def _last_tile(rs, d):
    n, A = d["mask"].shape
    lo = 16 * ((A - 1) // 16)
    d["mask"][:, :lo] = 0
    d["mask"][:, lo:] = rs.rand(n, A - lo) < 0.5
    d["action"] = (lo + rs.randint(0, A - lo, n)).astype(np.int32)
    d["mask"][np.arange(n), d["action"]] = 1
    d["meta"]["first_legal_column"] = lo


def _action_at(last):
    def fn(rs, d):
        n, A = d["mask"].shape
        d["action"] = np.full(n, A - 1 if last else 0, np.int32)
        d["mask"][np.arange(n), d["action"]] = 1
    return fn


def _equal_max(rs, d):
    A = d["A"]
    j1, j2 = 5, A - 3                                        # two different column tiles, the second inside the last one
    d["w"]["w2a_t"][:, j2] = d["w"]["w2a_t"][:, j1]
    d["w"]["b2a"][j1] = d["w"]["b2a"][j2] = 30.0             # far above every other logit: both are the row's maximum
    d["mask"][:, [j1, j2]] = 1
    d["meta"]["equal_max"] = (j1, j2)


def _span60(rs, d):
    d["w"]["w2a_t"] *= 15.0                                  # logits tens apart: the max-subtraction path
    d["w"]["b2a"] *= 15.0
    d["meta"]["span"] = 60.0


def _mask_bytes(rs, d):
    n, A = d["mask"].shape
    d["mask"][:] = np.array([0, 0, 0, 1, 2, 0x80, 0xff], np.uint8)[rs.randint(0, 7, (n, A))]
    d["mask"][np.arange(n), d["action"]] = np.array([1, 2, 0x80, 0xff], np.uint8)[rs.randint(0, 4, n)]
    d["meta"]["mask_bytes"] = True


def _adv_zero(rs, d):
    # two to four legal actions and the least likely of them chosen: 0.1 / |legal| and |logp[a]| >= log 2 keep the scale of N where
    # adv itself is rounding noise (with one legal action logp[a] = 0 and dL/dv would be noise over noise)
    n, A = d["mask"].shape
    logits = forward64(d["w"], d["obs"])[1]
    d["mask"][:] = 0
    for i in range(n):
        legal = rs.choice(A, 2 + i % 3, replace=False)
        d["mask"][i, legal] = 1
        d["action"][i] = legal[np.argmin(logits[i, legal])]
    d["q_fn"] = lambda d_: forward64(d_["w"], d_["obs"])[0].astype(np.float32)         # q = the fp64 value rounded to f32
    d["meta"]["adv_zero"] = True


def _q_big(rs, d):
    d["q"] = (np.where(rs.rand(len(d["q"])) < 0.5, -1.0, 1.0) * 1e4).astype(np.float32)


def _dead_rows(whole_tile):
    def fn(rs, d):
        M = d["M"]
        dead = np.arange(M) if whole_tile else np.array([0, M - 1, M])       # (n = M + 1: row M is also row n - 1)
        d["mask"][dead] = 0
        d["meta"]["dead"] = dead
    return fn


def _straddle(rs, d):
    # hidden units 176..191 (column tile 11: critic units 176..179, actor units 0..11) active on every sample: observations are >= 0
    d["w"]["w1t"][:, 176:192] = np.abs(d["w"]["w1t"][:, 176:192])
    d["w"]["b1"][176:192] = np.abs(d["w"]["b1"][176:192]) + np.float32(52.0 / QUANT)
    d["redraw"] = True
    d["meta"]["straddle"] = True


def b_count(kind, cmul, cadd):
    """The device-count path: n_samples = 3M on the host, the count in device memory; row POISON_ROW is NaN and every index entry
    past the count points at it."""
    def build(IN, A):
        M = samples_per_pass(IN, A)
        count, n_host, rows = cmul * M + cadd, 3 * M, 3 * M + 4
        rs, w, obs, mask, act, q = _plain(IN, A, rows, 40 + 7 * cmul + cadd + {"perm": 0, "repeat": 100, "reverse": 200}[kind], 2)
        obs[POISON_ROW], q[POISON_ROW], act[POISON_ROW], mask[POISON_ROW] = np.nan, np.nan, 0, 1
        if kind == "perm":
            head = 1 + rs.permutation(rows - 1)[:count]
        elif kind == "repeat":                               # a repeated row counts twice
            head = 1 + rs.randint(0, max(1, (count + 1) // 2), count)
        else:
            head = np.arange(rows - 1, rows - 1 - count, -1)
        index = np.full(n_host, POISON_ROW, np.int32)
        index[:count] = head
        return _case(w, obs, mask, act, q, 2, index=index, count=count, n=n_host, poison=True)
    return build


Case = collections.namedtuple("Case", "name build group")
CASES = [Case("sweep", b_sweep, "sweep")]
for _name, (_m, _a) in (("1", (0, 1)), ("M-1", (1, -1)), ("M", (1, 0)), ("M+1", (1, 1)), ("2M-1", (2, -1)), ("2M", (2, 0)), ("2M+1", (2, 1)),
                        ("4M+3", (4, 3))):
    for _p in (1, 2, 3, 256):
        CASES.append(Case("n=%s-parts%d" % (_name, _p), b_size(_m, _a, _p), "size"))
# azul_a2c_reduce_kernel adds eight parts per round and the rest one by one: 7, 8, 9 and 17 parts actually launched (the host entry
# launches min(tiles, workspace_parts); the other size cases launch at most 5)
REDUCE_EDGE_PARTS = collections.OrderedDict([("6M+9", 7), ("7M+9", 8), ("8M+9", 9), ("16M+9", 17)])
for _name in REDUCE_EDGE_PARTS:
    CASES.append(Case("n=%s-parts17" % _name, b_size(int(_name.split("M")[0]), 9, 17), "size"))
CASES.append(Case("n=389-parts3", b_long, "long"))           # run on the wide shapes whose action count ends inside a 16-column tile
CASES += [Case(nm, _edge(fn, 50 + i), "edge") for i, (nm, fn) in enumerate([
    ("one-legal-first", _one_legal("first")), ("one-legal-last", _one_legal("last")), ("one-legal-random", _one_legal("random")),
    ("all-legal", _all_legal), ("only-last-action", _one_legal("last")), ("last-tile-only", _last_tile),
    ("action-0", _action_at(False)), ("action-last", _action_at(True)), ("equal-max", _equal_max), ("logit-span-60", _span60),
    ("mask-bytes", _mask_bytes), ("adv-zero", _adv_zero), ("q-1e4", _q_big), ("dead-rows", _dead_rows(False)),
    ("dead-tile", _dead_rows(True)), ("straddle", _straddle)])]
for _kind in ("perm", "repeat", "reverse"):
    for _name, (_m, _a) in (("0", (0, 0)), ("1", (0, 1)), ("M-1", (1, -1)), ("M+1", (1, 1))):
        CASES.append(Case("index-%s-count=%s" % (_kind, _name), b_count(_kind, _m, _a), "count"))
BY_NAME = {c.name: c for c in CASES}


def cases_for(shape_name):
    """The cases of a shape: all of them, except that n = 389 runs where the action count is no multiple of 16 on a wide shape."""
    IN, A = SHAPES[shape_name]
    return [c for c in CASES if c.group != "long" or (shape_name != "ref" and A % 16 != 0)]


def all_params():
    return [(s, c.name) for s in SHAPES for c in cases_for(s)]


def build(shape_name, case_name):
    return BY_NAME[case_name].build(*SHAPES[shape_name])


# the subset the lockstep emulation runs (tests/test_hostcheck_learner.py on "ref", tests/test_hostcheck_learner_n.py on "p4_d9")
EMULATION_CASES = ("n=M+1-parts1", "n=M+1-parts2", "one-legal-random", "only-last-action", "index-perm-count=M-1")


def emulation_sweep_rows(IN, A):
    M = samples_per_pass(IN, A)
    return (0, M - 1, M, 2 * M)
