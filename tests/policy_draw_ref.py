"""Host reference of the policy head's draws (csrc/azul_policy.hpp: policy_head_rows), numpy only.

    philox4x32_10        Philox4x32-10 (Salmon et al., SC'11), vectorised over uint64 arrays holding 32-bit words
    policy_uniform       the kernels' mapping: ctr = (counter lo, counter hi, global game id, 0x415A554C "AZUL"), key = (seed lo, seed hi),
                         u = (word 0 >> 8) * 2^-24
    masked_log_softmax   log p over the legal actions and the entropy term -mean(log p over legal) of nn_runner.py:36-40, in float64
    sample               np.random.choice's inverse CDF (agent.py:68-69): float64 cumsum, normalised, searchsorted(u, side="right");
                         argmax mode (agent.py:70-71) is the first maximum among the legal actions; a row with no legal action gives -1
    boundary_distance    how far u lies from the CDF boundaries around the drawn action, so that a test can excuse draws that honestly sit
                         on a boundary (within the f32 error of the kernel's sums)
    head                 all of the above for rows of f32 logits + legal masks, the way the head entries are called
"""
import numpy as np

ARGMAX = 0xFFFFFFFFFFFFFFFF
AZUL_WORD = 0x415A554C
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2; broadcast together.  Returns the 4 output words as uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & _LO for v in ctr])
    c0, c1, c2, c3 = (c.copy() for c in (c0, c1, c2, c3))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _LO for v in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return c0, c1, c2, c3


def policy_word(seed, counter, game):
    """Word 0 of the kernels' Philox block for (seed, counter, global game id); `game` may be an array."""
    seed, counter = int(seed) & ARGMAX, int(counter) & ARGMAX
    game = np.asarray(game, dtype=np.uint64) & _LO
    return philox4x32_10((counter & 0xFFFFFFFF, counter >> 32, game, AZUL_WORD), (seed & 0xFFFFFFFF, seed >> 32))[0]


def policy_uniform(seed, counter, game):
    """The kernels' uniform in [0, 1): 24 bits of word 0, as float64 (exact)."""
    return (policy_word(seed, counter, game) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def masked_log_softmax(logits, mask):
    """float64 (z, w, logp, entropy) from f32 logits [N][A] and a mask: z = x - max over legal, w = exp(z) on legal actions (0 elsewhere),
    logp = z - log(sum w), entropy = -mean(logp over legal).  Rows without a legal action: z = 0, w = 0, entropy 0."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    legal = np.asarray(mask).astype(bool)
    m = np.where(legal, x, -np.inf).max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    z = np.where(legal, x - m, 0.0)
    w = np.where(legal, np.exp(z), 0.0)
    S = w.sum(axis=1, keepdims=True)
    logS = np.log(np.where(S > 0, S, 1.0))
    logp = z - logS
    cnt = legal.sum(axis=1)
    ent = np.where(cnt > 0, -(np.where(legal, logp, 0.0).sum(axis=1) / np.maximum(cnt, 1)), 0.0)
    return z, w, logp, ent


def sample(w, u, mask=None, logits=None, argmax=False):
    """np.random.choice's draw on weights w [N][A] (float64) with uniforms u [N]: searchsorted of the normalised cumsum, side="right".
    Argmax mode: the first maximum of `logits` among the legal actions.  Rows with no legal action (all-zero w / mask): -1."""
    if argmax:
        legal = np.asarray(mask).astype(bool)
        x = np.where(legal, np.asarray(logits, dtype=np.float32).astype(np.float64), -np.inf)
        return np.where(legal.any(axis=1), x.argmax(axis=1), -1)
    cdf = np.cumsum(w, axis=1)
    tot = cdf[:, -1:]
    cdf = cdf / np.where(tot > 0, tot, 1.0)
    a = (cdf <= np.asarray(u, dtype=np.float64)[:, None]).sum(axis=1)
    return np.where(tot[:, 0] > 0, a, -1)


def cdf_of(w):
    cdf = np.cumsum(w, axis=1)
    tot = cdf[:, -1:]
    return cdf / np.where(tot > 0, tot, 1.0)


def boundary_distance(u, cdf, action):
    """min(u - cdf[a-1], cdf[a] - u) for the drawn action a: how far the draw is from choosing a neighbour.  The ends of the CDF are no
    boundaries (u = 0 with nothing of positive weight before a, and cdf[a] = 1 with nothing after it): no other action lies beyond them."""
    n = cdf.shape[0]
    u = np.asarray(u, dtype=np.float64)
    a = np.clip(np.asarray(action), 0, cdf.shape[1] - 1)
    lo = np.where(a > 0, cdf[np.arange(n), np.maximum(a - 1, 0)], 0.0)
    hi = cdf[np.arange(n), a]
    return np.minimum(np.where(lo > 0, u - lo, np.inf), np.where(hi < 1.0, hi - u, np.inf))


def neighbours(cdf, u, action):
    """The two actions on either side of the CDF boundary nearest to u: (left, right), where `right` is the first action of positive weight
    after the boundary and `left` the last of positive weight before it."""
    n, A = cdf.shape
    w = np.diff(np.concatenate([np.zeros((n, 1)), cdf], axis=1), axis=1)
    out = []
    for r in range(n):
        bounds = cdf[r]
        k = int(np.argmin(np.abs(bounds - u[r])))              # boundary k separates actions <= k from actions > k
        pos = np.flatnonzero(w[r] > 0)
        left = pos[pos <= k]
        right = pos[pos > k]
        out.append((int(left[-1]) if left.size else -1, int(right[0]) if right.size else -1))
    return out


def additions(mask, npl):
    """Per row, the most inexact additions behind any partial sum of policy_head_rows: the legal actions of the fullest lane (adding an
    illegal action's 0 is exact) plus the 4 DPP steps of the row_shr scan / the butterfly sum."""
    legal = np.asarray(mask).astype(bool)
    n, na = legal.shape
    lanes = np.zeros((n, 16 * npl), bool)
    lanes[:, :na] = legal
    return lanes.reshape(n, 16, npl).sum(axis=2).max(axis=1) + 4


def draw_delta(z, w, mask, npl):
    """Per-row bound on |kernel CDF - exact CDF| at every boundary, in units of the row's total weight, from the f32 error analysis of
    policy_head_rows (u = 2^-24 the unit round-off):
      * each weight e_j = __expf(z_j) has relative error <= 2|z_j| u + 2u: v_exp_f32 evaluates 2^(z log2 e); rounding the product and the
        constant log2 e each move the exponent by <= |z| log2(e) u, i.e. a relative error of |z| u, plus v_exp_f32's 1 ulp.  The CDF moves
        by at most the weighted mean of those: sum_j (2|z_j| + 2) u w_j / S;
      * every cumulative sum cum_j (lane prefix from the row_shr scan, minus the lane's own sum, plus its sequential steps) and the
        butterfly sum S are sums of non-negative terms with at most k = additions() inexact steps: relative error <= k u each (+1 for the
        prefix's subtraction), so the crossing test target < cum_j moves by <= (2k + 1) u;
      * target = u S rounds once more (u is exact in f32): u.
    x - m is exact (Sterbenz: both are f32 of one sign within a factor 2 whenever exp(x - m) is not negligible).  Second-order terms are
    below 1e-9 of the bound; a factor 1 + 2^-4 covers them."""
    S = w.sum(axis=1)
    exp_err = ((2.0 * np.abs(z) + 2.0) * w).sum(axis=1) / np.where(S > 0, S, 1.0)
    k = additions(mask, npl)
    return 1.0625 * 2.0 ** -24 * (exp_err + 2.0 * k + 2.0)


def logp_tol(z, w, mask, npl):
    """Per-row bound on |kernel log p - exact log p| and on the entropy term: log S carries (npl + 4) u from the sum plus the exp errors
    above plus __logf's 2 ulp of log S (absolute: 2u |log S|, and v_log_f32's absolute error 2^-21 near S = 1); z_sel - log S adds one
    rounding of each.  The entropy's zsum is a sum of <= npl + 4 terms z_j <= 0 in sequence: (npl + 4) u sum |z|; divided by cnt and minus
    log S: one rounding each.  Doubled for second-order terms."""
    S = w.sum(axis=1)
    Sn = np.where(S > 0, S, 1.0)
    logS = np.log(Sn)
    uu = 2.0 ** -24
    exp_err = ((2.0 * np.abs(z) + 2.0) * w).sum(axis=1) / Sn
    base = exp_err * uu + (npl + 4) * uu + 2 * uu * np.abs(logS) + 2.0 ** -21
    legal = np.asarray(mask).astype(bool)
    cnt = np.maximum(legal.sum(axis=1), 1)
    zsum = np.abs(np.where(legal, z, 0.0)).sum(axis=1)
    zmax = np.abs(z).max(axis=1)
    lp = 2.0 * (base + uu * (zmax + np.abs(logS)) + 2.0 ** -22)
    ent = 2.0 * (base + (npl + 6) * uu * zsum / cnt + uu * (zsum / cnt + np.abs(logS)) + 2.0 ** -22)
    return lp, ent


def head(logits, mask, seed, counter, id_base=0, npl=None):
    """Everything the head entries return for f32 logits [N][A] / masks [N][A] at (seed, counter, global ids id_base + row), plus what a
    test needs to judge a kernel's answer: dict with action, logp (of the reference's action), entropy, u, cdf, delta (per row), z, w."""
    logits = np.asarray(logits, dtype=np.float32)
    n, A = logits.shape
    npl = npl or -(-A // 16)
    z, w, logp_all, ent = masked_log_softmax(logits, mask)
    ids = (np.arange(n, dtype=np.uint64) + np.uint64(id_base)) & _LO
    argmax = (int(seed) & ARGMAX) == ARGMAX
    u = np.zeros(n) if argmax else policy_uniform(seed, counter, ids)
    a = sample(w, u, mask=mask, logits=logits, argmax=argmax)
    cdf = cdf_of(w)
    lp = np.where(a >= 0, logp_all[np.arange(n), np.maximum(a, 0)], 0.0)
    return {"action": a, "logp": lp, "logp_all": logp_all, "entropy": ent, "u": u, "cdf": cdf, "delta": draw_delta(z, w, mask, npl), "z": z, "w": w,
            "npl": npl, "mask": np.asarray(mask).astype(bool), "argmax": argmax}


def compare(ref, action, logp, entropy, extra_lp=None, extra_draw=None, extra_ent=None):
    """Judge a kernel's (action, logp, entropy) rows against `head()`'s reference.  Draws whose u lies within the row's delta (plus
    `extra_draw`, e.g. the CDF shift that logit errors cause) of a CDF boundary are excused, and must still pick one of the two actions
    next to that boundary; every other draw must equal the reference's.  logp / entropy must lie within the per-row bounds of logp_tol
    (plus `extra_lp` / `extra_ent`), logp at the kernel's own action.  Returns (compared, excused) over the rows with a legal action;
    raises AssertionError naming the first bad rows."""
    action = np.asarray(action).astype(np.int64)
    logp, entropy = np.asarray(logp, np.float64), np.asarray(entropy, np.float64)
    n = action.shape[0]
    legal = ref["mask"]
    legal_any = legal.any(axis=1)
    assert np.array_equal(action[~legal_any], np.full((~legal_any).sum(), -1)), "rows without a legal action must give -1"
    assert (logp[~legal_any] == 0).all() and (entropy[~legal_any] == 0).all()
    rows = np.flatnonzero(legal_any)
    if rows.size == 0:
        return 0, 0
    assert ((action[rows] >= 0) & (action[rows] < ref["w"].shape[1])).all(), "action out of range"
    assert legal[rows, action[rows]].all(), "a draw picked an action the mask forbids"
    delta = ref["delta"] + (0.0 if extra_draw is None else extra_draw)
    u = ref["u"]
    dist = boundary_distance(u, ref["cdf"], ref["action"])
    near = (dist <= delta) & (not ref["argmax"])          # argmax mode: no boundary, every row must match
    bad = rows[(action[rows] != ref["action"][rows]) & ~near[rows]]
    assert bad.size == 0, "draw mismatch at rows %s: kernel %s, reference %s, u %s, distance %s > delta %s" % (
        bad[:8].tolist(), action[bad[:8]].tolist(), ref["action"][bad[:8]].tolist(), u[bad[:8]].tolist(), dist[bad[:8]].tolist(), delta[bad[:8]].tolist())
    exc = rows[near[rows]]
    if exc.size:
        nb = neighbours(ref["cdf"][exc], u[exc], ref["action"][exc])
        for r, (lo, hi) in zip(exc, nb):
            assert action[r] in (lo, hi, ref["action"][r]), "excused draw at row %d picked %d, not a neighbour (%d, %d) of its boundary" % (r, action[r], lo, hi)
    lp_tol, ent_tol = logp_tol(ref["z"], ref["w"], legal, ref["npl"])
    if extra_lp is not None:
        lp_tol = lp_tol + extra_lp
    if extra_ent is not None:
        ent_tol = ent_tol + extra_ent
    want_lp = ref["logp_all"][rows, action[rows]]
    err = np.abs(logp[rows] - want_lp)
    badl = rows[err > lp_tol[rows]]
    assert badl.size == 0, "log-prob off at rows %s: |err| %s > bound %s" % (badl[:8].tolist(), err[err > lp_tol[rows]][:8].tolist(), lp_tol[badl[:8]].tolist())
    err = np.abs(entropy[rows] - ref["entropy"][rows])
    bade = rows[err > ent_tol[rows]]
    assert bade.size == 0, "entropy off at rows %s: |err| %s > bound %s" % (bade[:8].tolist(), err[err > ent_tol[rows]][:8].tolist(), ent_tol[bade[:8]].tolist())
    return int(rows.size), int(exc.size)


def lane_edges(na):
    """Actions at the edges of the 16-lane split of a row of na actions (lane c owns npl c .. npl c + npl - 1; npl = 12 / 15 / 19)."""
    npl = -(-na // 16)
    return sorted({a for a in (0, npl - 1, npl, 14 * npl - 1, 14 * npl, 15 * npl - 1, 15 * npl, na - 1) if 0 <= a < na})


def input_families(na, n, seed):
    """Rows where heads go wrong, n per random family: {name: (logits f32 [rows][na], mask uint8 [rows][na])}.
      flat / peaked / one_hot: randn x 0.01, x 3 (the existing head tests' regime), x 50 (many legal weights underflow to exactly 0), 30 % legal
      offset:    randn x 3 + 1e4 (the logits' ulp is 2^-10; x - m stays exact)
      edges:     a single legal action at every lane edge (lane_edges), several rows each
      all_legal: every action legal, randn x 3;  none: no action legal"""
    rs = np.random.RandomState(seed)
    out = {}
    for name, scale in (("flat", 0.01), ("peaked", 3.0), ("one_hot", 50.0)):
        out[name] = ((rs.randn(n, na) * scale).astype(np.float32), (rs.rand(n, na) < 0.3).astype(np.uint8))
    out["offset"] = ((rs.randn(n, na) * 3 + 1e4).astype(np.float32), (rs.rand(n, na) < 0.3).astype(np.uint8))
    edges = lane_edges(na)
    rep = 8
    lg = (rs.randn(rep * len(edges), na) * 3).astype(np.float32)
    mk = np.zeros((rep * len(edges), na), np.uint8)
    for i, a in enumerate(edges):
        mk[i * rep:(i + 1) * rep, a] = 1
    out["edges"] = (lg, mk)
    out["all_legal"] = ((rs.randn(n // 4, na) * 3).astype(np.float32), np.ones((n // 4, na), np.uint8))
    out["none"] = ((rs.randn(8, na) * 3).astype(np.float32), np.zeros((8, na), np.uint8))
    return out


def zero_weight_rows(na, n, seed, where):
    """Rows (randn x 3 logits, 30 % legal, >= 2 legal actions) whose last (where="last") or first (where="first") legal action sits 110 below
    the row maximum: its f32 weight exp(-110) ~ 1.7e-48 is exactly 0, so np.random.choice on the f32 softmax (agent.py:68) never draws it.
    The legal action next to it holds the row maximum, so u = 1 - k 2^-24 (k <= 4) falls inside it.  Returns logits, mask, the zero-weight
    action and that neighbour (the last / first legal action of positive weight)."""
    rs = np.random.RandomState(seed)
    lg = (rs.randn(n, na) * 3).astype(np.float32)
    mk = (rs.rand(n, na) < 0.3).astype(np.uint8)
    mk[:, [0, na - 1]] = rs.rand(n, 2) < 0.5                    # often at the very ends of the row (lane 0 / the last lane)
    mk[:, na // 2] = 1
    mk[:, na // 2 + 1] = 1
    zero, other = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r in range(n):
        legal = np.flatnonzero(mk[r])
        k, nxt = (legal[-1], legal[-2]) if where == "last" else (legal[0], legal[1])
        lg[r, nxt] = lg[r, legal].max() + np.float32(1.0)     # the neighbour holds the maximum: its probability >= 1 / #legal
        lg[r, k] = np.float32(lg[r, nxt] - 110.0)
        zero[r], other[r] = k, nxt
    return lg, mk, zero, other
