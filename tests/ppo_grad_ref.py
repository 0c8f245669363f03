"""An independent float64 restatement of the PPO gradient (the clipped-surrogate head of csrc/azul_learner.hpp, OBJ = 1) and the
table of cases that tests/test_ppo_grad_ref.py, tests/test_gpu_ppo_grad.py and tests/test_hostcheck_ppo.py run through
azul_ppo_gradients.  Plain numpy on the CPU: no project code is imported here; the builders of tests/a2c_grad_ref.py (exact hidden
layer, kink margin, returns 1 to 6 away from the value, mask / softmax edges, the device-count path with its NaN poison row) are reused.

    forward as in tests/a2c_grad_ref.py:  v, logits;  logp = masked log-softmax, p = softmax over the legal actions
    r      = exp(logp[a] - old_logp)                Adv: an input (detached by construction)
    clipped = (Adv > 0 and r > 1 + eps) or (Adv < 0 and r < 1 - eps)
    L_pi   = -min(r Adv, clamp(r, 1 - eps, 1 + eps) Adv)        H = -sum_k p_k logp_k
    L_i    = (L_pi + c_v (q - v)^2 - c_e H) inv_n
    dL/dv       = -2 c_v (q - v) inv_n
    dLogits_k   = (g_a ([k == a] - p_k) + c_e p_k (logp_k + H)) inv_n,   g_a = clipped ? 0 : -Adv r     (legal k; 0 otherwise)
    the rest of the backward pass as there.  Sums: sum L_pi, sum (q - v)^2, sum H, count.

N, the per-element sum of absolute terms (that file's convention): the same backward pass on absolute values with
(|Adv r| ([k == a] + p_k) + c_e p_k (|logp_k| + |H|)) inv_n for dLogits (the unclipped magnitude also where the sample is clipped:
the bound never shrinks because of a decision) and 2 c_v |q - v| inv_n for dL/dv.

Every used sample of every case keeps |r - (1 +- eps)| >= R_MARGIN in float64: the f32 ratio carries about 1e-6 of relative error
from logp and the device exp, so no sample can land on the other side of a bound, where the difference would be O(1).  Samples closer
than that are redrawn when the case is built, never filtered at test time."""
import collections

import numpy as np

from tests import a2c_grad_ref as A2C

SHAPES, HID, ULP, POISON_ROW = A2C.SHAPES, A2C.HID, A2C.ULP, A2C.POISON_ROW
samples_per_pass, flat_size, offsets, normalised_error, k_case = A2C.samples_per_pass, A2C.flat_size, A2C.offsets, A2C.normalised_error, A2C.k_case
R_MARGIN = 1e-3
EPS, C_V, C_E = 0.2, 0.5, 0.01           # the defaults of the cases (PPOLearner's)


def _used(mask, index, count):
    """(source rows of the samples used, their positions in launch order, the count)."""
    if index is not None:
        cnt = len(index) if count is None else int(count)
        rows = np.asarray(index[:cnt], dtype=np.int64)
    else:
        cnt = mask.shape[0] if count is None else int(count)
        rows = np.arange(cnt, dtype=np.int64)
    live = (mask[rows] != 0).any(axis=1) if len(rows) else np.zeros(0, bool)
    return rows[live], np.nonzero(live)[0], cnt


def surrogate(dt, r, Adv, eps):
    """The clipped surrogate of one sample from its ratio: (L_pi, g_a = dL_pi/dlogp[a], clipped).  On a bound (r == 1 +- eps) and with
    Adv == 0 the sample is NOT clipped: the comparisons are strict."""
    lo, hi = dt(1) - dt(eps), dt(1) + dt(eps)
    clipped = ((Adv > 0) & (r > hi)) | ((Adv < 0) & (r < lo))
    L_pi = -np.minimum(r * Adv, np.minimum(np.maximum(r, lo), hi) * Adv)
    return L_pi, np.where(clipped, dt(0), -Adv * r), clipped


def _evaluate(dt, shape, w, obs, mask, action, q, old_logp, adv, eps, cv, ce, index, count, inv_n):
    IN, A = shape
    rows, pos, cnt = _used(mask, index, count)
    inv_n = dt(1.0 / max(cnt, 1) if inv_n is None else inv_n)
    eps, cv, ce = dt(eps), dt(cv), dt(ce)
    n = len(rows)
    x = obs[rows].astype(dt)
    legal = mask[rows] != 0
    act = np.asarray(action)[rows].astype(np.int64)
    qv = np.asarray(q)[rows].astype(dt)
    old = np.asarray(old_logp)[rows].astype(dt)
    Adv = np.asarray(adv)[rows].astype(dt)
    one = np.ones((n, 1), dt)
    X1 = np.concatenate([x, one], axis=1)
    W1 = np.concatenate([w["w1t"].astype(dt), w["b1"].astype(dt)[None]], axis=0)
    w2c, w2a_t = w["w2c"].astype(dt), w["w2a_t"].astype(dt)
    pre = X1 @ W1
    on = pre > 0
    H_ = np.where(on, pre, dt(0))
    v = H_[:, :HID] @ w2c + w["b2c"].astype(dt)[0]
    H1 = np.concatenate([H_[:, HID:], one], axis=1)
    logits = H1 @ np.concatenate([w2a_t, w["b2a"].astype(dt)[None]], axis=0)
    assert legal[np.arange(n), act].all(), "the chosen action of a used sample must be legal"
    m = np.where(legal, logits, -np.inf).max(axis=1, keepdims=True) if n else np.zeros((0, 1), dt)
    z = np.where(legal, logits - m, dt(0))
    e = np.where(legal, np.exp(z), dt(0))
    S = e.sum(axis=1, keepdims=True)
    logp = np.where(legal, z - np.log(S), dt(0))
    p = e / S
    lpa = logp[np.arange(n), act]
    r = np.exp(lpa - old)
    L_pi, ga, clipped = surrogate(dt, r, Adv, eps)
    ent = -(p * logp).sum(axis=1)
    hot = np.zeros((n, A), dt)
    hot[np.arange(n), act] = 1
    dlog = np.where(legal, (ga[:, None] * (hot - p) + ce * p * (logp + ent[:, None])) * inv_n, dt(0))
    td = qv - v
    dv = -dt(2) * cv * td * inv_n
    dZ = np.concatenate([dv[:, None] * w2c[None], dlog @ w2a_t.T], axis=1) * on
    flat = np.zeros(flat_size(IN, A), dt)
    o = offsets(IN, A)

    def put(vec, dW1_, dw2c_, db2c_, dW2_):
        vec[:o["b1"][0] + 360] = dW1_.reshape(-1)
        vec[o["w2c"][0]:o["w2c"][0] + HID] = dw2c_
        vec[o["b2c"][0]] = db2c_
        vec[o["w2a_t"][0]:] = dW2_.reshape(-1)

    put(flat, X1.T @ dZ, H_[:, :HID].T @ dv, dv.sum(), H1.T @ dlog)
    sums = np.array([L_pi.sum(), (td * td).sum(), ent.sum(), n], dt)
    # the sum of absolute terms
    Nlog = np.where(legal, (np.abs(Adv * r)[:, None] * (hot + p) + ce * p * (np.abs(logp) + np.abs(ent)[:, None])) * inv_n, dt(0))
    Ndv = dt(2) * cv * np.abs(td) * inv_n
    NdZ = np.concatenate([Ndv[:, None] * np.abs(w2c)[None], Nlog @ np.abs(w2a_t).T], axis=1) * on
    N = np.zeros(flat_size(IN, A), dt)
    put(N, np.abs(X1).T @ NdZ, H_[:, :HID].T @ Ndv, Ndv.sum(), H1.T @ Nlog)
    logp_out = np.full(cnt, np.nan, dt)           # launch order; NaN: the position carries no sample (nothing is written there)
    logp_out[pos] = lpa
    return {"flat": flat, "sums": sums, "N": N, "logp": logp_out, "ratio": r, "clipped": clipped, "adv": Adv,
            "margin": float(np.abs(pre).min()) if n else float("inf")}


def reference(shape, weights, obs, mask, action, q, old_logp, adv, eps, cv, ce, index=None, count=None, inv_n=None):
    """float64: {"flat", "sums" (four), "N", "logp" (per launch position, NaN without a sample), "ratio", "clipped", "adv", "margin"}."""
    return _evaluate(np.float64, shape, weights, obs, mask, action, q, old_logp, adv, eps, cv, ce, index, count, inv_n)


def reference_f32(shape, weights, obs, mask, action, q, old_logp, adv, eps, cv, ce, index=None, count=None, inv_n=None):
    """The same formulas in numpy float32: the yardstick of the tolerance (what plain f32 arithmetic loses), not a second reference."""
    with np.errstate(all="ignore"):
        return _evaluate(np.float32, shape, weights, obs, mask, action, q, old_logp, adv, eps, cv, ce, index, count, inv_n)


def call_args(c, **over):
    d = dict(c, **over)
    return (d["obs"], d["mask"], d["action"], d["q"], d["old_logp"], d["adv"], d["eps"], d["cv"], d["ce"], d["index"], d["count"], d["inv_n"])


def yardstick(shape, c, **over):
    """The case's f32 yardstick: the normalised error of reference_f32 against reference (CPU only, never the kernel)."""
    a = call_args(c, **over)
    ref = reference(shape, c["w"], *a)
    return normalised_error(reference_f32(shape, c["w"], *a)["flat"], ref["flat"], ref["N"])[0]


# ---- builders: a case of tests/a2c_grad_ref.py + PPO's inputs ------------------------------------------------------------------------
def logp64(c):
    """float64 logp[a] of every row that has a legal action (NaN elsewhere: poison and dead rows)."""
    ok = (c["mask"] != 0).any(axis=1) & np.isfinite(c["obs"]).all(axis=1)
    out = np.full(c["obs"].shape[0], np.nan)
    logits = A2C.forward64(c["w"], c["obs"][ok])[1]
    legal = c["mask"][ok] != 0
    zz = np.where(legal, logits, -np.inf)
    mx = zz.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.where(legal, np.exp(zz - mx), 0.0).sum(axis=1))
    out[ok] = logits[np.arange(ok.sum()), c["action"][ok]] - lse
    return out


def ratio_margin(c):
    """min over the used samples of the distance of the float64 ratio (from the f32 inputs as stored) to either bound."""
    ref = reference(tuple(c["shape"]), c["w"], *call_args(c))
    if not len(ref["ratio"]):
        return float("inf")
    return float(np.minimum(np.abs(ref["ratio"] - (1.0 + c["eps"])), np.abs(ref["ratio"] - (1.0 - c["eps"]))).min())


def _ppo(base, seed, eps=EPS, cv=C_V, ce=C_E, log_ratio=None, adv=None, **meta):
    """base: a builder of tests/a2c_grad_ref.py.  old_logp = fp64 logp[a] - log_ratio (so r = exp(log_ratio) up to the f32 rounding of
    old_logp), log ratios drawn in (-0.4, 0.4) unless given; advantages ~ 2 N(0, 1) unless given; rows closer than R_MARGIN to a bound
    are redrawn."""
    def build(IN, A):
        c = base(IN, A)
        rs = np.random.RandomState(seed)
        rows = c["obs"].shape[0]
        lp = logp64(c)
        have = np.isfinite(lp)
        lr = rs.uniform(-0.4, 0.4, rows) if log_ratio is None else np.asarray(log_ratio(rs, rows), np.float64)
        for _ in range(64):
            old = np.where(have, lp - lr, 0.0).astype(np.float32)
            r = np.exp(np.where(have, lp - old.astype(np.float64), 0.0))
            near = have & (np.minimum(np.abs(r - (1.0 + eps)), np.abs(r - (1.0 - eps))) < 2.0 * R_MARGIN)
            if not near.any():
                break
            assert log_ratio is None, "a chosen log-ratio sits on a bound"
            lr[near] = rs.uniform(-0.4, 0.4, int(near.sum()))
        else:
            raise AssertionError("could not keep the ratios away from the bounds")
        av = (2.0 * rs.randn(rows)).astype(np.float32) if adv is None else np.asarray(adv(rs, rows), np.float32)
        if c["meta"].get("poison"):
            old[POISON_ROW], av[POISON_ROW] = np.nan, np.nan
        c = dict(c, old_logp=np.ascontiguousarray(old), adv=np.ascontiguousarray(av), eps=float(eps), cv=float(cv), ce=float(ce), shape=(IN, A))
        c["meta"] = dict(c["meta"], **meta)
        assert ratio_margin(c) >= R_MARGIN
        return c
    return build


SPAN_LO, SPAN_HI = 60.0, 85.0


def _span60(rs, d):
    """logit-span-60 for this head: two actions, legal in every row, get the biases +32 and -32, so that the legal logits of every row
    span at least SPAN_LO and at most SPAN_HI whatever the row.  tests/a2c_grad_ref.py's editor multiplies the layer by 15, which gives
    spans far above 100: there p_k = e^-span falls below f32's normal range (2^-126), PPO's gradient of such an action --
    (g_a + c_e (logp_k + H)) p_k, with no 0.1 / |legal| term beside it as in the A2C head -- is a denormal, and no f32 evaluation can hold
    a denormal to a relative bound.  Up to SPAN_HI every term stays normal (e^-85 = 1.2e-37, times |logp_k| ~ 85) and the max-subtraction
    path is exercised as hard: exp arguments near -32 for the bulk of the row and below -64 at its bottom."""
    A = d["A"]
    j1, j2 = 5, A - 3                                        # two different column tiles, the second inside the last one
    d["w"]["b2a"][j1], d["w"]["b2a"][j2] = 32.0, -32.0
    d["mask"][:, [j1, j2]] = 1
    d["meta"]["span"] = (SPAN_LO, SPAN_HI)


CLIP_LOG_RATIOS = (0.5, -0.5, 0.5, -0.5, 0.05, -0.05)          # rows cycle: the four clipped / not clipped corners, then unclipped rows
CLIP_ADV_SIGNS = (1.0, 1.0, -1.0, -1.0, 1.0, -1.0)             # (Adv > 0, r > 1 + eps) clipped, (Adv > 0, r < 1 - eps), (Adv < 0, r > 1 + eps),
                                                               # (Adv < 0, r < 1 - eps) clipped, unclipped of both signs


def _cycle(values):
    return lambda rs, rows: np.array([values[i % len(values)] for i in range(rows)])


def _clip_adv(rs, rows):
    return _cycle(CLIP_ADV_SIGNS)(rs, rows) * (0.5 + 2.0 * rs.rand(rows))


Case = collections.namedtuple("Case", "name build group")
CASES = []
for _name, (_m, _a) in (("1", (0, 1)), ("M-1", (1, -1)), ("M", (1, 0)), ("M+1", (1, 1)), ("2M+1", (2, 1))):
    for _p in (1, 2, 3):
        CASES.append(Case("n=%s-parts%d" % (_name, _p), _ppo(A2C.b_size(_m, _a, _p), 300 + 10 * _m + _a + 100 * _p), "size"))
CASES += [Case(nm, _ppo(A2C._edge(fn, 50 + i), 400 + i), "edge") for i, (nm, fn) in enumerate([
    ("one-legal-random", A2C._one_legal("random")), ("all-legal", A2C._all_legal), ("last-tile-only", A2C._last_tile),
    ("action-last", A2C._action_at(True)), ("equal-max", A2C._equal_max), ("logit-span-60", _span60), ("mask-bytes", A2C._mask_bytes),
    ("dead-rows", A2C._dead_rows(False))])]
for _kind in ("perm", "repeat", "reverse"):
    CASES.append(Case("index-%s-count=M-1" % _kind, _ppo(A2C.b_count(_kind, 1, -1), 500 + len(_kind)), "count"))
_PLAIN = A2C.b_size(1, 1, 2)                                   # PPO's own cases: n = M + 1 on two parts
CASES += [
    Case("clip-all-four", _ppo(_PLAIN, 601, log_ratio=_cycle(CLIP_LOG_RATIOS), adv=_clip_adv, clip_all_four=True), "ppo"),
    Case("adv-zero", _ppo(_PLAIN, 602, ce=0.0, adv=lambda rs, rows: np.zeros(rows), adv_zero=True), "ppo"),
    Case("ratio-one", _ppo(_PLAIN, 603, ce=0.0, ratio_one=True), "ppo"),
    Case("no-entropy", _ppo(_PLAIN, 604, ce=0.0), "ppo"),
    Case("no-value", _ppo(_PLAIN, 605, cv=0.0, no_value=True), "ppo"),
    Case("eps-huge", _ppo(_PLAIN, 606, eps=1e30, log_ratio=_cycle((0.5, -0.5)), eps_huge=True), "ppo"),
]
BY_NAME = {c.name: c for c in CASES}


def all_params():
    return [(s, c.name) for s in SHAPES for c in CASES]


def build(shape_name, case_name):
    return BY_NAME[case_name].build(*SHAPES[shape_name])


def critic_elements(IN, A):
    """bool [flat]: dw2c, db2c and the critic half (hidden columns 0..179) of dw1t / db1."""
    o = offsets(IN, A)
    sel = np.zeros(flat_size(IN, A), bool)
    sel[:o["b1"][0]].reshape(IN, 360)[:, :HID] = True
    sel[o["b1"][0]:o["b1"][0] + HID] = True
    sel[o["w2c"][0]:o["b2c"][0] + 1] = True
    return sel


def actor_elements(IN, A):
    """bool [flat]: dw2a_t, db2a and the actor half (hidden columns 180..359) of dw1t / db1."""
    o = offsets(IN, A)
    sel = np.zeros(flat_size(IN, A), bool)
    sel[:o["b1"][0]].reshape(IN, 360)[:, HID:] = True
    sel[o["b1"][0] + HID:o["w2c"][0]] = True
    sel[o["w2a_t"][0]:] = True
    return sel


# the subset the lockstep emulation runs (tests/test_hostcheck_ppo.py on "ref" and "p4_d9")
EMULATION_CASES = ("n=M+1-parts1", "n=M+1-parts2", "clip-all-four", "one-legal-random", "index-perm-count=M-1")
