"""CPU: the float64 reference of the A2C gradient (tests/a2c_grad_ref.py) on its own -- against torch float64 autograd of the loss
of agent.py:39-62 written out here, against the loss terms of the golden Agent.update; the preconditions every case of the table
promises; negative controls (each structural error a kernel could make breaks the per-element bound by a wide factor); and the f32
yardstick of every case, from which the GPU test's K_case follows (LABNOTES.md holds the table)."""
import os

import numpy as np
import pytest
import torch

from tests import a2c_grad_ref as R

PARAMS = R.all_params()
IDS = ["%s-%s" % p for p in PARAMS]
WIDE_FACTOR = 100.0          # a negative control must miss the bound by at least this factor


def _autograd(shape, w, obs, mask, action, q, n_total):
    """agent.py:39-62 in torch float64: value and masked log-probabilities, adv = q - v (not detached), actor = -logp[a] adv,
    critic = adv^2 (half of it in the loss), entropy term = -mean of the legal log-probabilities; means over n_total."""
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    x = torch.tensor(obs, dtype=torch.float64)
    legal = torch.tensor(mask != 0)
    h = torch.relu(x @ t["w1t"] + t["b1"])
    value = h[:, :180] @ t["w2c"] + t["b2c"]
    logp = torch.log_softmax((h[:, 180:] @ t["w2a_t"] + t["b2a"]).masked_fill(~legal, float("-inf")), dim=1)
    lpa = logp[torch.arange(len(obs)), torch.tensor(action.astype(np.int64))]
    ent = -(torch.where(legal, logp, torch.zeros_like(logp)).sum(1) / legal.sum(1))
    adv = torch.tensor(q, dtype=torch.float64) - value
    actor, critic, entropy = (-lpa * adv).sum(), (adv ** 2).sum(), ent.sum()
    ((1.0 * actor + 0.5 * critic + 0.1 * entropy) / n_total).backward()
    IN, A = shape
    flat = np.zeros(R.flat_size(IN, A))
    for k, (o, shp) in R.offsets(IN, A).items():
        if k != "pad":
            flat[o:o + int(np.prod(shp))] = t[k].grad.numpy().reshape(-1)
    return flat, np.array([float(actor.detach()), float(critic.detach()), float(entropy.detach())])


@pytest.mark.parametrize("shape_name", ["ref", "p4_d9"])
@pytest.mark.parametrize("n,seed", [(1, 0), (19, 1), (70, 2)])
def test_reference_matches_float64_autograd(shape_name, n, seed):
    shape = IN, A = R.SHAPES[shape_name]
    rs = np.random.RandomState(seed)
    w = R.make_weights(IN, A, 77 + seed)
    obs = R.clear_rows(w, IN, n, rs)
    mask, act = R.random_mask(rs, n, A)
    q = (rs.randn(n) * 5).astype(np.float32)
    flat, sums, N, margin = R.reference(shape, w, obs, mask, act, q)
    want, wsums = _autograd(shape, w, obs, mask, act, q, n)
    assert margin >= R.MARGIN
    assert (np.abs(flat - want) <= 1e-10 * N).all(), float((np.abs(flat - want) / np.maximum(N, 1e-300)).max())
    assert np.allclose(sums[:3], wsums, rtol=1e-10, atol=0) and sums[3] == n
    assert (N >= np.abs(flat)).all() and flat[R.offsets(IN, A)["pad"][0]] == 0.0
    # rows without a legal action carry no sample but stay in the divisor; a selection through `index` is the same samples
    big = [np.concatenate([a, a[:1], a[:1]]) for a in (obs, mask, act, q)]
    big[1][-2:] = 0
    f2 = R.reference(shape, w, *big)[0]
    assert (np.abs(f2 * (n + 2) / n - flat) <= 1e-12 * N).all()
    perm = rs.permutation(n)
    f3, s3, _, _ = R.reference(shape, w, obs, mask, act, q, index=np.concatenate([perm, [0, 0]]).astype(np.int32), count=n)
    assert (np.abs(f3 - flat) <= 1e-12 * N).all() and s3[3] == n


def test_reference_matches_the_golden_agent_update_loss_terms(golden_dir):
    g = np.load(os.path.join(golden_dir, "a2c_update.npz"))
    b = lambda k: g["before_" + k]
    w = {"w1t": np.concatenate([b("critic_linear1.weight"), b("actor_linear1.weight")], axis=0).T, "b1": np.concatenate([b("critic_linear1.bias"), b("actor_linear1.bias")]),
         "w2c": b("critic_linear2.weight")[0], "b2c": b("critic_linear2.bias"), "w2a_t": b("actor_linear2.weight").T, "b2a": b("actor_linear2.bias")}
    w = {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}
    n = g["obs"].shape[0]
    _, sums, _, _ = R.reference((136, 180), w, g["obs"], g["mask"].astype(np.uint8), g["actions"].astype(np.int32), g["qvals"][:, 0].astype(np.float32))
    assert sums[3] == n
    for k, got in zip(("actor_loss", "critic_loss", "entropy_loss"), sums[:3] / n):
        assert np.isclose(got, float(g[k][0]), rtol=2e-5, atol=1e-6), (k, got, float(g[k][0]))


def test_the_table_holds_every_case_of_every_shape():
    assert len(R.SHAPES) == 5 and len(set(c.name for c in R.CASES)) == len(R.CASES)
    for s, (IN, A) in R.SHAPES.items():
        names = [c.name for c in R.cases_for(s)]
        assert ("n=389-parts3" in names) == (s != "ref" and A % 16 != 0)
        assert len(names) == len(R.CASES) - ("n=389-parts3" not in names)


@pytest.mark.parametrize("shape_name,case_name", PARAMS, ids=IDS)
def test_case_preconditions_and_f32_yardstick(shape_name, case_name):
    """What every builder promises (exact n, finite inputs, the kink margin, the logit span, the active straddling units, poison rows
    only past the count, indices in range) and the case's f32 yardstick with the K_case that follows from it."""
    shape = IN, A = R.SHAPES[shape_name]
    M = R.samples_per_pass(IN, A)
    c = R.build(shape_name, case_name)
    c2 = R.build(shape_name, case_name)
    for k in ("obs", "mask", "action", "q", "index"):                    # deterministic builders
        assert (c[k] is None and c2[k] is None) or np.array_equal(c[k], c2[k], equal_nan=True)
    meta, rows = c["meta"], c["obs"].shape[0]
    want_n = {"1": 1, "M-1": M - 1, "M": M, "M+1": M + 1, "2M-1": 2 * M - 1, "2M": 2 * M, "2M+1": 2 * M + 1, "4M+3": 4 * M + 3, "389": 389, "0": 0,
              "6M+9": 6 * M + 9, "7M+9": 7 * M + 9, "8M+9": 8 * M + 9, "16M+9": 16 * M + 9}
    group = R.BY_NAME[case_name].group
    if group == "sweep":
        assert c["n"] == rows == 2 * M + 1 and c["parts"] == 2
    elif group in ("size", "long"):
        assert c["n"] == rows == want_n[case_name[2:].rsplit("-parts", 1)[0]]
        assert c["parts"] == int(case_name.split("parts")[1])
        live = R.REDUCE_EDGE_PARTS.get(case_name[2:].rsplit("-parts", 1)[0])
        if live is not None:                                             # the parts the host entry launches: min(tiles, workspace_parts)
            assert min(c["parts"], -(-c["n"] // M)) == live
    elif group == "edge":
        assert c["n"] == rows == M + 1
    else:
        assert c["n"] == 3 * M == len(c["index"]) and c["count"] == want_n[case_name.split("=")[1]]
    assert c["mask"].shape == (rows, A) and c["obs"].shape == (rows, IN) and c["action"].shape == (rows,) and c["q"].shape == (rows,)
    assert (c["action"] >= 0).all() and (c["action"] < A).all()
    for k in ("w1t", "b1", "w2c", "b2c", "w2a_t", "b2a"):
        assert np.isfinite(c["w"][k]).all()
    used, cnt = R._used(c["mask"], c["index"], c["count"])
    if meta.get("poison"):
        idx = c["index"]
        assert (idx >= 0).all() and (idx < rows).all()
        assert (idx[c["count"]:] == R.POISON_ROW).all() and (idx[:c["count"]] != R.POISON_ROW).all()
        assert np.isnan(c["obs"][R.POISON_ROW]).all() and np.isnan(c["q"][R.POISON_ROW]) and c["action"][R.POISON_ROW] == 0
        assert (c["mask"][R.POISON_ROW] != 0).all()
        keep = np.arange(rows) != R.POISON_ROW
        assert np.isfinite(c["obs"][keep]).all() and np.isfinite(c["q"][keep]).all()
        if "repeat" in case_name and c["count"] >= 2:
            assert len(set(idx[:c["count"]].tolist())) < c["count"]
        if "reverse" in case_name:
            assert (np.diff(idx[:c["count"]]) < 0).all()
    else:
        assert np.isfinite(c["obs"]).all() and np.isfinite(c["q"]).all()
    if len(used):
        pre = R.pre64(c["w"], c["obs"][used])
        assert np.abs(pre).min() >= R.MARGIN >= 1e-3
        assert np.array_equal(c["obs"][used] @ c["w"]["w1t"] + c["w"]["b1"], pre)          # the hidden layer is exact in f32
        v, logits = R.forward64(c["w"], c["obs"][used])
        legal = c["mask"][used] != 0
        assert legal[np.arange(len(used)), c["action"][used]].all()
        if "span" in meta:
            lo, hi = np.where(legal, logits, np.inf).min(1), np.where(legal, logits, -np.inf).max(1)
            assert (hi - lo >= meta["span"]).all()
        if "equal_max" in meta:
            j1, j2 = meta["equal_max"]
            top = np.where(legal, logits, -np.inf).max(1)
            assert legal[:, j1].all() and legal[:, j2].all()
            assert (np.abs(logits[:, j1] - top) <= 1e-12).all() and (np.abs(logits[:, j2] - top) <= 1e-12).all()
        if meta.get("straddle"):
            assert (pre[:, 176:192] > 1e-3).all()
        if meta.get("adv_zero"):
            assert (np.abs(c["q"][used] - v) <= np.abs(v) * 2.0 ** -23 + 1e-30).all()
    if case_name.startswith("one-legal") or case_name == "only-last-action":
        assert ((c["mask"] != 0).sum(1) == 1).all()
        if case_name != "one-legal-random":
            assert (c["action"] == (0 if case_name == "one-legal-first" else A - 1)).all()
    if case_name == "all-legal":
        assert (c["mask"] != 0).all()
    if case_name == "last-tile-only":
        assert not c["mask"][:, :meta["first_legal_column"]].any() and meta["first_legal_column"] == 16 * ((A - 1) // 16)
    if case_name in ("action-0", "action-last"):
        assert (c["action"] == (0 if case_name == "action-0" else A - 1)).all()
    if case_name == "mask-bytes":
        assert set(np.unique(c["mask"]).tolist()) == {0, 1, 2, 0x80, 0xff}
    if case_name == "q-1e4":
        assert (np.abs(c["q"]) == 1e4).all()
    if "dead" in meta:
        assert not c["mask"][meta["dead"]].any() and (c["mask"] != 0).any(1).sum() == rows - len(meta["dead"])
        assert list(meta["dead"]) == (list(range(M)) if case_name == "dead-tile" else [0, M - 1, M])
    # ---- the yardstick (per launch for the sweep) and the condition on K_case
    if group == "sweep":
        ys = []
        for k in range(rows):
            one = dict(c, obs=c["obs"][k:k + 1], mask=c["mask"][k:k + 1], action=c["action"][k:k + 1], q=c["q"][k:k + 1], inv_n=1.0 / rows)
            ys.append(R.yardstick(shape, one))
        y = max(ys)
    else:
        y = R.yardstick(shape, c)
    K = R.k_case(y)
    print("YARDSTICK %s %s %.2f K_case %.1f" % (shape_name, case_name, y, K))
    assert K * R.ULP <= 1e-3, (y, K)


# ---- negative controls: the reference alone, perturbed the way a faulty kernel would be ----------------------------------------------
def _miss(shape, c, got, args=None):
    flat, _, N, _ = R.reference(shape, c["w"], *(args or R.call_args(c)))
    K = R.k_case(R.yardstick(shape, c))
    worst, zeros_ok = R.normalised_error(got, flat, N)
    return worst / K, zeros_ok


@pytest.mark.parametrize("shape_name", ["ref", "p4_d9"])
def test_negative_controls_break_the_bound_by_a_wide_factor(shape_name):
    shape = IN, A = R.SHAPES[shape_name]
    M = R.samples_per_pass(IN, A)
    o = R.offsets(IN, A)
    c = R.build(shape_name, "n=2M+1-parts2")
    n = c["n"]
    for k in (0, M - 1, M, 2 * M):
        # a dropped sample
        m = c["mask"].copy()
        m[k] = 0
        got = R.reference(shape, c["w"], *R.call_args(c, mask=m))[0]
        assert _miss(shape, c, got)[0] > WIDE_FACTOR, ("dropped", k)
        # a doubled sample
        idx = np.concatenate([np.arange(n), [k]]).astype(np.int32)
        got = R.reference(shape, c["w"], c["obs"], c["mask"], c["action"], c["q"], idx, n + 1, 1.0 / n)[0]
        assert _miss(shape, c, got)[0] > WIDE_FACTOR, ("doubled", k)
    # a sample shifted to another row: the position sweep's launch k answered with row k's observation under row k + 1's inputs
    s = R.build(shape_name, "sweep")
    for k in (0, M - 1, M, 2 * M - 1):
        one = dict(s, obs=s["obs"][k:k + 1], mask=s["mask"][k:k + 1], action=s["action"][k:k + 1], q=s["q"][k:k + 1], inv_n=1.0 / s["n"])
        got = R.reference(shape, s["w"], s["obs"][k:k + 1], s["mask"][k + 1:k + 2], s["action"][k + 1:k + 2], s["q"][k + 1:k + 2], inv_n=1.0 / s["n"])[0]
        assert _miss(shape, one, got)[0] > WIDE_FACTOR, ("shifted", k)
        got = R.reference(shape, s["w"], s["obs"][k + 1:k + 2], s["mask"][k + 1:k + 2], s["action"][k + 1:k + 2], s["q"][k + 1:k + 2], inv_n=1.0 / s["n"])[0]
        assert _miss(shape, one, got)[0] > WIDE_FACTOR, ("neighbour", k)
    # one 16x16 block of dw2a_t transposed
    flat = R.reference(shape, c["w"], *R.call_args(c))[0]
    got = flat.copy()
    blk = got[o["w2a_t"][0]:o["b2a"][0]].reshape(180, A)
    blk[16:32, 32:48] = blk[16:32, 32:48].T.copy()
    assert _miss(shape, c, got)[0] > WIDE_FACTOR
    # hidden column 180 (the first actor unit, inside the straddling column tile) zeroed
    t = R.build(shape_name, "straddle")
    got = R.reference(shape, t["w"], *R.call_args(t))[0]
    got[:o["b1"][0]].reshape(IN, 360)[:, 180] = 0.0
    got[o["b1"][0] + 180] = 0.0
    assert _miss(shape, t, got)[0] > WIDE_FACTOR
    # the last action ignored
    a = R.build(shape_name, "action-0")
    a["mask"][:, A - 1] = 1
    m = a["mask"].copy()
    m[:, A - 1] = 0
    got = R.reference(shape, a["w"], *R.call_args(a, mask=m))[0]
    assert _miss(shape, a, got)[0] > WIDE_FACTOR
