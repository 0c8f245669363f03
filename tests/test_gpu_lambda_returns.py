"""GPU: the TD(lambda) returns with critic bootstrap.  azul_lambda_returns_ring called directly on device arrays built from the case table
of tests/lambda_returns_cases.py and compared with its host model bit for bit (the library is built without contraction and fast-math: the
float32 recurrence has one result), guard rows and slots outside the span intact, lambda = 1 equal to azul_discounted_returns_ring on the
same buffers.  Then through every rollout path: after each window the whole `returns` buffer equals the model applied to the rollout's
own reward / done / value buffers (and tail_value with bootstrap_tail); without the switch the buffers are the Monte-Carlo scan's, as
before; and BatchedTrainer trains on them, counts every recorded step with bootstrap_tail and resumes bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS, BatchedTrainer
from tests import lambda_returns_cases as M
from tests import training_ring_cases as RC

pytestmark = pytest.mark.gpu

p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
f32 = C.c_float


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_lambda_returns_ring_on_the_case_table(case):
    reward, done, value, tail, ret_in = case.build()
    want = M.lambda_returns_ring(reward, done, value, tail, ret_in, case.gamma, case.lam, case.ring, case.played, case.span)
    r, d, v, t, out = dev(reward), dev(done), dev(value), dev(tail), dev(ret_in)
    L.check(L.lib.azul_lambda_returns_ring(p(r), p(d), p(v), p(t), p(out), f32(case.gamma), f32(case.lam), case.ring, case.played, case.span,
                                           case.N, None))
    torch.cuda.synchronize()
    got = host(out)
    M.compare_returns(case.id, got, want)                    # the span, the slots outside it and the guard rows behind the ring
    keep = np.ones(len(got), bool)
    keep[case.slots()] = False
    M.compare_returns(case.id, got[keep], ret_in[keep], "the rows outside the span and behind the ring")
    assert np.array_equal(host(r), reward) and np.array_equal(host(d), done) and np.array_equal(host(v), value)
    if case.lam == 1.0:
        # nothing flowing in: the Monte-Carlo scan's bits, from both entries on the same buffers
        new, old = dev(ret_in), dev(ret_in)
        L.check(L.lib.azul_lambda_returns_ring(p(r), p(d), p(v), None, p(new), f32(case.gamma), f32(1.0), case.ring, case.played, case.span,
                                               case.N, None))
        L.check(L.lib.azul_discounted_returns_ring(p(r), p(d), p(old), f32(case.gamma), case.ring, case.played, case.span, case.N, None))
        torch.cuda.synchronize()
        M.compare_returns(case.id + " vs azul_discounted_returns_ring", host(new), host(old))


# ---------------------------------------------------------------------------------------------------------------- through the rollouts
T, WINDOWS, GAMMA, LAM = 8, 3, 0.99, 0.5
RULES = {"first_player": "Random", "tile_pool": "Lid"}
# 17 games (one workgroup of the window kernels and one game); the rollout in two parts plays 18 = 2 x 9 (n_games % parts == 0)
ROLLOUTS = {
    "a-persistent-ring1": dict(n_games=17, persistent=True, opponent="random"),
    "b-persistent-ring3": dict(n_games=17, persistent=True, opponent="random", ring=3),
    "c-per-move-two-parts": dict(n_games=18, persistent=False, parts=2, opponent="random"),
    "d-wide-fused-ring2": dict(n_games=17, players=3, fused_wide=True, wide_ring=2, opponent="random"),
    "e-wide-per-move": dict(n_games=17, players=3, opponent="random"),
    "f-bootstrap-tail": dict(n_games=17, persistent=True, opponent="random", bootstrap_tail=True),
}


def _net(kw, seed=3):
    torch.manual_seed(seed)
    return BatchedActorCritic(188 if kw.get("players", 2) == 3 else 136, 180, 180).cuda()


def _rollout(name, **extra):
    kw = ROLLOUTS[name]
    return PolicyRollout(_net(kw), window=T, seed_base=5100, rules=RULES, **kw, **extra)


def _critic_f64(net, obs):
    """forward_critic (model.py:22-26) in float64 numpy."""
    sd = {k: host(v).astype(np.float64) for k, v in net.state_dict().items()}
    h = np.maximum(obs.astype(np.float64) @ sd["critic_linear1.weight"].T + sd["critic_linear1.bias"], 0.0)
    return (h @ sd["critic_linear2.weight"].T + sd["critic_linear2.bias"])[:, 0]


def _play_and_compare(name, ro, lam):
    """Three windows; after each, per part, `returns` of everything the buffers hold against the model on the rollout's own buffers."""
    R = ro.ring * T
    want = [np.zeros((R, ro.h), np.float32) for _ in range(ro.parts)]
    ends = 0
    for w in range(WINDOWS):
        traj = ro.run_window(GAMMA)
        ro.synchronize()
        played = (w + 1) * T if ro.ring > 1 else T
        for part in range(ro.parts):
            rg = ro.rings[part]
            rr, dd, vv = host(rg["reward"]), host(rg["done"]), host(rg["value"])[:, :, 0]
            assert np.isfinite(vv).all(), (name, w, part)
            cid = "%s window %d part %d" % (name, w, part)
            if lam is None:
                want[part] = RC.returns_ring(rr, dd, want[part], GAMMA, R, played, min(R, played))
            else:
                tail = host(traj[part]["tail_value"]) if ro.bootstrap_tail else None
                assert ("tail_value" in traj[part]) == ro.bootstrap_tail
                want[part] = M.lambda_returns_ring(rr, dd, vv, tail, want[part], GAMMA, lam, R, played, min(R, played))
                if ro.bootstrap_tail:
                    assert tail.shape == (ro.h,)
                    ref = _critic_f64(ro.policy, host(traj[part]["obs"][T]))
                    err = float(np.abs(tail.astype(np.float64) - ref).max())
                    print("%s: |tail_value - fp64 critic| max %.3g" % (cid, err))
                    assert err <= 2e-5, cid
            M.compare_returns(cid, host(rg["returns"]), want[part])
            if ro.ring == 1:
                assert traj[part]["returns"].data_ptr() == rg["returns"].data_ptr()
            ends += int((dd != 0).sum())
    assert ends > 0, name                                    # episodes ended inside the windows: both branches of the scan ran
    return want


@pytest.mark.parametrize("name", sorted(ROLLOUTS))
def test_rollout_returns_equal_the_model_on_the_rollouts_own_buffers(name):
    lam = 1.0 if name.startswith("f-") else LAM
    ro = _rollout(name, **({} if name.startswith("f-") else {"gae_lambda": LAM}))
    assert ro.gae_lambda == lam and ro.bootstrap_tail == name.startswith("f-")
    assert {"a": ro.persistent and ro.ring == 1, "b": ro.persistent and ro.ring == 3, "c": ro.window_entry is None and ro.parts == 2 and ro.use_graph,
            "d": ro.fused_wide and ro.ring == 2 and ro.wide, "e": ro.wide and ro.window_entry is None and ro.use_graph,
            "f": ro.persistent and ro.ring == 1}[name[0]], (name, ro.graph_error)
    _play_and_compare(name, ro, lam)
    with pytest.raises(ValueError, match="gae_lambda"):
        ro.run_window(GAMMA, gae_lambda=0.25)


def test_bootstrap_tail_with_a_lambda_below_one():
    ro = _rollout("f-bootstrap-tail", gae_lambda=LAM)
    assert ro.gae_lambda == LAM and ro.bootstrap_tail
    _play_and_compare("f-bootstrap-tail-lambda", ro, LAM)


@pytest.mark.parametrize("name", sorted(n for n in ROLLOUTS if not n.startswith("f-")))
def test_without_the_switch_the_rollouts_keep_the_monte_carlo_returns(name):
    """gae_lambda=None, and an explicit 1.0, run the launches of before: `returns` is the discounted scan of the rollout's own rewards and
    flags (tests/training_ring_cases.returns_ring), chained through a ring where there is one -- and the trajectories are those of the
    rollout with the switch (the scan reads the records, it never touches the games)."""
    plain = _rollout(name)
    one = _rollout(name, gae_lambda=1.0)
    lam = _rollout(name, gae_lambda=LAM)
    assert plain.gae_lambda is None and one.gae_lambda is None and not plain.bootstrap_tail
    for w in range(2):
        for ro in (plain, one, lam):
            ro.run_window(GAMMA)
            ro.synchronize()
        for part in range(plain.parts):
            for k in ("obs", "mask", "action", "reward", "done", "value", "log_prob", "entropy"):
                a, b, c = plain.rings[part][k], one.rings[part][k], lam.rings[part][k]
                assert torch.equal(a, b) and torch.equal(a, c), (name, w, part, k)
            assert torch.equal(plain.rings[part]["returns"].view(torch.int32), one.rings[part]["returns"].view(torch.int32)), (name, w, part)
    _play_and_compare(name, _rollout(name), None)


# ---------------------------------------------------------------------------------------------------------------- the trainer
def _trainer_state(t):
    return ({k: v.detach().cpu().clone() for k, v in t.rollout.policy.state_dict().items()}, t.rollout.envs[0].get_records().tobytes(),
            t.rollout.work[0]["counter"].tolist(), {k: v.detach().cpu().clone() for k, v in t.rollout.rings[0].items()},
            {k: v.detach().cpu().clone() for k, v in t.rollout.traj[0].items()})


@pytest.mark.parametrize("switch", [dict(gae_lambda=0.9), dict(bootstrap_tail=True, ring=1)], ids=["gae_lambda", "bootstrap_tail"])
def test_trainer_trains_on_the_lambda_returns_and_resumes_bit_for_bit(switch, tmp_path):
    kw = dict(n_games=17, window=T, results_dir=str(tmp_path), **switch)
    torch.manual_seed(4)
    tr = BatchedTrainer(BatchedActorCritic(136, 180, 180), seed_base=21, **kw)
    ro = tr.rollout
    tail = bool(switch.get("bootstrap_tail"))
    assert ro.persistent and ro.ring == (1 if tail else 3) and ro.gae_lambda == (1.0 if tail else 0.9) and ro.bootstrap_tail == tail

    def batch(t):
        row = t.run_batch()
        t.rollout.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(row[k]) for k in AGENT_STAT_KEYS[1:]), row
        if tail:                                             # every recorded step that carries an action is a sample, open episodes included
            n = int((t.rollout.traj[0]["action"] >= 0).sum())
            assert n > 0 and float(t.learner.statistics["samples"][-1]) == n
        return row

    batch(tr)
    batch(tr)
    assert tr.learner.updates == 2
    ck = os.path.join(str(tmp_path), "lambda.pt")
    tr.save_checkpoint(ck)
    row_a = batch(tr)
    want = _trainer_state(tr)
    torch.manual_seed(99)
    tr2 = BatchedTrainer(BatchedActorCritic(136, 180, 180), seed_base=9000, **kw)
    tr2.load_checkpoint(ck)
    row_b = batch(tr2)
    got = _trainer_state(tr2)
    assert tr2.batch == 3 and want[1] == got[1] and want[2] == got[2]
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    assert torch.equal(bits(want[3]["returns"]), bits(got[3]["returns"]))          # everything the buffers hold, older windows included
    for k in want[4]:                                                              # the window just played
        assert torch.equal(bits(want[4][k]), bits(got[4][k])), k
    assert ("tail_value" in got[4]) == tail
    # the window just played carries the lambda-returns of its own buffers
    rg = got[3]
    R, played = ro.ring * T, 3 * T if ro.ring > 1 else T
    prev = np.zeros((R, 17), np.float32)
    # (the ring of three windows is full after the third batch: every slot is rewritten, whatever it held)
    model = M.lambda_returns_ring(rg["reward"].numpy(), rg["done"].numpy(), rg["value"].numpy()[:, :, 0],
                                  got[4]["tail_value"].numpy() if tail else None, prev, 0.99, ro.gae_lambda, R, played, R)
    M.compare_returns("trainer " + "/".join(switch), rg["returns"].numpy(), model)
    for k in AGENT_STAT_KEYS[1:]:
        assert row_a[k] == row_b[k], k
