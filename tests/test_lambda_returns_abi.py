"""azul_lambda_returns_ring and the gae_lambda / bootstrap_tail switches without a device: the entry is declared, exported and bound; every
argument check of the header returns AZUL_ERR_INVALID before anything is launched; PolicyRollout and BatchedTrainer refuse what the
lambda-return cannot serve with a ValueError before anything is allocated, and resolve the admitted combinations."""
import ctypes as C
import os
import re

import pytest

from tests.test_mp_score_moves_model import _modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "azul_lambda_returns_ring"


def test_the_entry_is_declared_exported_and_bound():
    from azul_deep_reinforcement_learning_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "azul_hip.h")).read()
    decl = re.search(r"int %s\(([^;]*)\);" % ENTRY, header)
    assert decl, "not declared in include/azul_hip.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1).replace("\n", " ")).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["reward_ring_dev", "done_ring_dev", "value_ring_dev", "tail_value_dev", "returns_ring_dev",
                                                         "gamma", "lambda", "ring_steps", "steps_played", "span_steps", "n_games", "stream"]
    assert ENTRY in L.SIGNATURES
    fn = getattr(L.lib, ENTRY)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(args)


def test_argument_checks_need_no_gpu():
    from azul_deep_reinforcement_learning_amd import _lib as L
    fn = L.lib.azul_lambda_returns_ring
    one = C.c_void_p(8)                                        # a non-NULL placeholder; never dereferenced
    f32 = C.c_float
    ok = dict(reward=one, done=one, value=one, tail=None, returns=one, gamma=f32(0.99), lam=f32(0.95), ring=96, played=96, span=96, n=64)
    call = lambda **kw: (lambda a: fn(a["reward"], a["done"], a["value"], a["tail"], a["returns"], a["gamma"], a["lam"], a["ring"], a["played"],
                                      a["span"], a["n"], None))({**ok, **kw})
    refusals = [
        dict(reward=None), dict(done=None), dict(value=None), dict(returns=None),          # a NULL array (the tail alone is optional)
        dict(ring=0), dict(ring=-1, span=-1),                                               # ring_steps >= 1
        dict(span=0), dict(span=97), dict(ring=8, span=9, played=64),                       # 1 <= span_steps <= ring_steps
        dict(played=95), dict(played=0), dict(played=-96),                                  # steps_played >= span_steps
        dict(n=0), dict(n=-4),                                                              # n_games >= 1
        dict(ring=1 << 20, span=1, n=1 << 12),                                              # the slot index is 32 bits wide
        dict(lam=f32(-0.01)), dict(lam=f32(1.0001)), dict(lam=f32(2.0)),                    # 0 <= lambda <= 1
        dict(lam=f32(float("nan"))), dict(lam=f32(float("inf"))), dict(lam=f32(float("-inf"))),
        dict(gamma=f32(float("nan"))), dict(gamma=f32(float("inf"))), dict(gamma=f32(float("-inf"))),
        dict(tail=one, value=None), dict(tail=one, lam=f32(1.5)),
    ]
    for kw in refusals:
        assert call(**kw) == L.ERR_INVALID, kw
        assert L.lib.azul_last_error_string().decode().startswith(ENTRY + ":"), kw
    with pytest.raises(L.AzulHipError, match=ENTRY):
        L.check(call(lam=f32(-1.0)))


def _net(obs=136, act=180, hidden=180):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    return BatchedActorCritic(obs, act, hidden)


def test_rollout_refusals_come_before_any_allocation():
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    two = dict(n_games=8, window=8, opponent="random", persistent=True)
    refusals = [
        (two, {"opponent": None, "gae_lambda": 0.5}, "flat self-play"),                     # another seat's value
        (two, {"opponent": None, "gae_lambda": 0.0}, "flat self-play"),
        (two, {"opponent": None, "bootstrap_tail": True}, "flat self-play"),
        (two, {"opponent": None, "gae_lambda": 1.0, "bootstrap_tail": True}, "flat self-play"),
        (two, {"gae_lambda": -0.1}, r"gae_lambda must lie in \[0, 1\]"),
        (two, {"gae_lambda": 1.5}, r"gae_lambda must lie in \[0, 1\]"),
        (two, {"gae_lambda": float("nan")}, r"gae_lambda must lie in \[0, 1\]"),
        (two, {"opponent": None, "gae_lambda": 7.0}, r"gae_lambda must lie in \[0, 1\]"),
        (two, {"ring": 2, "bootstrap_tail": True}, "bootstrap_tail=True.*ring of 2 windows"),
        (two, {"ring": 3, "bootstrap_tail": True, "gae_lambda": 0.9}, "bootstrap_tail=True.*ring of 3 windows"),
    ]
    wide = dict(n_games=8, window=8, opponent="random", players=3, fused_wide=True)
    refusals += [
        (wide, {"wide_ring": 2, "bootstrap_tail": True}, "bootstrap_tail=True.*ring of 2 windows"),
        (wide, {"opponent": None, "gae_lambda": 0.5}, "flat self-play"),
        (wide, {"opponent": None, "fused_wide": False, "bootstrap_tail": True}, "flat self-play"),
    ]
    for base, kw, match in refusals:
        with pytest.raises(ValueError, match=match):
            PolicyRollout(_net(188 if base is wide else 136), **{**base, **kw})


def test_check_modes_resolves_the_switches():
    two = dict(players=2, opponent="random", persistent=True)
    for kw in ({}, {"gae_lambda": None}, {"gae_lambda": 1.0}, {"gae_lambda": 1}):          # the launches of before
        for ring in (1, 3):
            ro = _modes(**two, ring=ring, **kw)
            assert ro.gae_lambda is None and not ro.bootstrap_tail and ro.ring == ring
    ro = _modes(players=2, opponent=None, persistent=True, gae_lambda=1.0)
    assert ro.gae_lambda is None and ro.opponent is None                                    # flat self-play keeps its Monte-Carlo return
    for lam in (0.0, 0.5, 0.95):
        for ring in (1, 3):
            ro = _modes(**two, ring=ring, gae_lambda=lam)
            assert ro.gae_lambda == lam and not ro.bootstrap_tail and ro.ring == ring and ro.window_entry
    ro = _modes(**two, bootstrap_tail=True)
    assert ro.gae_lambda == 1.0 and ro.bootstrap_tail and ro.ring == 1
    ro = _modes(**two, bootstrap_tail=True, gae_lambda=0.9)
    assert ro.gae_lambda == 0.9 and ro.bootstrap_tail
    # a ring the modes resolve away (no window kernel: the move-by-move path keeps one window) admits the tail
    ro = _modes(players=2, opponent="random", persistent=False, ring=3, bootstrap_tail=True)
    assert ro.ring == 1 and ro.bootstrap_tail and ro.window_entry is None and ro.use_graph
    # every opponent kind with records of one seat, both record families
    for kw in (dict(players=2, opponent="greedy"), dict(players=2, opponent="greedy", fused_opponent=True), dict(players=3),
               dict(players=3, opponent="random", fused_wide=True, wide_ring=2), dict(players=3, fused_wide=True, fused_seats=True),
               dict(players=2, opponent=_net())):
        assert _modes(**kw, gae_lambda=0.5).gae_lambda == 0.5
    assert _modes(players=3, opponent="random", fused_wide=True, bootstrap_tail=True).bootstrap_tail


def test_trainer_refusals_come_before_any_allocation():
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    refusals = [
        ({"gae_lambda": 1.2}, r"gae_lambda must lie in \[0, 1\]"),
        ({"gae_lambda": -1}, r"gae_lambda must lie in \[0, 1\]"),
        ({"opponent": None, "gae_lambda": 0.9}, "opponent other than None"),
        ({"opponent": None, "bootstrap_tail": True, "ring": 1}, "opponent other than None"),
        ({"bootstrap_tail": True}, "bootstrap_tail=True.*ring=1"),                          # the trainer's default ring of three windows
        ({"bootstrap_tail": True, "ring": 2, "gae_lambda": 0.9}, "bootstrap_tail=True.*ring=1"),
    ]
    for kw, match in refusals:
        with pytest.raises(ValueError, match=match):
            BatchedTrainer(_net(), n_games=8, window=8, **kw)
    with pytest.raises(ValueError, match="bootstrap_tail=True.*ring=1"):
        BatchedTrainer(_net(188), n_games=8, window=8, players=3, fused_wide=True, fused_learner=True, ring=2, bootstrap_tail=True)
