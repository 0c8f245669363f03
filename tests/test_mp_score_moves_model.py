"""The host model of azul_batch_mp_score_moves (tests/mp_score_moves_model.py) against independent statements, on CPU: at perspective 0 the
table is MPRunner.potential() of the moved game (tests/mp_runner_model.py, the model of the wide runner's reward); a move leaves every
other seat's what-if score alone (what lets the kernel price only the mover per candidate); the census of the shared states holds every
edge class in every shape that can reach it; and the mode checks of PolicyRollout(opponent="greedy_margin"), without a device."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr
from tests import mp_score_moves_model as mm
from tests.mp_runner_model import MPRunner

IDS = [mm.shape_id(s) for s in mm.SHAPES]
# what the census must find at least, per shape: measured far above these on the stream states alone (`tie` over 200 times)
MIN_COUNT = 3


def _game(rec, shape):
    return dr.Game(np.asarray(rec).view(oz.RECORD_NP_DTYPE).reshape(()), mm.cfg_of(shape))


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_perspective_0_is_the_runners_potential_of_the_moved_game(i):
    shape = mm.SHAPES[i]
    P, ext, pool, first = shape
    tabs, _ = mm.tables(i, 0)
    moves = 0
    for rec, tab in zip(mm.states(i), tabs):
        g = _game(rec, shape)
        assert np.array_equal(tab != mm.ILLEGAL, g.mask())
        for a in np.flatnonzero(g.mask()):
            run = MPRunner(P, first, pool, ext, rng=oz.Rng())
            run.g = mm._moved(g, a)
            assert int(tab[a]) == run.potential(), (a,)
            moves += 1
    assert moves > 1000


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_a_move_leaves_the_other_seats_whatif_scores_alone(i):
    shape = mm.SHAPES[i]
    P = shape[0]
    for rec in mm.states(i):
        g = _game(rec, shape)
        me, base = g.mover(), mm._scores(g.g, P)
        for a in np.flatnonzero(g.mask()):
            s = mm._scores(mm._moved(g, a), P)
            assert [s[j] for j in range(P) if j != me] == [base[j] for j in range(P) if j != me], (a,)


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_table_perspectives_agree_with_each_other(i):
    """At two seats another seat's view is the mover's negated; the mover's perspective is the seat's own; best is np.argmax's."""
    shape = mm.SHAPES[i]
    P = shape[0]
    mover = mm.tables(i, mm.PERSP_MOVER)
    for k, rec in enumerate(mm.states(i)):
        me = _game(rec, shape).mover()
        assert np.array_equal(mm.tables(i, me)[0][k], mover[0][k]) and mm.tables(i, me)[1][k] == mover[1][k]
        legal = mover[0][k] != mm.ILLEGAL
        if P == 2:
            assert np.array_equal(mm.tables(i, 1 - me)[0][k][legal], -mover[0][k][legal])
        assert mover[1][k] == (int(np.argmax(mover[0][k])) if legal.any() else -1)


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_census_every_reachable_class_is_in_the_shared_states(i):
    shape = mm.SHAPES[i]
    per, stream, domain = mm.census(i)
    assert len(per) == mm.N_STATES
    out = mm.unreachable(shape)
    assert out <= set(mm.CLASSES)
    for k in mm.CLASSES:
        total = stream[k] + domain[k]
        if k in out:
            assert total == 0, (k, "listed as unreachable, yet found")
        else:
            assert total >= MIN_COUNT, (k, stream[k], domain[k])
    assert stream["tie"] >= 200
    assert per[-1]["none_legal"] == 1                                       # the game before its first round
    assert _game(mm.states(i)[-1], shape).g.current_player == 0 and _game(mm.states(i)[-1], shape).mover() == shape[0] - 1
    assert any(per[k]["none_legal"] for k in range(mm.N_STREAM))            # ended games of the streams
    if "best_high" not in out:
        assert stream["best_high"] >= MIN_COUNT and domain["best_high"] >= 1


# ---- PolicyRollout(opponent="greedy_margin"): the mode checks, without a device ------------------------------------------------------------
def _modes(players=3, rules=None, hidden=180, **kw):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    rules = {"first_player": "Random", "tile_pool": "Lid"} if rules is None else rules
    args = dict(n_games=8, parts=1, rules=rules, window=8, use_graph=True, fused_head=True, opponent="greedy_margin", fused_mlp=True,
                persistent=False, action_selection="Distribution", ring=1, opponent_selection="Distribution", opponent_trace=0, move_limit=0,
                players=players, fused_wide=False, fused_opponent=False, wide_ring=1)
    n_obs, n_act = batch_shape(players, rules)
    ro = PolicyRollout.__new__(PolicyRollout)              # the checks alone: no device, no library call
    ro._check_modes(BatchedActorCritic(n_obs, n_act, hidden), **{**args, **kw})
    return ro


@pytest.mark.parametrize("players,rules", [(3, None), (4, {"first_player": 1, "tile_pool": "Random", "displays": "2P+1"}),
                                           (2, {"first_player": "Random", "tile_pool": "Lid", "bonuses": "end"})])
def test_check_modes_admits_greedy_margin_on_the_per_cut_path(players, rules):
    for persistent in (False, True):
        ro = _modes(players, rules, hidden=64, persistent=persistent, opponent_trace=5)
        assert ro.opponent == "greedy_margin" and ro.scripted and ro.cut and ro.wide and ro.opp_policy is None
        assert not ro.fused_wide and not ro.fused_opponent and not ro.fused_greedy and not ro.persistent and not ro.use_graph
        assert ro.ring == 1 and ro.opp_slots == 5 and ro._persp() == 0


def test_greedy_margin_refusals_come_before_any_allocation():
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    # through the constructor itself: a refusal must not need a device
    with pytest.raises(ValueError, match="opponent=\"greedy\""):
        PolicyRollout(BatchedActorCritic(136, 180, 180), n_games=8, opponent="greedy_margin")
    for kw in ({"fused_wide": True}, {"fused_opponent": True}, {"fused_wide": True, "fused_opponent": True}):
        with pytest.raises(ValueError, match="greedy_margin.*per-cut path"):
            PolicyRollout(BatchedActorCritic(188, 180, 180), n_games=8, opponent="greedy_margin", players=3, **kw)
    # opponent="greedy" on a wide batch keeps its refusal, and now names the wide twin
    with pytest.raises(ValueError, match="two-player reference batches only.*greedy_margin"):
        PolicyRollout(BatchedActorCritic(188, 180, 180), n_games=8, opponent="greedy", players=3)
    with pytest.raises(ValueError, match="no move limit"):
        PolicyRollout(BatchedActorCritic(188, 180, 180), n_games=8, opponent="greedy_margin", players=3, move_limit=30)
