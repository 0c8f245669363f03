"""The host model of azul_batch_playout_moves_policy (tests/playout_policy_model.py: include/azul_hip.h's playout under a playout policy,
statement by statement on the oracle) held to the existing models and to cases worked by hand, and the condition of the tests that run
the kernel against it: the states they use hold every class of ply, playout and state.  Plus the refusals of the greedy-playout opponent
that need no device."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr
from tests import playout_moves_model as pm
from tests import playout_policy_model as pp
from tests import score_moves_model as sm

CLASSES = pp.PLY_CLASSES + pp.PLAYOUT_CLASSES + pp.STATE_CLASSES


def test_the_uniform_policy_is_the_existing_model():
    """policy = uniform, explore 0: tests/playout_moves_model.py's tables of the 360 shared states, playout by playout."""
    vals, legal, movers, _ = pp.stream_values(0, pm.KMAX, pp.UNIFORM)
    want_vals, want_legal, want_movers, _ = pm.stream_values()
    assert np.array_equal(vals, want_vals) and np.array_equal(legal, want_legal) and np.array_equal(movers, want_movers)
    for K in (1, 2, 3):
        tabs, best = pp._tables(vals, legal, movers, K, pp.PERSP_CURRENT)
        assert np.array_equal(tabs, pm.stream_tables(K)[0]) and np.array_equal(best, pm.stream_tables(K)[1])


def test_the_greedy_ply_is_greedy_of_game():
    """pp.greedy_ply (one evaluation per legal action, and whether the action order decided) answers what sm.greedy_of_game answers, on every
    shared state, and that is azul_batch_score_moves' `best` of the state."""
    recs = sm.stream_states()[0]
    best = sm.stream_tables(pp.PERSP_CURRENT)[1]
    tied = 0
    for i, r in enumerate(recs):
        game = sm._game(r)
        move, tie = pp.greedy_ply(game)
        assert move == sm.greedy_of_game(game) == best[i], i
        tab = sm.stream_tables(pp.PERSP_CURRENT)[0][i]
        lg = tab[tab != sm.ILLEGAL]
        assert tie == (len(lg) >= 2 and int((lg == lg.max()).sum()) >= 2), i
        tied += int(tie)
    assert 0 < tied < len(recs)


@pytest.mark.parametrize("explore,K", pp.CONFIGS)
def test_the_shared_states_hold_every_class(explore, K):
    """Coverage is a CONDITION of the tests that run the kernel: the emulation and the GPU test run the 360 shared states at these two
    configurations.  Every class at least once; a playout with both an explored and a greedy ply needs draws, so it is asked for where
    explore > 0 only."""
    total = pp.census(explore, K)
    print((explore, K), total)
    for name in CLASSES:
        if name == "explored_and_greedy" and explore == 0:
            assert total[name] == 0
        else:
            assert total[name] >= 1, (name, total)
    assert 1 <= total["longest"] < pp.MAX_PLIES
    _, legal, _, _ = pp.stream_values(explore, K)
    assert total["playouts"] == int(legal.sum()) * K                  # (explore 0, K 1: one playout per legal candidate)


@pytest.mark.parametrize("n", [dr.CPU_N, dr.GPU_N], ids=["emulation", "gpu"])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_the_domain_records_hold_every_class(cfg, n):
    """The same condition for the arbitrary in-domain records (pm.domain_values' batches), per pool, at the configuration the kernel tests
    run them at: (explore 64, K 2); and no playout that the ply bound cuts."""
    explore, K = 64, 2
    total = pp.domain_census(cfg, n, explore, K)
    print(dr.config_id(cfg), n, total)
    for name in CLASSES:
        assert total[name] >= 1, (name, total)
    assert total["longest"] < pp.MAX_PLIES


def _hand(rec, per_playout, best, flipped_best, **kw):
    """`per_playout`: action -> score[0] - score[1] of ONE playout (player 1 moves); every playout of these records gives the same."""
    for K in (1, 3):
        for persp, sign in ((0, 1), (1, -1), (pp.PERSP_CURRENT, 1)):
            tab, b = pp.table(rec, G=77, K=K, perspective=persp, **kw)
            want = np.full(180, pp.ILLEGAL, np.int64)
            for a, v in per_playout.items():
                want[a] = sign * K * v
            assert np.array_equal(tab, want), (K, persp)
            assert b == (best if sign == 1 else flipped_best), (K, persp)


@pytest.mark.parametrize("explore", [0, 64, 255])
def test_the_stuck_and_last_move_records_by_hand(explore):
    """No ply is played in either record (tests/playout_moves_model.py derives their tables by hand), so the policy cannot matter."""
    worst = lambda acts: min(a for a, v in acts.items() if v == min(acts.values()))
    _hand(pm.stuck_record(), pm.STUCK_ACTIONS, pm.STUCK_BEST, worst(pm.STUCK_ACTIONS), explore=explore)
    _hand(pm.last_move_record(), pm.LAST_MOVE_ACTIONS, pm.LAST_MOVE_BEST, worst(pm.LAST_MOVE_ACTIONS), explore=explore)
    for rec in (pm.stuck_record(), pm.last_move_record()):
        assert all(f["plies"] == 0 for f in pp.state_values(rec, 77, 2, explore=explore)[2])


def test_the_crafted_record_with_a_greedy_ply_decided_by_the_action_order_by_hand():
    rec = pp.tie_ply_record()
    _hand(rec, pp.TIE_PLY_ACTIONS, pp.TIE_PLY_BEST, 1)
    vals, legal, facts = pp.state_values(rec, G=77, K=1)
    assert sorted(np.flatnonzero(legal)) == sorted(pp.TIE_PLY_ACTIONS)
    assert len(facts) == 12 and all(f["plies"] == 1 and f["greedy"] == 1 and f["first_of_equals"] == 1 and f["explored"] == 0 for f in facts)
    # the ply itself: after either colour's candidate player 2 answers with the floor row, the first of six equal values
    game = sm._game(rec)
    for a in pp.TIE_PLY_ACTIONS:
        g, (d, c, p) = sm._moved(game, a)
        oz.lib().oz_next_player(C.byref(g))
        assert pp.greedy_ply(g) == (pp.TIE_PLY_REPLY[c], True) and int(oz.check_all_valid(g).sum()) == 6, a
    # no draw decides anything at explore 0: any seed, call and game id give the same table
    assert np.array_equal(pp.table(rec, 1, 2, seed=5, call=9)[0], pp.table(rec, 77, 2)[0])


def test_at_explore_0_k_playouts_are_k_times_one():
    t1, b1 = pp.stream_tables(0, 1)
    t3, b3 = pp.stream_tables(0, 3)
    legal = t1 != pp.ILLEGAL
    assert np.array_equal(t3 != pp.ILLEGAL, legal) and np.array_equal(t3[legal], 3 * t1[legal]) and np.array_equal(b1, b3)
    # ... by the definition, not by the shortcut: three playouts run one by one on a few states
    recs, p0 = sm.stream_states()[0], pp.stream_tables(0, 3, 0)[0]
    for i in (0, 57, 119, 200, 359):
        game = sm._game(recs[i])
        draws = pp._Draws(pp.SEED, pp.CALL, pp.GBASE + i, 3)
        for a in np.flatnonzero(oz.check_all_valid(game)):
            v = [pp.playout(game, int(a), k, draws, pp.GREEDY, 0)[0] for k in range(3)]
            assert v[0] == v[1] == v[2] and sum(v) == int(p0[i, a]), (i, a)
    assert not draws.blocks                                           # no word was read


def test_explore_reads_the_low_byte_and_plays_the_uniform_ordinal_from_the_same_word():
    """A playout at explore 255 whose words' low bytes are all below 255 is the uniform policy's playout; the model at explore 255 and the
    uniform model agree on every such candidate of a few states, and differ somewhere at explore 64."""
    recs = sm.stream_states()[0]
    same = differ = 0
    for i in (5, 130, 250):
        game = sm._game(recs[i])
        draws = pp._Draws(pp.SEED, pp.CALL, pp.GBASE + i, 1)
        for a in np.flatnonzero(oz.check_all_valid(game)):
            u, _ = pm.playout(game, int(a), 0, draws)
            g255, f = pp.playout(game, int(a), 0, draws, pp.GREEDY, 255)
            if f["greedy"] == 0:
                assert g255 == u, (i, a)
                same += 1
            differ += int(pp.playout(game, int(a), 0, draws, pp.GREEDY, 64)[0] != u)
    assert same >= 10 and differ >= 1


def _check(**over):
    from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
    ro = PolicyRollout.__new__(PolicyRollout)
    args = dict(policy=None, n_games=4, parts=1, window=8, use_graph=True, fused_head=True, opponent="playout", fused_mlp=True, persistent=True,
                action_selection="Distribution", ring=3, opponent_selection="Distribution", opponent_trace=0, move_limit=0, fused_wide=False,
                fused_opponent=False, wide_ring=1, rules={"first_player": "Random", "tile_pool": "Lid"}, players=2)
    args.update(over)
    ro._check_modes(**args)
    return ro


def test_greedy_playout_opponent_refusals_need_no_device():
    for bad in ("Greedy", "random", 1, None):
        with pytest.raises(ValueError, match="opponent_playout_policy"):
            _check(opponent_playout_policy=bad)
    for bad in (-1, 256, 1.5, "3", True):
        with pytest.raises(ValueError, match="opponent_playout_explore"):
            _check(opponent_playout_policy="greedy", opponent_playout_explore=bad)
    with pytest.raises(ValueError, match="opponent_playout_explore"):
        _check(opponent_playout_policy="uniform", opponent_playout_explore=1)
    # the other refusals of opponent="playout" are unchanged
    with pytest.raises(ValueError, match="answers per cut"):
        _check(opponent_playout_policy="greedy", fused_opponent=True)
    with pytest.raises(ValueError, match="opponent_playouts"):
        _check(opponent_playout_policy="greedy", opponent_playouts=257)


def test_greedy_playout_opponent_resolves_to_the_per_cut_path():
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    ro = _check(policy=BatchedActorCritic(136, 180, 180), opponent_playouts=1, opponent_playout_policy="greedy", opponent_playout_explore=64)
    assert ro.opponent == "playout" and ro.scripted and ro.cut and ro.opponent_playouts == 1
    assert ro.opponent_playout_policy == "greedy" and ro.opponent_playout_explore == 64
    assert ro.window_entry is None and not ro.persistent and not ro.use_graph and ro.ring == 1
    ro = _check(policy=BatchedActorCritic(136, 180, 180))
    assert ro.opponent_playout_policy == "uniform" and ro.opponent_playout_explore == 0
    # another opponent ignores the two arguments
    ro = _check(policy=BatchedActorCritic(136, 180, 180), opponent="greedy", opponent_playout_policy="greedy", opponent_playout_explore=9)
    assert ro.opponent_playout_policy == "uniform" and ro.opponent_playout_explore == 0
