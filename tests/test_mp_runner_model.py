"""The P-player GameRunner model (tests/mp_runner_model.py, composed from oracle primitives) against the reference itself.

  * P = 3, 4: tests/golden/runner_players.npz -- the reference's own GameRunner.step / opponent_move / get_state / get_valid_moves and
    RandomAgent on Azul(players=P) (tools/gen_golden_mp_runner.py) -- is replayed move for move: the what-if score vectors, the reward
    derived from them (phi = s[0] - max_{j>0} s[j]: beyond the reference for P > 2), done, the game's fields, move_counter, the next
    observation and mask, and every MT19937 word and index.
  * P = 2: the model equals the oracle's GameRunner (oz_runner_init / _reset / _step: game_runner.py:23-85, pinned to the reference by
    tests/golden/traj_*.npz) move for move, reward included -- phi IS the reference's shaped reward there."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests.mp_runner_model import MPRunner, OK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_players.npz")


def model_fields(m):
    g = m.g
    P = m.P
    pl = np.zeros((4, 25), np.int64)
    pl[:P] = np.ctypeslib.as_array(g.pattern_lines)[:P].reshape(P, 25)
    wl = np.zeros((4, 25), np.int64)
    wl[:P] = np.ctypeslib.as_array(g.walls)[:P].reshape(P, 25)
    fl, sc = np.zeros(4, np.int64), np.zeros(4, np.int64)
    fl[:P] = np.ctypeslib.as_array(g.floors)[:P]
    sc[:P] = np.ctypeslib.as_array(g.score)[:P]
    box = np.ctypeslib.as_array(g.box) if m.pool == oz.POOL_LID else np.zeros(5, np.int64)
    lid = np.ctypeslib.as_array(g.lid) if m.pool == oz.POOL_LID else np.zeros(5, np.int64)
    return np.concatenate([np.ctypeslib.as_array(g.displays).reshape(25), np.ctypeslib.as_array(g.center), pl.reshape(-1), wl.reshape(-1), fl, sc,
                           box, lid, [g.current_player, g.next_first_player, g.turn_counter]]).astype(np.int64)


def parse_key(key):
    p, f, pool, _ = key.split("_")
    P = int(p[1:])
    first = oz.FIRST_RANDOM if f == "fRandom" else int(f[1:])
    return P, first, oz.POOL_LID if pool == "lid" else oz.POOL_RANDOM


def _keys():
    return [str(k) for k in np.load(GOLDEN)["keys"]]


@pytest.mark.parametrize("key", _keys())
def test_model_replays_the_reference_gamerunner(key):
    z = np.load(GOLDEN)
    f = lambda name: z[key + "__" + name]
    P, first, pool = parse_key(key)
    r = oz.Rng()
    oz.lib().oz_rng_set(C.byref(r), np.ascontiguousarray(f("mt0"), np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), int(f("pos0")))
    m = MPRunner(P, first, pool, rng=r)
    assert m.runner_init() == OK                                          # GameRunner.__init__
    assert np.array_equal(model_fields(m), f("init_fields"))
    assert np.array_equal(m.obs(0), f("init_obs")) and np.array_equal(m.mask(), f("init_mask"))
    assert m.reset() == OK                                                # reset(): the opening replies
    assert np.array_equal(model_fields(m), f("reset_fields"))
    assert np.array_equal(m.obs(0), f("reset_obs")) and np.array_equal(m.mask(), f("reset_mask"))
    mt, pos = m.rng_state()
    assert np.array_equal(mt, f("reset_mt")) and pos == int(f("reset_pos"))
    phi_prev, episodes = 0, 0
    for t, a in enumerate(f("action")):
        st, rew, dn = m.step(int(a))
        assert st == OK, (t, st)
        s = f("whatif")[t][:P]
        assert m.whatif_scores() == [int(x) for x in s], t
        assert int(f("reward")[t]) == int(s[0] - s[1]) - (0 if t == 0 or f("done")[t - 1] else int(f("whatif")[t - 1][0] - f("whatif")[t - 1][1]))
        phi = int(s[0] - max(s[1:]))
        assert rew == phi - phi_prev, t                                   # beyond the reference for P > 2: the margin over the best opponent
        phi_prev = phi
        assert dn == int(f("done")[t]), t
        assert np.array_equal(model_fields(m), f("fields")[t]), t
        assert m.moves == int(f("move_counter")[t]), t
        if dn:
            episodes += 1
            assert m.reset() == OK
            phi_prev = 0
        assert np.array_equal(m.obs(0), f("obs")[t]), t
        assert np.array_equal(m.mask(), f("mask")[t]), t
        mt, pos = m.rng_state()
        assert pos == int(f("pos")[t]) and np.array_equal(mt, f("mt")[t]), t
    assert episodes >= 1, "the stream should cross at least one reset"


@pytest.mark.parametrize("first,pool", [(oz.FIRST_RANDOM, oz.POOL_LID), (1, oz.POOL_RANDOM), (2, oz.POOL_LID)])
def test_model_at_two_players_is_the_oracle_gamerunner(first, pool):
    L = oz.lib()
    for seed in range(5):
        q, rq = oz.Runner(), oz.seeded_rng(500 + seed)
        m = MPRunner(2, first, pool, seed=500 + seed)
        assert L.oz_runner_init(C.byref(q), first, pool, C.byref(rq)) == m.runner_init() == OK
        assert L.oz_runner_reset(C.byref(q), C.byref(rq)) == m.reset() == OK
        pick = random.Random(seed)
        for t in range(300):
            legal = np.flatnonzero(m.mask())
            a = int(pick.choice(list(legal)))
            rew, dn = C.c_int64(), C.c_int()
            st_q = L.oz_runner_step(C.byref(q), a, C.byref(rq), C.byref(rew), C.byref(dn))
            st, r, d = m.step(a)
            assert (st, r, d) == (st_q, rew.value, dn.value), (seed, t)
            assert bytes(m.g) == bytes(q.game) and m.phi == q.player_score and m.moves == q.move_counter, (seed, t)
            assert m.rng_state()[1] == rq.idx and np.array_equal(m.rng_state()[0], np.ctypeslib.as_array(rq.mt))
            if d:
                assert L.oz_runner_reset(C.byref(q), C.byref(rq)) == m.reset()
