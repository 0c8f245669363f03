"""The P-player GameRunner model with an external opponent (tests/mp_net_model.py, composed from oracle primitives) against the reference.

tests/golden/runner_players_net.npz is the reference's own GameRunner on Azul(players=3|4) with opponent = the reference's Agent on an
ActorCritic(obs_size, 180) (tools/gen_golden_mp_net_opponent.py).  The model, fed the recorded answers, must hand the opponent exactly what
the reference handed it on every call -- the mover-perspective get_state (order = [p] + the others), the legal mask and the player moved
for, at the same move_counter -- and reproduce every agent step: the what-if score vector and the reward derived from it (phi = s[0] -
max_{j>0} s[j], beyond the reference for P > 2), done, the game's fields, move_counter, the next get_state(0) / mask and every MT19937 word."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as oz
from tests.mp_net_model import OK, MPNetRunner
from tests.test_mp_runner_model import parse_key

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_players_net.npz")


def fields_of(g, P, pool):
    pl = np.zeros((4, 25), np.int64)
    pl[:P] = np.ctypeslib.as_array(g.pattern_lines)[:P].reshape(P, 25)
    wl = np.zeros((4, 25), np.int64)
    wl[:P] = np.ctypeslib.as_array(g.walls)[:P].reshape(P, 25)
    fl, sc = np.zeros(4, np.int64), np.zeros(4, np.int64)
    fl[:P] = np.ctypeslib.as_array(g.floors)[:P]
    sc[:P] = np.ctypeslib.as_array(g.score)[:P]
    box = np.ctypeslib.as_array(g.box) if pool == oz.POOL_LID else np.zeros(5, np.int64)
    lid = np.ctypeslib.as_array(g.lid) if pool == oz.POOL_LID else np.zeros(5, np.int64)
    return np.concatenate([np.ctypeslib.as_array(g.displays).reshape(25), np.ctypeslib.as_array(g.center), pl.reshape(-1), wl.reshape(-1), fl, sc,
                           box, lid, [g.current_player, g.next_first_player, g.turn_counter]]).astype(np.int64)


def _keys():
    return [str(k) for k in np.load(GOLDEN)["keys"]]


class Calls:
    """The recorded opponent calls, answered in order; every call's view is checked against the reference's."""

    def __init__(self, f, model):
        self.f, self.m, self.i = f, model, 0

    def answer(self, obs, mask, player):
        f, i = self.f, self.i
        assert i < len(f("call_answer")), "more opponent calls than the reference made"
        assert np.array_equal(obs, f("call_state")[i].astype(np.float32)), ("state", i)
        assert np.array_equal(mask, f("call_mask")[i]), ("mask", i)
        assert player == int(f("call_player")[i]), ("player", i)
        assert self.m.moves == int(f("call_moves")[i]), ("move_counter", i)
        self.i += 1
        return int(f("call_answer")[i])


@pytest.mark.parametrize("key", _keys())
def test_model_replays_the_reference_with_a_network_opponent(key):
    z = np.load(GOLDEN)
    f = lambda name: z[key + "__" + name]
    P, first, pool = parse_key(key)
    r = oz.Rng()
    oz.lib().oz_rng_set(C.byref(r), np.ascontiguousarray(f("mt0"), np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), int(f("pos0")))
    m = MPNetRunner(P, first, pool, rng=r)
    calls = Calls(f, m)
    assert m.runner_init() == OK                                          # GameRunner.__init__
    assert m.reset_with(calls.answer) == OK                               # reset(): the opening moves, answered by the net
    assert calls.i == int((f("call_step") == -1).sum())
    phi_prev, episodes = 0, 0
    for t, a in enumerate(f("action")):
        n0 = calls.i
        st, rew, dn, replies = m.step_with(int(a), calls.answer)
        assert st == OK, (t, st)
        assert calls.i - n0 == int((f("call_step") == t).sum()), t       # this step's calls, opening of the next episode included
        s = f("whatif")[t][:P]
        phi = int(s[0] - max(s[1:]))
        assert rew == phi - phi_prev, t                                   # beyond the reference for P > 2: the margin over the best opponent
        phi_prev = phi
        assert dn == int(f("done")[t]), t
        assert np.array_equal(fields_of(m.closed_game, P, pool), f("fields")[t]), t
        if dn:
            episodes += 1
            phi_prev = 0
        else:
            assert m.moves == int(f("move_counter")[t]), t
        assert np.array_equal(m.obs(0), f("obs")[t]), t
        assert np.array_equal(m.mask(), f("mask")[t]), t
        mt, pos = m.rng_state()
        assert pos == int(f("pos")[t]) and np.array_equal(mt, f("mt")[t]), t
    assert calls.i == len(f("call_answer"))
    assert episodes >= 1, "the stream should cross at least one reset"


def test_fixture_covers_forced_moves_of_the_agents_seat():
    """The agent's own moves with fewer than two legal actions are the opponent's too (game_runner.py:46): the fixture holds some."""
    z = np.load(GOLDEN)
    assert sum(int((z[k + "__call_player"] == 1).sum()) for k in _keys()) > 0

