"""The P-player GameRunner with an external opponent on CPU: azx::net_body_x (csrc/azul_rules_x.hpp, the body of azul_x_net_kernel) compiled
UNMODIFIED by g++ and run under the lockstep 64-lane emulation of tests/hostcheck/simt, against the model composed from the oracle
(tests/mp_net_model.py, itself pinned to the reference by tests/test_mp_net_model.py).  After every cut of the protocol (begin / reply /
reset) every output is compared: pending, replies, status, the reward / done written by the launch that closes a step (and nothing written
by any other), the observation from the mover's perspective and the legal mask of every game that owes an opponent_move() (and nothing
written for the others), the owing count, the 256-byte records INCLUDING the runner's tail (bytes 228..231), all 624 MT19937 words and the
index, and the episode / stuck / statistics counters.

  * (3, 5) and (4, 5) under the reference's rules, answered with the fixture's recorded network answers and with random legal answers;
  * (2, 5), (3, 7) and (4, 9) with extended rules, random legal answers;
  * illegal answers (out of range, -1, a masked action) leave the game and the debt as they are;
  * a crafted state in which nobody can move closes the step with done = 2 and counts a stuck slot."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests.mp_net_model import READY, MPNetRunner
from tests.test_hostcheck_runner_x import _craft, ptr
from tests.test_mp_runner_model import parse_key
from tests.hostcheck import hostcheck

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_players_net.npz")
XNET = {"begin": 0, "reply": 1, "reset": 2}


def load():
    L = C.CDLL(hostcheck.build("libsimt_net_x.so"))
    L.shx_net.restype = C.c_longlong
    L.shx_net.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_void_p] * 10
    return L


class NetEmu:
    """n games of one batch shape on the emulated kernel body, next to n models; the host's protocol buffers persist across cuts."""

    def __init__(self, L, P, first, pool, ext, n, seed0=None, rngs=None):
        self.L, self.P, self.n = L, P, n
        self.D = 2 * P + 1 if ext & oz.EXT_DISPLAYS_2P1 else 5
        self.NA, self.OBS = (self.D + 1) * 30, 5 * self.D + 6 + 52 * P + 1
        self.models = [MPNetRunner(P, first, pool, ext, seed=None if rngs else seed0 + g, rng=rngs[g] if rngs else None) for g in range(n)]
        for m in self.models:
            assert m.runner_init() == 0                                   # GameRunner.__init__ (azul_batch_mp_runner_init's job)
        self.sync_from_models()
        self.ep, self.stuck, self.ss = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 10))
        self.first = first
        self.xpool = 2 if ext & oz.EXT_FINITE_BAG else (1 if pool == oz.POOL_LID else 0)
        self.eb, self.sd = int(bool(ext & oz.EXT_END_BONUS)), int(bool(ext & oz.EXT_SHORT_DEAL))
        self.pending, self.replies, self.status = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)

    def sync_from_models(self):
        self.state = np.stack([m.record() for m in self.models])
        self.mt = np.stack([m.rng_state()[0] for m in self.models]).astype(np.uint32)
        self.pos = np.array([m.rng_state()[1] for m in self.models], np.uint32)

    def owing(self):
        return [g for g, m in enumerate(self.models) if m.pending != READY]

    def cut(self, op, actions=None):
        n = self.n
        out = {"reward": np.full(n, -77, np.int32), "done": np.full(n, 9, np.uint8), "obs": np.full((n, self.OBS), -5, np.float32),
               "mask": np.full((n, self.NA), 7, np.uint8), "owing": np.zeros(1, np.uint32)}
        acts = None if actions is None else np.ascontiguousarray(actions, np.int32)
        ops = self.L.shx_net(n, self.P, self.D, ptr(self.state), ptr(self.mt), ptr(self.pos), ptr(self.ep), ptr(self.stuck), ptr(self.ss),
                             self.first, self.xpool, self.eb, self.sd, XNET[op], ptr(acts), None, ptr(self.pending), ptr(self.replies),
                             ptr(out["reward"]), ptr(out["done"]), ptr(self.status), ptr(out["obs"]), ptr(out["mask"]), ptr(out["owing"]))
        assert ops > 0
        moved = []
        for g, m in enumerate(self.models):
            was_closed = m.closed if op == "reply" else False
            if op == "begin":
                st = m.net_begin(actions[g])
            elif op == "reply":
                st = m.net_reply(actions[g])
            else:
                m.net_reset()
                st = 0
            moved.append(st)
            closed_now = m.closed and not was_closed
            assert self.pending[g] == m.pending and self.replies[g] == min(m.replies, 255), (op, g, self.pending[g], m.pending)
            assert self.status[g] == m.st, (op, g, self.status[g], m.st)
            if closed_now:
                assert (out["reward"][g], out["done"][g]) == (m.rew, m.dn), (op, g, out["reward"][g], out["done"][g], m.rew, m.dn)
            else:
                assert (out["reward"][g], out["done"][g]) == (-77, 9), (op, g)
            if m.pending != READY:
                obs, mask, _ = m.opp_view()
                assert np.array_equal(out["obs"][g], obs), (op, g, np.flatnonzero(out["obs"][g] != obs))
                assert np.array_equal(out["mask"][g], mask), (op, g)
            else:
                assert (out["obs"][g] == -5).all() and (out["mask"][g] == 7).all(), (op, g)
            assert np.array_equal(self.state[g], m.record()), (op, g, np.flatnonzero(self.state[g] != m.record()))
            mt, pos = m.rng_state()
            assert self.pos[g] == pos and np.array_equal(self.mt[g], mt), (op, g)
            assert (self.ep[g], self.stuck[g]) == (m.episodes, m.stuck), (op, g)
            assert np.array_equal(self.ss[g], m.stat_sum), (op, g)
        assert int(out["owing"][0]) == len(self.owing()), (op, int(out["owing"][0]), self.owing())
        return out, moved

    def run_replies(self, answer, max_rounds=400):
        """Reply rounds while any game owes an opponent_move(); answer(g, model) -> action (ignored for the games that owe nothing)."""
        rounds = 0
        while self.owing():
            acts = [answer(g, m) if m.pending != READY else -3 for g, m in enumerate(self.models)]
            self.cut("reply", acts)
            rounds += 1
            assert rounds < max_rounds
        return rounds


def pick_agent(emu, rnd, illegal_rate=0.03):
    acts = []
    for m in emu.models:
        legal = np.flatnonzero(m.mask())
        if rnd.random() < illegal_rate or len(legal) == 0:
            bad = np.flatnonzero(m.mask() == 0)
            acts.append(rnd.choice([-1, emu.NA] + ([int(bad[0])] if len(bad) else [])))
        else:
            acts.append(int(rnd.choice(list(legal))))
    return acts


def random_answers(rnd, illegal_rate=0.0):
    def answer(g, m):
        mask = m.mask()
        if rnd.random() < illegal_rate:
            bad = np.flatnonzero(mask == 0)
            return rnd.choice([-1, len(mask), 10_000] + ([int(bad[0])] if len(bad) else []))
        return int(rnd.choice(list(np.flatnonzero(mask))))
    return answer


CASES = [  # (P, first, pool, ext): (3, 5) / (4, 5) under the reference's rules; (2, 5), (3, 7), (4, 9) with extended rules
    (3, oz.FIRST_RANDOM, oz.POOL_LID, 0),
    (4, 1, oz.POOL_RANDOM, 0),
    (2, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_END_BONUS),
    (3, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS),
    (4, 2, oz.POOL_RANDOM, oz.EXT_DISPLAYS_2P1 | oz.EXT_FINITE_BAG | oz.EXT_SHORT_DEAL),
]


@pytest.mark.parametrize("P,first,pool,ext", CASES)
def test_net_body_matches_the_model_with_random_answers(P, first, pool, ext):
    L = load()
    emu = NetEmu(L, P, first, pool, ext, 2, 8100 + 31 * P + ext)
    rnd = random.Random(P * 1000 + ext)
    answer = random_answers(rnd, illegal_rate=0.05)                      # some answers are not legal: nothing moves, the debt stays
    emu.cut("reset")
    emu.run_replies(answer)
    statuses = set()
    for t in range(70):
        emu.cut("begin", pick_agent(emu, rnd))
        emu.run_replies(answer)
        statuses.update(int(m.st) for m in emu.models)
    assert emu.ep.sum() >= 1
    assert statuses & {1, 4}, "the run should meet refused moves"


def _fixture_keys():
    keys = [str(k) for k in np.load(GOLDEN)["keys"]]
    return sorted({k.rsplit("_", 1)[0] for k in keys})


@pytest.mark.parametrize("stem", _fixture_keys())
def test_net_body_replays_the_fixtures_network_answers(stem):
    """The reference's own runs with a network opponent (two seeds of one batch shape = one wave): the fixture's agent actions and the
    net's recorded answers, handed to the games that owe them, reproduce the model -- and so the reference -- call by call."""
    z = np.load(GOLDEN)
    keys = [k for k in (str(x) for x in z["keys"]) if k.rsplit("_", 1)[0] == stem]
    P, first, pool = parse_key(keys[0])
    rngs = []
    for k in keys:
        r = oz.Rng()
        oz.lib().oz_rng_set(C.byref(r), np.ascontiguousarray(z[k + "__mt0"], np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)), int(z[k + "__pos0"]))
        rngs.append(r)
    emu = NetEmu(load(), P, first, pool, 0, len(keys), rngs=rngs)
    nxt = [0] * len(keys)

    def answer(g, m):
        f = lambda name: z[keys[g] + "__" + name]
        i = nxt[g]
        obs, mask, player = m.opp_view()
        assert np.array_equal(obs, f("call_state")[i].astype(np.float32)) and player == int(f("call_player")[i]), (g, i)
        nxt[g] += 1
        return int(f("call_answer")[i])

    emu.cut("reset")
    emu.run_replies(answer)
    for t in range(len(z[keys[0] + "__action"])):
        emu.cut("begin", [int(z[k + "__action"][t]) for k in keys])
        emu.run_replies(answer)
        for g, k in enumerate(keys):
            m = emu.models[g]
            assert m.st == 0 and m.dn == int(z[k + "__done"][t]), (k, t)
            assert np.array_equal(m.obs(0), z[k + "__obs"][t]) and np.array_equal(m.mask(), z[k + "__mask"][t]), (k, t)
            assert nxt[g] == int((z[k + "__call_step"] <= t).sum()), (k, t)
    assert [int(x) for x in emu.ep] == [int(z[k + "__done"].sum()) for k in keys]


@pytest.mark.parametrize("P", [3, 4])
def test_nobody_can_move_closes_the_step_with_done_2(P):
    """The agent takes the last tile; the first-player token keeps the round open, yet the next seat has no legal move (hazard H3): the step
    closes with done = 2, reward 0, a stuck slot, and the slot restarts with its opening owed to the net."""
    L = load()
    emu = NetEmu(L, P, oz.FIRST_RANDOM, oz.POOL_LID, 0, 2, 9300 + P)
    for m in emu.models:
        _craft(m, token_only=False)
    emu.sync_from_models()
    a = int(np.flatnonzero(emu.models[0].mask())[0])
    out, _ = emu.cut("begin", [a, a])
    assert list(out["done"]) == [2, 2] and list(out["reward"]) == [0, 0] and emu.stuck.sum() == 2
    assert list(emu.status) == [3, 3]
    emu.run_replies(random_answers(random.Random(P)))


def test_an_illegal_answer_moves_nothing_and_keeps_the_debt():
    L = load()
    emu = NetEmu(L, 3, 1, oz.POOL_LID, 0, 2, 9400)
    emu.cut("reset")
    assert not emu.owing()                                              # seat 0 opens: nothing owed
    rnd = random.Random(5)
    emu.cut("begin", pick_agent(emu, rnd, illegal_rate=0.0))
    assert emu.owing() == [0, 1]
    before = emu.state.copy(), emu.mt.copy(), emu.pos.copy()
    bad = [int(np.flatnonzero(m.mask() == 0)[0]) for m in emu.models]
    _, moved = emu.cut("reply", [bad[0], -1])
    assert moved == [1, 4] and list(emu.status) == [1, 4] and list(emu.pending) == [1, 1] and list(emu.replies) == [0, 0]
    assert np.array_equal(emu.state, before[0]) and np.array_equal(emu.mt, before[1]) and np.array_equal(emu.pos, before[2])
    emu.run_replies(random_answers(rnd))                                # a legal answer then ends the step; its status stays the first one
    assert list(emu.status) == [1, 4]
