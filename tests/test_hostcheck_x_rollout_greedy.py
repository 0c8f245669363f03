"""The window kernel of wide batches with GREEDY_MARGIN seats on CPU: x_policy_rollout_body<P, D, 3> (csrc/azul_rollout2.hpp, the body of
azul_x_policy_rollout_kernel<P, D, 3> -- the agent's pass, then reply rounds answered by azx::greedy_pick_x inside the wave that holds the
game, the game and its NetStep in registers for the step) compiled UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts
(tests/hostcheck/simt: run_workgroup, s_barrier, MFMA emulation, LDS poisoned before every workgroup).  Every step of every game is checked
against references that share no code with the kernel:
  * the agent's value, log-prob and entropy against a numpy f32 forward on the observation the kernel recorded, its action against
    tests/policy_draw_ref.py (host Philox4x32-10 + fp64 inverse CDF), rows near a CDF boundary excused;
  * the env and the opponent: tests/mp_net_model.MPNetRunner driven with the kernel's own agent actions and answered by
    tests/mp_score_moves_model.greedy_of_game gives the recorded observations, masks, players, rewards, done flags, reply counts and
    traced answers, and after the window the same records (runner tail included), all 624 MT19937 words and the index, counters and status;
  * opp_logp is never written, the trace is written exactly for the replies a game owed (and only the first opp_slots of them), and
    nothing is written past any output array (guard cells, buffer_oob).
19 games: a ragged last workgroup, an odd count, a wave with one live half.  The games start part-way through their episodes, a third of
them a few steps before their end.  The census -- sibling halves owing different numbers of replies, a step without a reply, an episode
ending inside a step, an opening played inside reply rounds, a tie resolved to the lowest action -- is computed from the replay, never from
the kernel's counters, and every class has to occur over the cases."""
import functools
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests import mp_score_moves_model as mm
from tests import policy_draw_ref as pdr
from tests.mp_net_model import READY, MPNetRunner
from tests.hostcheck import window
from tests.hostcheck.window import GUARD, buf, games_fields_x
from tests.hostcheck.window import load_x as load, weights_x as weights

N, T = 19, 6
CLASSES = ("siblings_differ", "zero_replies", "episode_ends_in_step", "opening_in_reply_rounds", "tie_to_lowest")


CASES = [  # (P, first, pool, ext, trace slots)
    (3, oz.FIRST_RANDOM, oz.POOL_LID, 0, 64),
    (4, 2, oz.POOL_RANDOM, oz.EXT_DISPLAYS_2P1 | oz.EXT_SHORT_DEAL, 64),
    (2, oz.FIRST_RANDOM, oz.POOL_RANDOM, oz.EXT_END_BONUS | oz.EXT_FINITE_BAG, 64),
    (3, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS, 1),         # a trace shorter than a step's replies
]
IDS = ["p3d5", "p4d9", "p2d5x", "p3d7_short_trace"]


def _answer_and_tie(m, P, cfg):
    """The model's greedy answer on the runner's own game, and whether the maximum is shared (the first of the tied actions is the answer)."""
    a = mm.greedy_of_game(m.g, P)
    tab = mm.table(m.record(), cfg)
    assert a == mm.greedy(tab) and a >= 0
    return a, int((tab == tab[a]).sum() > 1)


def _warm_models(P, first, pool, ext, rnd):
    """N runners opened as GameRunner() + reset() and played part of an episode with random legal moves on every seat; every third game
    stops one to three agent steps before its episode would end."""
    def play(seed, steps):
        r = random.Random(seed)
        pick = lambda obs, mask, player: int(r.choice(list(np.flatnonzero(mask)))) if mask.any() else -1
        m = MPNetRunner(P, first, pool, ext, seed=seed)
        m.runner_init()
        m.reset_with(pick)
        k = 0
        while k < steps:
            m.step_with(pick(*m.opp_view()), pick)
            k += 1
            if m.dn:
                break
        return m, k
    models = []
    for g in range(N):
        seed = 6000 + 31 * P + 7 * ext + g
        if g % 3 == 0:
            _, length = play(seed, 10 ** 6)             # the episode's length under this seed's random moves
            m, _ = play(seed, max(0, length - 1 - g % 3 - (g // 3) % 3))
        else:
            m, _ = play(seed, rnd.randrange(0, 30))
        models.append(m)
    return models


@functools.lru_cache(maxsize=None)
def run_case(i):
    """One launch of case i, every output checked against the references; returns the census of the replay."""
    P, first, pool, ext, slots = CASES[i]
    L = load()
    n, seed, counter, id_base = N, 0x5EED + P, 40, 1000
    D = 2 * P + 1 if ext & oz.EXT_DISPLAYS_2P1 else 5
    NA, OBS = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
    cfg = (P, ext, pool)
    models = _warm_models(P, first, pool, ext, random.Random(100 * P + ext))
    state = np.stack([m.record() for m in models])
    mt = np.stack([m.rng_state()[0] for m in models]).astype(np.uint32)
    pos = np.array([m.rng_state()[1] for m in models], np.uint32)
    ep = np.array([m.episodes for m in models], np.uint64)
    stuck = np.array([m.stuck for m in models], np.uint32)
    ss = np.stack([m.stat_sum for m in models]).astype(np.float64)
    w = weights(OBS, NA, seed)
    o, whole = {}, {}
    for k, shape, dt, fill in (("obs", (T + 1, n, OBS), np.float32, -99), ("mask", (T + 1, n, NA), np.uint8, 0xEE), ("player", (T + 1, n), np.uint8, 9),
                               ("action", (T, n), np.int32, -7), ("reward", (T, n), np.int32, -7777), ("done", (T, n), np.uint8, 9),
                               ("value", (T, n), np.float32, np.nan), ("logp", (T, n), np.float32, np.nan), ("entropy", (T, n), np.float32, np.nan),
                               ("status", (n,), np.uint8, 99), ("opp_action", (T, slots, n), np.int32, -5), ("opp_logp", (T, slots, n), np.float32, 55.0),
                               ("opp_replies", (T, n), np.uint8, 201)):
        whole[k], o[k] = buf(shape, dt, fill)
    oob0 = L.sxr_buffer_oob()
    ops = window.run(L, **games_fields_x(n, P, D, state, mt, pos, ep, stuck, ss, first, pool, ext, id_base), opp=3, agent=w, n_steps=T, **o,
                     opp_slots=slots, seed=seed, counter=counter, max_replies=512)
    assert ops > 0
    assert L.sxr_buffer_oob() == oob0
    for k in whole:                                    # nothing written past any array
        tail = whole[k][-GUARD:]
        assert (np.isnan(tail).all() if k in ("value", "logp", "entropy") else (tail == whole[k][-1]).all()), k
    assert (o["opp_logp"] == 55.0).all()               # the greedy seats have no log-probabilities: never written
    # -- the agent's network and head, step by step, against a numpy f32 forward and the host draw reference
    for t in range(T):
        obs = o["obs"][t]
        assert np.array_equal(obs, np.round(obs)), t
        h = np.maximum(obs @ w["w1t"] + w["b1"], np.float32(0))
        value = h[:, :180] @ w["w2c"] + w["b2c"][0]
        logits = (h[:, 180:] @ w["w2a_t"] + w["b2a"]).astype(np.float32)
        assert np.allclose(o["value"][t], value, atol=1e-4, rtol=1e-5), t
        ref = pdr.head(logits, o["mask"][t], seed, counter + t, id_base=id_base)
        pdr.compare(ref, o["action"][t], o["logp"][t], o["entropy"][t], extra_lp=4e-4, extra_draw=4e-4, extra_ent=4e-4)
    # -- the env and the greedy seats: the kernel's agent actions through the model, the model's own greedy answers
    census = dict.fromkeys(CLASSES, 0)
    replies = np.zeros((T, n), np.int64)
    for g, m in enumerate(models):
        for t in range(T):
            assert np.array_equal(o["obs"][t, g], m.obs(0).astype(np.float32)), (g, t)
            assert np.array_equal(o["mask"][t, g], m.mask()) and o["player"][t, g] == m.g.current_player, (g, t)
            m.net_begin(int(o["action"][t, g]))
            j = 0
            while m.pending != READY:
                assert j < 512, (g, t)
                a, tie = _answer_and_tie(m, P, cfg)
                census["tie_to_lowest"] += tie
                if j < slots:
                    assert int(o["opp_action"][t, j, g]) == a, (g, t, j, tie)
                if m.closed and m.dn == 1:
                    census["opening_in_reply_rounds"] += 1     # an answer of the next episode's opening, inside the step
                m.net_reply(a)
                j += 1
            assert (o["opp_action"][t, j:, g] == -5).all(), (g, t)             # no reply, no trace
            assert (o["reward"][t, g], o["done"][t, g], o["opp_replies"][t, g]) == (m.rew, m.dn, m.replies), (g, t)
            assert m.replies == j
            replies[t, g] = j
            census["zero_replies"] += int(j == 0)
            census["episode_ends_in_step"] += int(m.dn == 1)
        assert np.array_equal(o["obs"][T, g], m.obs(0).astype(np.float32)), g
        assert np.array_equal(o["mask"][T, g], m.mask()) and o["player"][T, g] == m.g.current_player, g
        assert np.array_equal(state[g], m.record()), (g, np.flatnonzero(state[g] != m.record()))
        mtm, posm = m.rng_state()
        assert pos[g] == posm and np.array_equal(mt[g], mtm), g
        assert (ep[g], stuck[g]) == (m.episodes, m.stuck) and np.array_equal(ss[g], m.stat_sum), g
        assert o["status"][g] == m.st, g
    for g in range(0, n - 1, 2):                        # games 2 w and 2 w + 1 share a wave
        census["siblings_differ"] += int((replies[:, g] != replies[:, g + 1]).sum())
    assert replies.sum() >= T * n                       # the seats really moved
    if slots < 64:
        assert (replies > slots).any()                  # (the short trace is shorter than some step's replies)
    return census


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_window_kernel_with_greedy_margin_seats_matches_forward_draw_reference_and_model_replay(i):
    census = run_case(i)
    print(IDS[i], census)
    assert all(census[k] >= 1 for k in CLASSES), census    # (each case meets every class on its own; the census below needs one of them)


def test_census_every_class_occurs():
    total = dict.fromkeys(CLASSES, 0)
    for i in range(len(CASES)):
        for k, v in run_case(i).items():
            total[k] += v
    print(total)
    assert all(total[k] >= 1 for k in CLASSES), total
