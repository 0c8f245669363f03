"""The window kernel of wide batches with a NETWORK opponent on CPU: x_policy_rollout_body<P, D, 2> (csrc/azul_rollout2.hpp, the body of
azul_x_policy_rollout_vs_kernel -- the agent's pass, then reply rounds on the opponent's weights while any game of the workgroup owes an
opponent_move(), the game and its reply-loop state kept in LDS between the passes) compiled UNMODIFIED by g++ and run as a workgroup of eight
emulated wavefronts (tests/hostcheck/simt: run_workgroup, s_barrier, MFMA emulation, LDS poisoned before every workgroup).  Every step of every
game is checked against references that share no code with the kernel:
  * the agent's value, log-prob and entropy against a numpy f32 forward on the observation the kernel recorded, its action against
    tests/policy_draw_ref.py (host Philox4x32-10 + fp64 inverse CDF), rows near a CDF boundary excused;
  * every opponent answer the kernel recorded (opp_action / opp_logp, round j of step t) against a numpy f32 forward_actor of the opponent's
    weights on the model's mover-perspective observation and the draw reference at key opp_seed + j, counter + t;
  * the env: tests/mp_net_model.MPNetRunner driven with the kernel's own agent actions and answers gives the recorded observations, masks,
    players, rewards, done flags and reply counts, and after the window the same records (runner tail included), MT19937 words and index,
    counters and status;
  * the trace is written exactly for the rounds a game owed, and nothing is written past any output array (guard cells).
The games start part-way through their episodes, so that episodes end, and the next episodes' openings are played, inside reply rounds; the
batch of 37 games leaves the last workgroup ragged."""
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests import policy_draw_ref as pdr
from tests.mp_net_model import READY, MPNetRunner
from tests.hostcheck import window
from tests.hostcheck.window import GUARD, buf, games_fields_x
from tests.hostcheck.window import load_x as load, weights_x as weights

SLOTS = 64                     # trace slots per step: more than any step's reply rounds with legal answers


CASES = [  # (P, first, pool, ext, opponent selection)
    (3, oz.FIRST_RANDOM, oz.POOL_LID, 0, "Distribution"),
    (4, oz.FIRST_RANDOM, oz.POOL_LID, 0, "Max"),
    (4, 2, oz.POOL_RANDOM, oz.EXT_DISPLAYS_2P1 | oz.EXT_SHORT_DEAL, "Distribution"),
    (3, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS, "Distribution"),
    (2, oz.FIRST_RANDOM, oz.POOL_RANDOM, oz.EXT_END_BONUS | oz.EXT_FINITE_BAG, "Max"),
]


@pytest.mark.parametrize("P,first,pool,ext,sel", CASES, ids=["p3d5", "p4d5_max", "p4d9", "p3d7", "p2d5x_max"])
def test_window_kernel_vs_network_matches_numpy_forwards_draw_reference_and_net_model(P, first, pool, ext, sel):
    L = load()
    n, T, seed, counter, id_base = 37, 10, 0x5EED + P, 40, 1000
    opp_seed = pdr.ARGMAX if sel == "Max" else 0x0770 + P
    D = 2 * P + 1 if ext & oz.EXT_DISPLAYS_2P1 else 5
    NA, OBS = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
    rnd = random.Random(100 * P + ext)

    def rand_answer(obs, mask, player):
        legal = np.flatnonzero(mask)
        return int(rnd.choice(list(legal))) if len(legal) else -1

    models = [MPNetRunner(P, first, pool, ext, seed=4000 + 17 * P + g) for g in range(n)]
    for m in models:                                   # GameRunner() + reset() with the opponent, then part of an episode
        m.runner_init()
        m.reset_with(rand_answer)
        for _ in range(rnd.randrange(0, 45)):           # (an episode: some 40 agent steps)
            m.step_with(rand_answer(*m.opp_view()), rand_answer)
    state = np.stack([m.record() for m in models])
    mt = np.stack([m.rng_state()[0] for m in models]).astype(np.uint32)
    pos = np.array([m.rng_state()[1] for m in models], np.uint32)
    ep = np.array([m.episodes for m in models], np.uint64)
    stuck = np.array([m.stuck for m in models], np.uint32)
    ss = np.stack([m.stat_sum for m in models]).astype(np.float64)
    w, wo = weights(OBS, NA, seed), weights(OBS, NA, seed + 1)
    o, whole = {}, {}
    for k, shape, dt, fill in (("obs", (T + 1, n, OBS), np.float32, -99), ("mask", (T + 1, n, NA), np.uint8, 0xEE), ("player", (T + 1, n), np.uint8, 9),
                               ("action", (T, n), np.int32, -7), ("reward", (T, n), np.int32, -7777), ("done", (T, n), np.uint8, 9),
                               ("value", (T, n), np.float32, np.nan), ("logp", (T, n), np.float32, np.nan), ("entropy", (T, n), np.float32, np.nan),
                               ("status", (n,), np.uint8, 99), ("opp_action", (T, SLOTS, n), np.int32, -5), ("opp_logp", (T, SLOTS, n), np.float32, 55.0),
                               ("opp_replies", (T, n), np.uint8, 201)):
        whole[k], o[k] = buf(shape, dt, fill)
    oob0 = L.sxr_buffer_oob()
    ops = window.run(L, **games_fields_x(n, P, D, state, mt, pos, ep, stuck, ss, first, pool, ext, id_base), opp=2, agent=w, opponent=wo,
                     n_steps=T, **o, opp_slots=SLOTS, seed=seed, opp_seed=opp_seed, counter=counter, max_replies=512)
    assert ops > 0
    assert L.sxr_buffer_oob() == oob0
    for k in whole:                                    # nothing written past any array
        tail = whole[k][-GUARD:]
        assert (np.isnan(tail).all() if tail.dtype == np.float32 and k in ("value", "logp", "entropy") else (tail == whole[k][-1]).all()), k
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
    # -- the env and the opponent: the kernel's agent actions and answers through the model, every answer against the references
    dones = in_round_openings = answers = 0
    for g, m in enumerate(models):
        for t in range(T):
            assert np.array_equal(o["obs"][t, g], m.obs(0).astype(np.float32)), (g, t)
            assert np.array_equal(o["mask"][t, g], m.mask()) and o["player"][t, g] == m.g.current_player, (g, t)
            m.net_begin(int(o["action"][t, g]))
            j = 0
            while m.pending != READY:
                assert j < SLOTS, (g, t)
                vobs, vmask, _ = m.opp_view()
                ho = np.maximum(vobs[None] @ wo["w1t"][:, 180:] + wo["b1"][180:], np.float32(0))
                lo = (ho @ wo["w2a_t"] + wo["b2a"]).astype(np.float32)
                ref = pdr.head(lo, vmask[None], opp_seed if sel == "Max" else opp_seed + j, counter + t, id_base=id_base + g)
                a = int(o["opp_action"][t, j, g])
                pdr.compare(ref, [a], [o["opp_logp"][t, j, g]], ref["entropy"], extra_lp=4e-4, extra_draw=4e-4)
                if m.closed and m.dn == 1:
                    in_round_openings += 1             # an answer of the next episode's opening, inside the step
                m.net_reply(a)
                answers += 1
                j += 1
            assert (o["opp_action"][t, j:, g] == -5).all() and (o["opp_logp"][t, j:, g] == 55.0).all(), (g, t)    # no round, no trace
            assert (o["reward"][t, g], o["done"][t, g], o["opp_replies"][t, g]) == (m.rew, m.dn, m.replies), (g, t)
            dones += int(m.dn == 1)
        assert np.array_equal(o["obs"][T, g], m.obs(0).astype(np.float32)), g
        assert np.array_equal(o["mask"][T, g], m.mask()) and o["player"][T, g] == m.g.current_player, g
        assert np.array_equal(state[g], m.record()), (g, np.flatnonzero(state[g] != m.record()))
        mtm, posm = m.rng_state()
        assert pos[g] == posm and np.array_equal(mt[g], mtm), g
        assert (ep[g], stuck[g]) == (m.episodes, m.stuck) and np.array_equal(ss[g], m.stat_sum), g
        assert o["status"][g] == m.st, g
    assert answers > T * n                             # every step had replies on average
    assert dones > 0 and in_round_openings > 0         # episodes ended inside the window, and the next ones opened inside reply rounds
