"""The window kernel of wide batches on CPU: x_policy_rollout_body (csrc/azul_rollout2.hpp, the body of azul_x_policy_rollout_kernel --
env phases on the P-seat GameRunner of azul_rules_x.hpp, layers 1 and 2 as v_mfma_f32_16x16x4_f32 chains over zero-padded K and partial
column tiles, the head of azul_policy_head_n_kernel, the trajectory slots copied out of LDS in dwords) compiled UNMODIFIED by g++ and run as
a workgroup of eight emulated wavefronts (tests/hostcheck/simt: run_workgroup, s_barrier, MFMA emulation, LDS poisoned before every
workgroup).  Every move of every game is checked against references that share no code with the kernel:
  * value, log-prob and entropy against a numpy f32 forward of the same weights on the observation the kernel recorded;
  * the action against tests/policy_draw_ref.py (host Philox4x32-10 + fp64 inverse CDF), rows near a CDF boundary excused;
  * the env: the kernel's own actions replayed through tests/mp_runner_model.py (the oracle's P-seat GameRunner) give the recorded
    observations, masks, players, rewards and done flags, and after the window the same records (runner tail included), MT19937 words and
    index, counters and status;
  * the trajectory arrays are written exactly where they belong: guard cells around every output stay untouched.
The games start part-way through their episodes (random legal moves on the models first), so that episodes end and restart inside the
window; the batch of 37 games leaves the last workgroup ragged."""
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests import policy_draw_ref as pdr
from tests.mp_runner_model import MPRunner
from tests.hostcheck import window
from tests.hostcheck.window import GUARD, buf, games_fields_x
from tests.hostcheck.window import load_x as load, weights_x as weights


CASES = [  # (P, first, pool, ext, opp)
    (3, oz.FIRST_RANDOM, oz.POOL_LID, 0, 0), (3, oz.FIRST_RANDOM, oz.POOL_LID, 0, 1),
    (4, oz.FIRST_RANDOM, oz.POOL_RANDOM, oz.EXT_DISPLAYS_2P1 | oz.EXT_SHORT_DEAL, 0),
    (4, 2, oz.POOL_LID, oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS, 1),
    (3, oz.FIRST_RANDOM, oz.POOL_LID, oz.EXT_DISPLAYS_2P1, 0), (3, 1, oz.POOL_RANDOM, oz.EXT_DISPLAYS_2P1 | oz.EXT_FINITE_BAG, 1),
]


@pytest.mark.parametrize("P,first,pool,ext,opp", CASES, ids=["p3d5_opp0", "p3d5_opp1", "p4d9_opp0", "p4d9_opp1", "p3d7_opp0", "p3d7_opp1"])
def test_window_kernel_matches_numpy_forward_draw_reference_and_runner_model(P, first, pool, ext, opp):
    L = load()
    n, T, seed, counter, id_base = 37, 8, 0x5EED + P, 40, 1000
    D = 2 * P + 1 if ext & oz.EXT_DISPLAYS_2P1 else 5
    NA, OBS = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
    rnd = random.Random(100 * P + ext + opp)
    models = [MPRunner(P, first, pool, ext, seed=3000 + 17 * P + g) for g in range(n)]
    for g, m in enumerate(models):                     # GameRunner() (+ reset() with RandomAgent seats), then part of an episode
        m.runner_init()
        if opp:
            m.reset()
        for _ in range(rnd.randrange(0, 30 * P if opp == 0 else 10 * P)):     # (an episode: ~26 P moves, ~8 P agent steps)
            legal = np.flatnonzero(m.mask())
            a = int(rnd.choice(list(legal))) if len(legal) else -1
            (m.agent_step if opp else m.policy_step)(a)
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
                               ("status", (n,), np.uint8, 99)):
        whole[k], o[k] = buf(shape, dt, fill)
    oob0 = L.sxr_buffer_oob()
    ops = window.run(L, **games_fields_x(n, P, D, state, mt, pos, ep, stuck, ss, first, pool, ext, id_base), opp=opp, agent=w, n_steps=T, **o,
                     seed=seed, counter=counter)
    assert ops > 0
    assert L.sxr_buffer_oob() == oob0
    for k in whole:                                    # nothing written past any array
        tail = whole[k][-GUARD:]
        assert (np.isnan(tail).all() if tail.dtype == np.float32 and k in ("value", "logp", "entropy") else (tail == whole[k][-1]).all()), k
    # -- the network and the head, move by move, against a numpy f32 forward and the host draw reference
    for t in range(T):
        obs = o["obs"][t]
        assert np.array_equal(obs, np.round(obs)), t                      # get_state is integer-valued
        h = np.maximum(obs @ w["w1t"] + w["b1"], np.float32(0))
        value = h[:, :180] @ w["w2c"] + w["b2c"][0]
        logits = (h[:, 180:] @ w["w2a_t"] + w["b2a"]).astype(np.float32)
        assert np.allclose(o["value"][t], value, atol=1e-4, rtol=1e-5), t
        ref = pdr.head(logits, o["mask"][t], seed, counter + t, id_base=id_base)
        # the kernel's logits differ from numpy's by f32 summation order (|err| < 1e-4): CDF shift and log-prob slack of that size
        pdr.compare(ref, o["action"][t], o["logp"][t], o["entropy"][t], extra_lp=4e-4, extra_draw=4e-4, extra_ent=4e-4)
    # -- the env: the kernel's actions through the model
    dones = 0
    for g, m in enumerate(models):
        last = None
        for t in range(T):
            p = 0 if opp else (m.g.current_player - 1) % P
            assert np.array_equal(o["obs"][t, g], m.obs(p).astype(np.float32)), (g, t)
            assert np.array_equal(o["mask"][t, g], m.mask()), (g, t)
            assert o["player"][t, g] == m.g.current_player, (g, t)
            a = int(o["action"][t, g])
            st, rew, dn = (m.agent_step if opp else m.policy_step)(a)
            assert (o["reward"][t, g], o["done"][t, g]) == (rew, dn), (g, t)
            dones += int(dn != 0)
            last = st
        p = 0 if opp else (m.g.current_player - 1) % P
        assert np.array_equal(o["obs"][T, g], m.obs(p).astype(np.float32)), g
        assert np.array_equal(o["mask"][T, g], m.mask()) and o["player"][T, g] == m.g.current_player, g
        assert np.array_equal(state[g], m.record()), (g, np.flatnonzero(state[g] != m.record()))
        mtm, posm = m.rng_state()
        assert pos[g] == posm and np.array_equal(mt[g], mtm), g
        assert (ep[g], stuck[g]) == (m.episodes, m.stuck) and np.array_equal(ss[g], m.stat_sum), g
        assert o["status"][g] == last, g
    assert dones > 0                                   # episodes ended (and restarted) inside the window
