"""The greedy opponent INSIDE the persistent policy rollout kernel, on CPU: azul_policy_rollout2_kernel<LID, 3> (csrc/azul_rollout2.hpp: the
agent's move, then az2::greedy_pick2's answers while either half of the wave owes an opponent_move(), csrc/azul_env2.hpp) compiled
UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts (tests/hostcheck/simt_rollout2.cpp: sr2_window, opp 3).  Every game is replayed
through the oracle's callback GameRunner with the host model's greedy choice (tests/score_moves_model.py) as the opponent, fed the
kernel's own agent actions: observation, mask, player, reward, done, the number of opponent moves and every traced answer per step; the
final record bytes, all 624 MT19937 words and the index, the episode / stuck counters, the returns scan; opp_logp untouched; the agent's
value / log-prob / entropy against a numpy forward.  Both rule sets, a ragged last workgroup with an odd game count, a trace shorter
than a step's replies, and the move limit.  Reference: azulnet/game_runner.py:37-55, 76-85; azulnet/nn_runner.py:17-47."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests import greedy_rollout_cases as gc
from tests.hostcheck import window
from tests.hostcheck.window import forward, games_fields, to_agent_decision
from tests.hostcheck.window import load2 as load, weights2 as weights
from tests.test_hostcheck_env2 import RULES, start_batch


def run_greedy(L, first, pool, n, T, seed0, warm, slots=4, move_limit=0, gamma=0.9):
    state, mt, pos = start_batch(n, seed0, first, pool, warm)
    rng = np.random.default_rng(seed0)
    for g in range(n):
        state[g], mt[g], pos[g] = to_agent_decision(state[g].view(oz.RECORD_DTYPE)[0], mt[g], pos[g], first, pool, rng)
    state0, mt0, pos0 = state.copy(), mt.copy(), pos.copy()
    ep, stuck, ss = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 10))
    w = weights(seed0)
    o = {"obs": np.full((T + 1, n, 136), -99, np.float32), "mask": np.full((T + 1, n, 180), 0xEE, np.uint8),
         "player": np.full((T + 1, n), 9, np.uint8), "action": np.full((T, n), -7, np.int32), "reward": np.full((T, n), -7777, np.int32),
         "done": np.full((T, n), 9, np.uint8), "value": np.full((T, n), np.nan, np.float32), "logp": np.full((T, n), np.nan, np.float32),
         "entropy": np.full((T, n), np.nan, np.float32), "status": np.full(n, 99, np.uint8), "returns": np.full((T, n), np.nan, np.float32),
         "opp_action": np.full((T, slots, n), -9, np.int32), "opp_logp": np.full((T, slots, n), 123.5, np.float32),
         "opp_replies": np.full((T, n), 200, np.uint8)}
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **games_fields(n, state, mt, pos, ep, stuck, ss, first, pool), move_limit=move_limit, opp=3, agent=w, n_steps=T, **o,
                     gamma=gamma, seed=4242, counter=17, opp_slots=slots)
    assert ops > 0 and L.sr2_buffer_oob() == oob0
    assert (o["opp_logp"] == 123.5).all()                   # the greedy player has no log-probability: never written
    fp = first if first else oz.FIRST_RANDOM
    tot = {"calls": 0, "forced": 0, "opening": 0, "ties": 0, "cuts": 0, "episodes": 0, "untraced": 0, "zero": 0, "siblings": 0}
    for g in range(n):
        tag = (first, pool, g)
        for t in range(T):
            a = int(o["action"][t, g])
            value, logp, ent = forward(w, o["obs"][t, g], o["mask"][t, g])
            assert abs(o["value"][t, g] - value) < 2e-4 * max(1.0, abs(value)) and abs(o["logp"][t, g] - logp[a]) < 2e-4, (tag, t)
            assert abs(o["entropy"][t, g] - ent) < 2e-4 * max(1.0, ent), (tag, t)
        run, c = gc.replay(state0[g].view(oz.RECORD_DTYPE)[0], mt0[g], pos0[g], fp, pool, o["action"][:, g], o["opp_action"][:, :, g],
                           o["opp_replies"][:, g], o["obs"][:, g], o["mask"][:, g], o["player"][:, g], o["reward"][:, g], o["done"][:, g], move_limit)
        for k in ("calls", "forced", "opening", "cuts"):
            tot[k] += c[k]
        rep = o["opp_replies"][:, g].astype(int)
        # slots beyond a step's replies keep what they held
        assert (o["opp_action"][:, :, g][np.arange(slots)[None, :] >= rep[:, None]] == -9).all(), tag
        tot["untraced"] += int((rep > slots).sum())
        tot["zero"] += int((rep == 0).sum())
        m_e, idx = run.rng_state()
        assert state[g].tobytes() == run.record().tobytes() and int(pos[g]) == idx and np.array_equal(mt[g], m_e), tag
        assert int(ep[g]) == int((o["done"][:, g] == 1).sum()) and int(stuck[g]) == int((o["done"][:, g] == 3).sum()), tag
        assert int(o["status"][g]) == (gc.ST_TRUNCATED if int(o["done"][T - 1, g]) == 3 else 0), tag
        tot["episodes"] += int((o["done"][:, g] != 0).sum())
        q, want = np.float32(0), np.zeros(T, np.float32)
        for t in range(T - 1, -1, -1):
            q = np.float32(o["reward"][t, g]) + np.float32(gamma) * (np.float32(0) if o["done"][t, g] else q)
            want[t] = q
        assert np.array_equal(o["returns"][:, g], want), tag
    rep = o["opp_replies"].astype(int)
    tot["siblings"] = int((rep[:, 0:n - n % 2:2] != rep[:, 1:n:2]).sum())          # the halves of a wave owed different numbers of replies
    return ops, tot


@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
def test_greedy_opponent_in_the_rollout_kernel_replays_through_the_oracle(ruleset):
    L = load()
    first, pool = RULES[ruleset]
    ops, tot = run_greedy(L, first, pool, n=19, T=24, seed0=300, warm=40)          # (a ragged last workgroup, an odd count)
    assert ops > 5000 and tot["calls"] >= 19 * 24 // 2
    assert tot["zero"] >= 1 and tot["siblings"] >= 10 and tot["forced"] >= 1 and tot["episodes"] >= 1, tot


def test_greedy_opponent_with_a_move_limit_and_a_short_trace():
    """The move limit (beyond the reference, off by default) on the greedy protocol: a move of either side that ends a round once the
    episode has played `limit` moves cuts the episode (done = 3, reward 0, slot restarted, the opponent opens); one trace slot only."""
    L = load()
    first, pool = RULES["lid_randomfirst"]
    ops, tot = run_greedy(L, first, pool, n=16, T=24, seed0=900, warm=20, slots=1, move_limit=22)
    assert tot["cuts"] >= 6 and tot["opening"] >= 1 and tot["untraced"] >= 10, tot
