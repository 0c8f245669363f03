"""The persistent policy rollout kernel ITSELF on CPU: azul_policy_rollout2_kernel (csrc/azul_rollout2.hpp -- env phases, matrix phases
on v_mfma_f32_16x16x4_f32 with weights streamed through buffer loads, the sampling head, trajectory slots written by the idle waves,
the fused returns scan), compiled UNMODIFIED by g++ and run as a workgroup of eight emulated wavefronts (tests/hostcheck/simt:
run_workgroup, s_barrier, MFMA and buffer-load emulation).  Checked per move and game:
  * the network: value, log-prob of the sampled action and the entropy term against a numpy fp32 forward of the same weights on the
    observation the kernel recorded (model.py:22-41, agent.py:64-72), within fp32 tolerance;
  * the sampled action is legal;
  * the env: the kernel's own actions replayed through the oracle give the recorded observations, masks, players, rewards, done flags,
    final records, MT19937 words and counters (game_runner.py:43-97, nn_runner.py:17-47);
  * the returns scan (nn_runner.py:70-76) and that no buffer load ever left its resource.
Under ASan / UBSan (tests/hostcheck/run_sanitizers.sh) every LDS and global index the kernel forms is checked as well."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests.hostcheck import window
from tests.hostcheck.window import forward, games_fields, to_agent_decision
from tests.hostcheck.window import load2 as load, weights2 as weights
from tests.test_hostcheck_env2 import RULES, oracle_play, start_batch


def run(L, first, pool, opponent, n, T, seed0, warm=0, gamma=0.9, with_returns=True):
    state, mt, pos = start_batch(n, seed0, first, pool, warm)
    state0, mt0, pos0 = state.copy(), mt.copy(), pos.copy()
    ep, stuck, ss = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 10))
    w = weights(seed0)
    o = {"obs": np.full((T + 1, n, 136), -99, np.float32), "mask": np.full((T + 1, n, 180), 0xEE, np.uint8),
         "player": np.full((T + 1, n), 9, np.uint8), "action": np.full((T, n), -7, np.int32), "reward": np.full((T, n), -7777, np.int32),
         "done": np.full((T, n), 9, np.uint8), "value": np.full((T, n), np.nan, np.float32), "logp": np.full((T, n), np.nan, np.float32),
         "entropy": np.full((T, n), np.nan, np.float32), "status": np.full(n, 99, np.uint8),
         "returns": np.full((T, n), np.nan, np.float32)}
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **games_fields(n, state, mt, pos, ep, stuck, ss, first, pool), opp=int(opponent), agent=w, n_steps=T,
                     **dict(o, returns=o["returns"] if with_returns else None), gamma=gamma, seed=4242, counter=17)
    assert ops > 0
    assert L.sr2_buffer_oob() == oob0                       # no weight fragment was ever requested outside its matrix
    episodes = 0
    for g in range(n):
        tag = (first, pool, opponent, g)
        # -- the network and the head, move by move, on what the kernel recorded
        for t in range(T):
            a = int(o["action"][t, g])
            mask = o["mask"][t, g]
            assert set(np.unique(mask)) <= {0, 1} and 0 <= a < 180 and mask[a] == 1, (tag, t)
            value, logp, ent = forward(w, o["obs"][t, g], mask)
            assert abs(o["value"][t, g] - value) < 2e-4 * max(1.0, abs(value)), (tag, t)
            assert abs(o["logp"][t, g] - logp[a]) < 2e-4, (tag, t)
            assert abs(o["entropy"][t, g] - ent) < 2e-4 * max(1.0, ent), (tag, t)
        # -- the env: the kernel's actions through the oracle
        acts = o["action"][:, g]
        e, rec, mt_e, idx = oracle_play(state0[g].view(oz.RECORD_DTYPE)[0], mt0[g], pos0[g], T, first, pool, opponent, lambda m, t: int(acts[t]))
        assert np.array_equal(o["mask"][:, g].astype(bool), np.array(e["mask"], bool)), tag
        assert np.array_equal(o["obs"][:, g].astype(np.int64), np.array(e["obs"])), tag
        assert np.array_equal(o["player"][:, g], np.array(e["player"])), tag
        assert np.array_equal(o["reward"][:, g], np.array(e["reward"])), tag
        assert np.array_equal(o["done"][:, g].astype(bool), np.array(e["done"])), tag
        assert state[g].tobytes() == rec.tobytes() and int(pos[g]) == idx and np.array_equal(mt[g], mt_e), tag
        assert int(ep[g]) == int(np.sum(e["done"])) and int(stuck[g]) == 0 and int(o["status"][g]) == 0, tag
        episodes += int(np.sum(e["done"]))
        if with_returns:
            q, want = np.float32(0), np.zeros(T, np.float32)
            for t in range(T - 1, -1, -1):
                q = np.float32(o["reward"][t, g]) + np.float32(gamma) * (np.float32(0) if o["done"][t, g] else q)
                want[t] = q
            assert np.array_equal(o["returns"][:, g], want), tag
    return ops, episodes


@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
def test_policy_on_both_sides(ruleset):
    L = load()
    first, pool = RULES[ruleset]
    ops, _ = run(L, first, pool, False, n=16, T=7, seed0=60, warm=30)
    assert ops > 5000


def test_random_agent_opponent_and_a_ragged_last_workgroup():
    L = load()
    first, pool = RULES["lid_randomfirst"]
    ops, _ = run(L, first, pool, True, n=19, T=5, seed0=80, warm=45)
    assert ops > 5000


# ---- the NETWORK opponent (azul_policy_rollout2_kernel<LID, 2>; game_runner.py:27-30 GameRunner(opponent=Agent(...))) ----------------------
def actor_forward(w, obs, mask):
    h = np.maximum(obs.astype(np.float32) @ w["w1t"][:, 180:] + w["b1"][180:], np.float32(0))
    logits = (h @ w["w2a_t"] + w["b2a"]).astype(np.float64)
    legal = mask.astype(bool)
    z = logits[legal]
    lse = z.max() + np.log(np.exp(z - z.max()).sum())
    logp = np.full(180, -np.inf)
    logp[legal] = z - lse
    return logp


def run_vs(L, first, pool, n, T, seed0, warm, slots=8, argmax=False, move_limit=0):
    state, mt, pos = start_batch(n, seed0, first, pool, warm)
    rng = np.random.default_rng(seed0)
    for g in range(n):
        state[g], mt[g], pos[g] = to_agent_decision(state[g].view(oz.RECORD_DTYPE)[0], mt[g], pos[g], first, pool, rng)
    state0, mt0, pos0 = state.copy(), mt.copy(), pos.copy()
    ep, stuck, ss = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 10))
    wa, wo = weights(seed0), weights(seed0 + 1)
    o = {"obs": np.full((T + 1, n, 136), -99, np.float32), "mask": np.full((T + 1, n, 180), 0xEE, np.uint8),
         "player": np.full((T + 1, n), 9, np.uint8), "action": np.full((T, n), -7, np.int32), "reward": np.full((T, n), -7777, np.int32),
         "done": np.full((T, n), 9, np.uint8), "value": np.full((T, n), np.nan, np.float32), "logp": np.full((T, n), np.nan, np.float32),
         "entropy": np.full((T, n), np.nan, np.float32), "status": np.full(n, 99, np.uint8), "returns": np.full((T, n), np.nan, np.float32),
         "opp_action": np.full((T, slots, n), -9, np.int32), "opp_logp": np.full((T, slots, n), np.nan, np.float32),
         "opp_replies": np.full((T, n), 200, np.uint8)}
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **games_fields(n, state, mt, pos, ep, stuck, ss, first, pool), move_limit=move_limit, opp=2, agent=wa, opponent=wo,
                     n_steps=T, **o, gamma=0.9, seed=4242, opp_seed=window.ARGMAX if argmax else 777, counter=17, opp_slots=slots)
    assert ops > 0 and L.sr2_buffer_oob() == oob0
    episodes = forced = opening = cuts = 0
    for g in range(n):
        tag = (first, pool, g)
        assert int(o["opp_replies"][:, g].max()) <= slots, "raise `slots`: a step had more replies than the trace holds"
        cur = {"t": 0, "j": 0}
        handed = []

        def opponent(s, m):
            t, j = cur["t"], cur["j"]
            a = int(o["opp_action"][t, j, g])
            assert 0 <= a < 180 and m[a], (tag, t, j, a)
            handed.append((t, j, s.copy(), m.copy(), int(run.q.game.current_player)))
            cur["j"] += 1
            return a

        run = oz.NetRunner(opponent, first if first else oz.FIRST_RANDOM, pool, rec=state0[g].view(oz.RECORD_DTYPE)[0], mt=mt0[g], pos=pos0[g])
        for t in range(T):
            cur["t"], cur["j"] = t, 0
            mask = run.get_valid_moves()
            assert np.array_equal(o["mask"][t, g].astype(bool), mask), (tag, t)
            assert np.array_equal(o["obs"][t, g].astype(np.int64), run.get_state(0)), (tag, t)
            assert int(o["player"][t, g]) == 1 == int(run.q.game.current_player) and mask.sum() >= 2, (tag, t)
            a = int(o["action"][t, g])
            assert mask[a]
            value, logp, ent = forward(wa, o["obs"][t, g], o["mask"][t, g])
            assert abs(o["value"][t, g] - value) < 2e-4 * max(1.0, abs(value)) and abs(o["logp"][t, g] - logp[a]) < 2e-4, (tag, t)
            assert abs(o["entropy"][t, g] - ent) < 2e-4 * max(1.0, ent), (tag, t)
            rc, rew, dn = run.step(a, move_limit)                           # game_runner.py:43-55 with the recorded opponent
            assert rc == 0 and rew == int(o["reward"][t, g]) and int(dn) == int(o["done"][t, g]), (tag, t, rew, dn, int(o["done"][t, g]))
            cuts += int(dn) == 3
            if dn:
                episodes += 1
                before = cur["j"]
                assert run.reset() == 0                                     # nn_runner.py:20: the next episode, the opponent opens (:84-85)
                opening += cur["j"] - before
            assert cur["j"] == int(o["opp_replies"][t, g]), (tag, t, cur["j"], int(o["opp_replies"][t, g]))
        assert np.array_equal(o["mask"][T, g].astype(bool), run.get_valid_moves()) and np.array_equal(o["obs"][T, g].astype(np.int64), run.get_state(0)), tag
        m_e, idx = run.rng_state()
        assert state[g].tobytes() == run.record().tobytes() and int(pos[g]) == idx and np.array_equal(mt[g], m_e), tag
        assert int(ep[g]) == int((o["done"][:, g] == 1).sum()) and int(stuck[g]) == int((o["done"][:, g] == 3).sum()), tag
        assert int(o["status"][g]) == (6 if int(o["done"][T - 1, g]) == 3 else 0), tag
        # the opponent saw the MOVER's perspective and sampled from ITS net: log-prob of every answer against a numpy forward_actor
        for t, j, s, m, player in handed:
            lp = actor_forward(wo, s, m)
            a = int(o["opp_action"][t, j, g])
            assert abs(o["opp_logp"][t, j, g] - lp[a]) < 2e-4, (tag, t, j)
            if argmax:
                assert a == int(np.argmax(np.where(m, lp, -np.inf))) or abs(lp[a] - lp[m].max()) < 1e-5, (tag, t, j)
            forced += player == 1
        q, want = np.float32(0), np.zeros(T, np.float32)
        for t in range(T - 1, -1, -1):
            q = np.float32(o["reward"][t, g]) + np.float32(0.9) * (np.float32(0) if o["done"][t, g] else q)
            want[t] = q
        assert np.array_equal(o["returns"][:, g], want), tag
    run_vs.last_done = o["done"]
    return (ops, episodes, forced, opening, cuts) if move_limit else (ops, episodes, forced, opening)


def test_network_opponent_with_a_move_limit():
    """The move limit (beyond the reference, off by default) on the network-opponent protocol: a move of either side that ends a round
    without ending the game once the episode has played `limit` moves cuts the episode (done = 3, reward 0, slot restarted and opened)."""
    L = load()
    first, pool = RULES["lid_randomfirst"]
    ops, episodes, forced, opening, cuts = run_vs(L, first, pool, n=16, T=24, seed0=900, warm=20, move_limit=22)
    assert cuts >= 6


def test_network_opponent_in_the_rollout_kernel_replays_through_the_oracle():
    """GameRunner(opponent=Agent(...)) inside the kernel: the agent's records as with the RandomAgent opponent, every opponent_move() --
    replies, player 1's forced moves, the opening moves after an episode end -- answered by the second net on the mover's perspective."""
    L = load()
    first, pool = RULES["lid_randomfirst"]
    ops, episodes, forced, opening = run_vs(L, first, pool, n=19, T=6, seed0=300, warm=40)        # (a ragged last workgroup)
    assert ops > 5000 and episodes >= 1 and forced >= 1
    ops, episodes, forced, opening = run_vs(L, first, pool, n=16, T=30, seed0=500, warm=50)
    assert episodes >= 10 and forced >= 8 and opening >= 3


def test_network_opponent_window_ending_on_an_episode_end_reports_no_status():
    """The launch status is the LAST step's.  A window whose last step ends an episode also opens the next one (the opponent's opening
    moves while player 1 is not to move, game_runner.py:84-85): the opening loop that ends with player 1 to move leaves no status --
    AZUL_STUCK is for an opening in which the seat to move has no legal action.  (run_vs asserts the status of every game.)"""
    L = load()
    first, pool = RULES["lid_randomfirst"]
    run_vs(L, first, pool, n=16, T=30, seed0=500, warm=50)
    ends = [t for t in range(30) if (run_vs.last_done[t] == 1).any()]
    assert ends
    T = ends[0] + 1                                                         # the same window, cut right after its first episode end
    ops, episodes, forced, opening = run_vs(L, first, pool, n=16, T=T, seed0=500, warm=50)
    assert episodes >= 1 and (run_vs.last_done[T - 1] == 1).any()


def test_network_opponent_argmax_and_the_random_pool():
    L = load()
    first, pool = RULES["random_first1"]
    run_vs(L, first, pool, n=16, T=5, seed0=410, warm=30, argmax=True)
