"""azul_batch_score_moves on the MI355X: the table and `best` of the 360 states of three oracle streams against the host model
(tests/score_moves_model.py) at batch sizes 1, 2, 3 and 33, both pools, the three perspectives, with the games untouched; the optional
outputs and the refusals; PolicyRollout(opponent="greedy") replayed game by game through the oracle's GameRunner with the model's greedy
choice as the opponent; a BatchedTrainer smoke run.  The CPU suite runs the same kernel under the lockstep emulation
(tests/test_hostcheck_score_moves.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as oz
from tests import score_moves_model as sm

pytestmark = pytest.mark.gpu
CANARY = 0x5EED5EED
RULESETS = {"lid_randomfirst": ({"first_player": "Random", "tile_pool": "Lid"}, oz.FIRST_RANDOM, oz.POOL_LID),
            "random_first1": ({"first_player": 1, "tile_pool": "Random"}, 1, oz.POOL_RANDOM)}


def _batch(recs, rules):
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    env = BatchedAzul(len(recs), rules=rules, device="cuda", seed=77)
    env.set_records(np.ascontiguousarray(recs).view(env.record_dtype).reshape(-1))
    return env


def _snapshot(env):
    c = env.counters()
    mt, pos = env.get_rng_range()
    return env.get_records().tobytes(), mt.tobytes(), pos.tobytes(), c["episodes"].tobytes(), c["stuck"].tobytes(), c["stat_sums"].tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 33])
@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
def test_table_and_best_equal_the_model_and_the_games_are_untouched(ruleset, n):
    from azul_deep_reinforcement_learning_amd import _lib as L
    rules = RULESETS[ruleset][0]
    recs = sm.stream_states()[0]
    # a window of the shared states per size, chosen so that the four sizes together cover states of every part of the streams
    lo = {1: 119, 2: 57, 3: 200, 33: 0}[n]
    chunks = [slice(lo, lo + n)] if n < 33 else [slice(i, i + 33) for i in range(0, 330, 33)] + [slice(327, 360)]
    for sl in chunks:
        env = _batch(recs[sl], rules)
        before = _snapshot(env)
        for persp in (0, 1, L.PERSP_CURRENT):
            tabs, best = sm.stream_tables(persp)
            s, b = env.score_moves(persp)
            assert s.dtype == torch.int32 and tuple(s.shape) == (n, 180) and b.dtype == torch.int32 and tuple(b.shape) == (n,)
            assert np.array_equal(s.cpu().numpy().astype(np.int64), tabs[sl]), (sl, persp)
            assert np.array_equal(b.cpu().numpy(), best[sl]), (sl, persp)
        assert np.array_equal(env.greedy_action().cpu().numpy(), sm.stream_tables(L.PERSP_CURRENT)[1][sl]), sl
        # the legal mask is where the table holds a score
        assert np.array_equal(env.get_valid_moves().cpu().numpy(), sm.stream_tables(0)[0][sl] != sm.ILLEGAL)
        # an active mask with holes: the rows of the other games keep what they held
        active = torch.tensor([(i % 3) != 1 for i in range(n)], dtype=torch.uint8, device="cuda")
        s = torch.full((n, 180), CANARY, dtype=torch.int32, device="cuda")
        b = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
        env.score_moves(L.PERSP_CURRENT, active=active, scores=s, best=b)
        g = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
        env.greedy_action(active=active, out=g)
        on = active.cpu().numpy() != 0
        tabs, best = sm.stream_tables(L.PERSP_CURRENT)
        s, b, g = s.cpu().numpy(), b.cpu().numpy(), g.cpu().numpy()
        assert np.array_equal(s[on].astype(np.int64), tabs[sl][on]) and (s[~on] == CANARY).all()
        assert np.array_equal(b[on], best[sl][on]) and (b[~on] == CANARY).all()
        assert np.array_equal(g, b)
        assert _snapshot(env) == before, "score_moves changed records, MT19937 state or counters"


def test_optional_outputs_and_refusals():
    from azul_deep_reinforcement_learning_amd import BatchedAzul, _lib as L
    recs = sm.stream_states()[0][30:37]
    tabs, best = sm.stream_tables(L.PERSP_CURRENT)
    env = _batch(recs, RULESETS["lid_randomfirst"][0])
    n = len(recs)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    s = torch.full((n, 180), CANARY, dtype=torch.int32, device="cuda")
    b = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    assert L.lib.azul_batch_score_moves(env._h, L.PERSP_CURRENT, None, ptr(s), None, None) == L.SUCCESS          # scores only
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy().astype(np.int64), tabs[30:37]) and (b.cpu().numpy() == CANARY).all()
    s.fill_(CANARY)
    assert L.lib.azul_batch_score_moves(env._h, L.PERSP_CURRENT, None, None, ptr(b), None) == L.SUCCESS          # best only
    torch.cuda.synchronize()
    assert np.array_equal(b.cpu().numpy(), best[30:37]) and (s.cpu().numpy() == CANARY).all()
    # refusals, before any launch: both outputs NULL, a perspective that is none of 0 / 1 / CURRENT, a wide batch
    b.fill_(CANARY)
    assert L.lib.azul_batch_score_moves(env._h, L.PERSP_CURRENT, None, None, None, None) == L.ERR_INVALID
    assert b"both NULL" in L.lib.azul_last_error_string()
    for bad in (-1, 3, L.PERSP_MOVER):
        assert L.lib.azul_batch_score_moves(env._h, bad, None, ptr(s), ptr(b), None) == L.ERR_INVALID
        assert b"perspective" in L.lib.azul_last_error_string()
    wide = BatchedAzul(4, players=3, device="cuda", seed=1)
    wide.init()
    ws = torch.full((4, 180), CANARY, dtype=torch.int32, device="cuda")
    wb = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    assert L.lib.azul_batch_score_moves(wide._h, 0, None, ptr(ws), ptr(wb), None) == L.ERR_INVALID
    assert b"wide batch" in L.lib.azul_last_error_string()
    with pytest.raises(L.AzulHipError, match="wide batch"):
        wide.score_moves(0)
    with pytest.raises(L.AzulHipError, match="wide batch"):
        wide.greedy_action()
    torch.cuda.synchronize()
    for t in (s, b, ws, wb):
        assert (t.cpu().numpy() == CANARY).all()


def _replay_with_the_greedy_model(rec0, mt0, pos0, first, pool, action, opp_action, opp_replies, obs, mask, player, reward, done):
    """tests/net_replay.py's loop with the MODEL's greedy choice as the opponent (instead of the recorded answers): the oracle's
    GameRunner(opponent=greedy) fed the recorded agent actions; every env-side record and every traced answer must equal the rollout's."""
    S, R = len(action), opp_action.shape[1]
    assert int(opp_replies.max(initial=0)) <= R, "a step had more replies than the trace holds: raise opponent_trace"
    cur = {"t": 0, "j": 0, "calls": 0, "forced": 0}

    def opponent(s, m):
        a = sm.greedy_of_game(run.q.game)
        assert a >= 0 and m[a], ("greedy answer not legal", cur["t"], cur["j"], a)
        assert a == int(opp_action[cur["t"], cur["j"]]), ("traced opp_action", cur["t"], cur["j"], a, int(opp_action[cur["t"], cur["j"]]))
        assert np.array_equal(s, oz.get_state(run.q.game, run.q.game.current_player - 1))
        cur["j"] += 1
        cur["calls"] += 1
        cur["forced"] += int(run.q.game.current_player == 1)
        return a

    run = oz.NetRunner(opponent, first, pool, rec=rec0, mt=mt0, pos=pos0)
    for t in range(S):
        cur["t"], cur["j"] = t, 0
        m = run.get_valid_moves()
        assert np.array_equal(np.asarray(mask[t]).astype(bool), m), ("mask", t)
        assert np.array_equal(np.asarray(obs[t]).astype(np.int64), run.get_state(0)), ("obs", t)
        assert int(player[t]) == 1 == int(run.q.game.current_player) and int(m.sum()) >= 2, ("player", t)
        a = int(action[t])
        assert 0 <= a < 180 and m[a], ("agent action", t, a)
        rc, rew, dn = run.step(a)
        assert rc == 0 and rew == int(reward[t]) and dn == bool(done[t]), ("reward / done", t, rew, int(reward[t]), dn, int(done[t]))
        if dn:
            assert run.reset() == 0
        assert cur["j"] == int(opp_replies[t]), ("replies", t, cur["j"], int(opp_replies[t]))
    assert np.array_equal(np.asarray(mask[S]).astype(bool), run.get_valid_moves()) and np.array_equal(np.asarray(obs[S]).astype(np.int64), run.get_state(0))
    return run, cur["calls"], cur["forced"]


@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
def test_greedy_rollout_replays_through_the_oracle(ruleset):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    rules, first, pool = RULESETS[ruleset]
    torch.manual_seed(3)
    net = BatchedActorCritic(136, 180, 180)
    T, n = 8, 6
    ro = PolicyRollout(net, n_games=n, window=T, opponent="greedy", opponent_trace=4, rules=rules, seed_base=900)
    assert ro.opponent == "greedy" and not ro.persistent and not ro.use_graph and ro.ring == 1
    env = ro.envs[0]
    start = env.get_records()
    rng0 = [env.get_rng(g) for g in range(n)]
    wins = []
    for _ in range(2):
        tr = ro.run_window()
        ro.synchronize()
        wins.append({k: v.cpu().numpy().copy() for k, v in tr[0].items()})
    finals, (fmt, fpos) = env.get_records(), env.get_rng_range()
    assert (np.concatenate([w["opp_logp"] for w in wins]) == 0).all()
    cat = lambda key, sl: np.concatenate([w[key][sl] for w in wins])
    calls = 0
    for g in range(n):
        slot = lambda key: np.concatenate([w[key][:T, g] for w in wins] + [wins[-1][key][T:T + 1, g]])
        run, c, _ = _replay_with_the_greedy_model(start[g], rng0[g][0], rng0[g][1], first, pool, cat("action", (slice(None), g)),
                                                  cat("opp_action", (slice(None), slice(None), g)), cat("opp_replies", (slice(None), g)),
                                                  slot("obs"), slot("mask"), slot("player"), cat("reward", (slice(None), g)), cat("done", (slice(None), g)))
        calls += c
        assert run.record().tobytes() == finals[g].tobytes(), g
        m_e, idx = run.rng_state()
        assert int(fpos[g]) == idx and np.array_equal(fmt[g], m_e), g
    assert calls >= 2 * T * n // 2                       # the opponent really moved: about one reply per agent step


def test_trainer_against_the_greedy_opponent():
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS, BatchedTrainer
    torch.manual_seed(4)
    tr = BatchedTrainer(BatchedActorCritic(136, 180, 180), opponent="greedy", n_games=8, window=8)
    assert tr.rollout.opponent == "greedy" and tr.rollout.ring == 1 and not tr.rollout.persistent
    rows = [tr.run_batch() for _ in range(2)]
    torch.cuda.synchronize()
    assert tr.learner.updates == 2
    for r in rows:
        assert all(np.isfinite(r[k]) for k in AGENT_STAT_KEYS[1:]), r
