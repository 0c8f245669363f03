"""azul_batch_mp_score_moves on the MI355X: the table and `best` of the shared states of tests/mp_score_moves_model.py (three oracle
streams, arbitrary in-domain records, a game before its first round) against that model for the five shapes (P, D) = (2, 5), (3, 5),
(3, 7), (4, 5), (4, 9) at batch sizes 1, 2, 3 and 33, every perspective, with the games untouched; the optional outputs and the refusals;
PolicyRollout(players=P, opponent="greedy_margin") replayed game by game through tests/mp_net_model.MPNetRunner with the model's greedy
choice as every other seat; a BatchedTrainer smoke run.  The CPU suite runs the same kernel under the lockstep emulation
(tests/test_hostcheck_mp_score_moves.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as oz
from tests import mp_score_moves_model as mm

pytestmark = pytest.mark.gpu
CANARY = 0x5EED5EED
IDS = [mm.shape_id(s) for s in mm.SHAPES]


def rules_of(shape):
    P, ext, pool, first = shape
    r = {"first_player": "Random" if first == oz.FIRST_RANDOM else first, "tile_pool": "Lid" if pool == oz.POOL_LID else "Random"}
    if ext & oz.EXT_DISPLAYS_2P1:
        r["displays"] = "2P+1"
    if ext & oz.EXT_END_BONUS:
        r["bonuses"] = "end"
    if ext & oz.EXT_SHORT_DEAL:
        r["short_deal"] = True
    return r


def _batch(recs, shape):
    from azul_deep_reinforcement_learning_amd import MultiplayerAzul
    env = MultiplayerAzul(len(recs), rules=rules_of(shape), players=shape[0], device="cuda", seed=77)
    env.set_records(np.ascontiguousarray(recs).view(env.record_dtype).reshape(-1))
    return env


def _snapshot(env):
    c = env.counters()
    mt, pos = env.get_rng_range()
    return env.get_records().tobytes(), mt.tobytes(), pos.tobytes(), c["episodes"].tobytes(), c["stuck"].tobytes(), c["stat_sums"].tobytes()


def _chunks(n):
    """Windows over the shared states: one per small size, placed in different parts of the streams, the domain records and the game
    before its first round; at 33 every state, so that the four sizes together cover every class of the census whatever the shape."""
    if n < 33:
        return [slice(lo, lo + n) for lo in ({1: 119, 2: 57, 3: 200}[n], mm.N_STATES - n, mm.N_STREAM + 7 * n)]
    return [slice(i, i + 33) for i in range(0, mm.N_STATES - 33, 33)] + [slice(mm.N_STATES - 33, mm.N_STATES)]


@pytest.mark.parametrize("n", [1, 2, 3, 33])
@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_table_and_best_equal_the_model_and_the_games_are_untouched(i, n):
    from azul_deep_reinforcement_learning_amd import _lib as L
    shape = mm.SHAPES[i]
    NA, recs = mm.num_actions(shape), mm.states(i)
    chunks = _chunks(n)
    assert n < 33 or set(range(mm.N_STATES)) == {g for sl in chunks for g in range(sl.start, sl.stop)}
    for sl in chunks:
        env = _batch(recs[sl], shape)
        assert env.num_actions == NA
        before = _snapshot(env)
        for persp in mm.perspectives(shape):
            tabs, best = mm.tables(i, persp)
            s, b = env.score_moves(persp)
            assert s.dtype == torch.int32 and tuple(s.shape) == (n, NA) and b.dtype == torch.int32 and tuple(b.shape) == (n,)
            assert np.array_equal(s.cpu().numpy().astype(np.int64), tabs[sl]), (sl, persp)
            assert np.array_equal(b.cpu().numpy(), best[sl]), (sl, persp)
        tabs, best = mm.tables(i, L.PERSP_MOVER)
        assert np.array_equal(env.score_moves()[1].cpu().numpy(), best[sl]), sl              # the default perspective is the mover's
        assert np.array_equal(env.greedy_action().cpu().numpy(), best[sl]), sl
        # the legal mask is where the table holds a score
        assert np.array_equal(env.get_valid_moves().cpu().numpy().astype(bool), mm.tables(i, 0)[0][sl] != mm.ILLEGAL)
        # an active mask with holes: the rows of the other games keep what they held
        active = torch.tensor([(g % 3) != 1 for g in range(n)], dtype=torch.uint8, device="cuda")
        s = torch.full((n, NA), CANARY, dtype=torch.int32, device="cuda")
        b = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
        env.score_moves(L.PERSP_MOVER, active=active, scores=s, best=b)
        g = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
        env.greedy_action(active=active, out=g)
        on = active.cpu().numpy() != 0
        s, b, g = s.cpu().numpy(), b.cpu().numpy(), g.cpu().numpy()
        assert np.array_equal(s[on].astype(np.int64), tabs[sl][on]) and (s[~on] == CANARY).all()
        assert np.array_equal(b[on], best[sl][on]) and (b[~on] == CANARY).all()
        assert np.array_equal(g, b)
        assert _snapshot(env) == before, "score_moves changed records, MT19937 state or counters"


def test_a_best_move_numbered_256_or_above_on_nine_displays():
    i = len(mm.SHAPES) - 1
    best = mm.tables(i, mm.PERSP_MOVER)[1]
    high = np.flatnonzero(best >= 256)
    assert len(high) >= 3
    env = _batch(mm.states(i)[high], mm.SHAPES[i])
    got = env.greedy_action().cpu().numpy()
    assert np.array_equal(got, best[high]) and (got >= 256).all()


@pytest.mark.parametrize("i", range(len(mm.SHAPES)), ids=IDS)
def test_optional_outputs_and_refusals(i):
    from azul_deep_reinforcement_learning_amd import BatchedAzul, _lib as L
    shape = mm.SHAPES[i]
    P, NA = shape[0], mm.num_actions(shape)
    sl = slice(30, 37)
    tabs, best = mm.tables(i, L.PERSP_MOVER)
    env = _batch(mm.states(i)[sl], shape)
    n = 7
    ptr = lambda t: C.c_void_p(t.data_ptr())
    s = torch.full((n, NA), CANARY, dtype=torch.int32, device="cuda")
    b = torch.full((n,), CANARY, dtype=torch.int32, device="cuda")
    assert L.lib.azul_batch_mp_score_moves(env._h, L.PERSP_MOVER, None, ptr(s), None, None) == L.SUCCESS         # scores only
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy().astype(np.int64), tabs[sl]) and (b.cpu().numpy() == CANARY).all()
    s.fill_(CANARY)
    assert L.lib.azul_batch_mp_score_moves(env._h, L.PERSP_MOVER, None, None, ptr(b), None) == L.SUCCESS         # best only
    torch.cuda.synchronize()
    assert np.array_equal(b.cpu().numpy(), best[sl]) and (s.cpu().numpy() == CANARY).all()
    # refusals, before any launch: a NULL batch, both outputs NULL, a perspective that is no seat and not the mover, a two-player batch
    b.fill_(CANARY)
    assert L.lib.azul_batch_mp_score_moves(None, 0, None, ptr(s), ptr(b), None) == L.ERR_INVALID
    assert b"batch is NULL" in L.lib.azul_last_error_string()
    assert L.lib.azul_batch_mp_score_moves(env._h, L.PERSP_MOVER, None, None, None, None) == L.ERR_INVALID
    assert b"both NULL" in L.lib.azul_last_error_string()
    for bad in (-1, P, 5, 6, 8):
        assert L.lib.azul_batch_mp_score_moves(env._h, bad, None, ptr(s), ptr(b), None) == L.ERR_INVALID
        assert b"perspective" in L.lib.azul_last_error_string()
    two = BatchedAzul(4, device="cuda", seed=1)
    two.runner_init()
    ts = torch.full((4, 180), CANARY, dtype=torch.int32, device="cuda")
    tb = torch.full((4,), CANARY, dtype=torch.int32, device="cuda")
    assert L.lib.azul_batch_mp_score_moves(two._h, 0, None, ptr(ts), ptr(tb), None) == L.ERR_INVALID
    msg = L.lib.azul_last_error_string()
    assert b"two-player batch of 128-byte records" in msg and b"use azul_batch_score_moves" in msg
    torch.cuda.synchronize()
    for t in (s, b, ts, tb):
        assert (t.cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("i", [1, 4], ids=[IDS[1], IDS[4]])
def test_greedy_margin_rollout_replays_through_the_model(i):
    """Every game of two windows replayed through MPNetRunner.reset_with / step_with from its seed: the model's opening leads to the
    rollout's starting record and MT19937 state; the opponent callback is the model's greedy choice on the runner's own game; every
    observation, mask, reward, done, reply count and traced answer equals the rollout's, and so do the final records and streams."""
    from azul_deep_reinforcement_learning_amd import PolicyRollout, _lib as L
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    from tests.mp_net_model import MPNetRunner
    shape = mm.SHAPES[i]
    P, ext, pool, first = shape
    rules = rules_of(shape)
    n_obs, n_act = batch_shape(P, rules)
    torch.manual_seed(3 + i)
    T, n, R = 8, 6, 48
    ro = PolicyRollout(BatchedActorCritic(n_obs, n_act, 180), players=P, n_games=n, window=T, opponent="greedy_margin", opponent_trace=R,
                       rules=rules, seed_base=900)
    assert ro.opponent == "greedy_margin" and ro.cut and not ro.fused_wide and not ro.use_graph and ro.ring == 1
    assert not hasattr(ro, "ow1t")                                          # no opponent weights are staged
    env = ro.envs[0]
    start = env.get_records().view(np.uint8).reshape(n, 256)
    mt0, pos0 = env.get_rng_range()
    wins = []
    for _ in range(2):
        tr = ro.run_window()
        ro.synchronize()
        wins.append({k: v.cpu().numpy().copy() for k, v in tr[0].items()})
    finals, (fmt, fpos) = env.get_records().view(np.uint8).reshape(n, 256), env.get_rng_range()
    assert (np.concatenate([w["opp_logp"] for w in wins]) == 0).all()
    replies = 0
    for g in range(n):
        m = MPNetRunner(P, first, pool, ext, seed=900 + g)
        trace = {"want": None, "j": 0}

        def answer(obs, mask, player, m=m, trace=trace):
            a = mm.greedy_of_game(m.g, P)
            assert a >= 0 and mask[a], ("greedy answer not legal", g, a)
            if trace["want"] is not None:
                assert trace["j"] < R and a == int(trace["want"][trace["j"]]), ("traced opp_action", g, trace["j"], a)
            trace["j"] += 1
            return a

        assert m.runner_init() == 0 and m.reset_with(answer) == 0
        assert np.array_equal(m.record(), start[g]), g
        assert np.array_equal(m.rng_state()[0], mt0[g]) and m.rng_state()[1] == int(pos0[g]), g
        for w, win in enumerate(wins):
            for t in range(T):
                assert np.array_equal(win["obs"][t, g], m.obs(0).astype(np.float32)), (g, w, t)
                assert np.array_equal(win["mask"][t, g].astype(bool), m.mask()), (g, w, t)
                assert int(win["player"][t, g]) == int(m.g.current_player), (g, w, t)
                trace["want"], trace["j"] = win["opp_action"][t, :, g], 0
                st, rew, dn, rep = m.step_with(int(win["action"][t, g]), answer)
                assert (st, rew, dn, rep) == (0, int(win["reward"][t, g]), int(win["done"][t, g]), int(win["opp_replies"][t, g])), (g, w, t)
                replies += trace["j"]
            assert np.array_equal(win["obs"][T, g], m.obs(0).astype(np.float32)) and np.array_equal(win["mask"][T, g].astype(bool), m.mask())
        assert np.array_equal(m.record(), finals[g]), g
        assert np.array_equal(m.rng_state()[0], fmt[g]) and m.rng_state()[1] == int(fpos[g]), g
    assert replies >= 2 * T * n                              # the opponents really moved: at least one reply per agent step on average


def test_trainer_against_the_greedy_margin_opponent():
    from azul_deep_reinforcement_learning_amd.batch import batch_shape
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS, BatchedTrainer
    torch.manual_seed(4)
    n_obs, n_act = batch_shape(3, {})
    tr = BatchedTrainer(BatchedActorCritic(n_obs, n_act, 180), players=3, opponent="greedy_margin", n_games=8, window=8)
    assert tr.rollout.opponent == "greedy_margin" and tr.rollout.ring == 1 and not tr.rollout.fused_wide
    rows = [tr.run_batch() for _ in range(2)]
    torch.cuda.synchronize()
    assert tr.learner.updates == 2
    for r in rows:
        print(r)
        assert all(np.isfinite(r[k]) for k in AGENT_STAT_KEYS[1:]), r
