"""Arbitrary in-domain records (tests/domain_records.py: states no game reaches) on the MI355X through BatchedAzul, one batch per
config, against the oracle -- the comparisons of tests/test_hostcheck_domain_records.py on the real kernels:
  * 256 records through the rule entries: mask, flags, observations from every seat and from the mover's, statistics, the score preview
    (azul_batch_score_preview / azul_batch_mp_score_preview), count_score, move, step incl. the deal (status, record, 624 words, index),
    new_round, next_player, the sampler on the game's own and on a foreign mask -- the five (P, D) instantiations of the wide rule book
    with its four rule switches, and the two-player record with both pools;
  * 257 records through score_moves / greedy_action (the last wave holds one game);
  * 33 games x 64 moves of flat self-play from handed-in records, with record snapshots and without outputs;
  * set_state's refusals for wide records, one record per clause of record_in_domain;
  * the overflow records (the refill finds more than 255 tiles): the oracle's answer -- acceptance did not change, the deal's totals did.
Every action and every stream index is checked on the host before a launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle as oz
from tests import domain_records as dr
from tests import score_moves_model as sm
from tests import wide_stream_cases as W

pytestmark = pytest.mark.gpu

N = dr.GPU_N
ALL = dr.WIDE_CONFIGS + dr.TWO_CONFIGS


def _id(cfg):
    return ("two-" if cfg in dr.TWO_CONFIGS else "wide-") + dr.config_id(cfg)


def make_env(cfg, n):
    from azul_deep_reinforcement_learning_amd import BatchedAzul, _lib as L
    from azul_deep_reinforcement_learning_amd.multiplayer import MultiplayerAzul
    P, ext, pool = cfg
    rules = W.device_rules(oz.FIRST_RANDOM, pool)
    assert (L.RULE_DISPLAYS_2P1, L.RULE_END_BONUS, L.RULE_SHORT_DEAL, L.RULE_FINITE_BAG) == (dr.DISPLAYS_2P1, dr.END_BONUS, dr.SHORT_DEAL, dr.FINITE_BAG)
    if cfg in dr.TWO_CONFIGS:
        env = BatchedAzul(n, rules=rules)
        assert not env.wide
    else:
        env = MultiplayerAzul(n, rules=rules, players=P, ext_rules=ext)
        assert env.wide and env.displays == dr.displays(cfg)
    return env


def hand_in(env, recs, ans):
    pos = np.array([a.pos for a in ans], np.uint32)
    assert (pos <= 624).all()
    env.set_records(recs)
    env.set_rng_range(np.stack([a.mt for a in ans]), pos)


def same_streams(env, want, on, tag):
    """want[g] = (..., words, index) for the games in `on`."""
    mt, pos = env.get_rng_range()
    for g in on:
        assert np.array_equal(mt[g], want[g][-2]) and int(pos[g]) == want[g][-1], tag + (g, "stream")


def same_records(env, want, on, tag):
    got = env.get_records()
    for g in on:
        assert got[g].tobytes() == want[g].tobytes(), tag + (g, "record")


@pytest.mark.parametrize("cfg", ALL, ids=_id)
def test_rule_entries_on_arbitrary_records_equal_the_oracle(cfg):
    from azul_deep_reinforcement_learning_amd import _lib as L
    P = cfg[0]
    recs, ans = dr.batch(cfg, N)
    env = make_env(cfg, N)
    NA = env.num_actions
    every = range(N)
    tag = (_id(cfg),)
    hand_in(env, recs, ans)

    # -- the queries: nothing moves
    mask = env.get_valid_moves().cpu().numpy()
    obs = [env.get_state(p).cpu().numpy().astype(np.int64) for p in range(P)]
    obs_mover = env.get_state(L.PERSP_MOVER).cpu().numpy().astype(np.int64)
    flags = env.flags().cpu().numpy()
    stats = env.statistics().cpu().numpy()
    phi = env.score_preview().cpu().numpy()
    for g, a in enumerate(ans):
        assert np.array_equal(mask[g], a.mask), tag + (g, "mask")
        for p in range(P):
            assert np.array_equal(obs[p][g], a.obs[p]), tag + (g, "obs", p)
        assert np.array_equal(obs_mover[g], a.obs_mover), tag + (g, "obs mover")
        assert (int(flags[g]) & 3) == a.flags, tag + (g, "flags")
        assert np.allclose(stats[g], a.stats, rtol=0, atol=1e-12, equal_nan=True) and np.array_equal(np.isnan(stats[g]), np.isnan(a.stats)), tag + (g, "stats")
        assert int(phi[g]) == a.phi, tag + (g, "preview")
    same_records(env, recs, every, tag + ("queries",))
    same_streams(env, [(a.mt, a.pos) for a in ans], every, tag + ("queries",))

    # -- count_score, next_player, new_round (rule errors incl.)
    env.count_score()
    same_records(env, [a.scored for a in ans], every, tag + ("count_score",))
    env.set_records(recs)
    env.next_player()
    same_records(env, [a.passed for a in ans], every, tag + ("next_player",))
    env.set_records(recs)
    st = env.new_round().cpu().numpy()
    for g, a in enumerate(ans):
        assert int(st[g]) == a.dealt[0], tag + (g, "new_round status")
    same_records(env, [a.dealt[1] for a in ans], every, tag + ("new_round",))
    same_streams(env, [a.dealt for a in ans], every, tag + ("new_round",))

    # -- move and step on the first, middle and last legal action (games with fewer picks sit the later rounds out)
    for k in range(3):
        on = [g for g, a in enumerate(ans) if len(a.picks) > k]
        assert on
        actions = np.array([a.picks[k] if len(a.picks) > k else 0 for a in ans], np.int32)
        active = np.array([len(a.picks) > k for a in ans], np.uint8)
        assert ((actions >= 0) & (actions < NA)).all() and all(ans[g].mask[actions[g]] for g in on)
        hand_in(env, recs, ans)
        env.move(actions, active=active)
        same_records(env, [a.moved.get(int(actions[g])) for g, a in enumerate(ans)], on, tag + ("move", k))
        hand_in(env, recs, ans)
        st = env.azul_step(actions, active=active).cpu().numpy()
        want = [a.stepped.get(int(actions[g])) for g, a in enumerate(ans)]
        for g in on:
            assert int(st[g]) == want[g][0], tag + (g, "step status", k)
        same_records(env, [w and w[1] for w in want], on, tag + ("step", k))
        same_streams(env, want, on, tag + ("step", k))
        off = [g for g in every if g not in on]
        same_records(env, recs, off, tag + ("inactive", k))
        same_streams(env, [(a.mt, a.pos) for a in ans], off, tag + ("inactive", k))

    # -- the sampler: the game's own mask, a foreign mask
    hand_in(env, recs, ans)
    act = env.random_action().cpu().numpy()
    for g, a in enumerate(ans):
        assert int(act[g]) == a.action[0], tag + (g, "random_action")
    same_streams(env, [a.action for a in ans], every, tag + ("random_action",))
    hand_in(env, recs, ans)
    act = env.sample_mask(np.stack([a.sample_mask for a in ans])).cpu().numpy()
    for g, a in enumerate(ans):
        assert int(act[g]) == a.sampled[0], tag + (g, "sample_mask")
    same_streams(env, [a.sampled for a in ans], every, tag + ("sample_mask",))
    same_records(env, recs, every, tag + ("sampler",))
    torch.cuda.synchronize()


@pytest.mark.parametrize("cfg", ALL, ids=_id)
def test_step_refills_the_bag_with_more_than_255_tiles_like_the_oracle(cfg):
    """The overflow records: in the documented domain, outside the closure bound.  set_state accepts them as before (records of the existing
    deal tests lie outside the bound too); the deal's totals are plain sums now, so the oracle's answer comes out."""
    P = cfg[0]
    n = 10
    recs = dr.overflow(n, P, dr.displays(cfg), 77, cfg not in dr.TWO_CONFIGS)
    ans = dr.answers(recs, cfg, 900)
    env = make_env(cfg, n)
    for k in range(2):
        on = [g for g, a in enumerate(ans) if len(a.picks) > k]
        actions = np.array([a.picks[k] if len(a.picks) > k else 0 for a in ans], np.int32)
        active = np.array([len(a.picks) > k for a in ans], np.uint8)
        assert on and ((actions >= 0) & (actions < env.num_actions)).all() and all(ans[g].mask[actions[g]] for g in on)
        hand_in(env, recs, ans)
        st = env.azul_step(actions, active=active).cpu().numpy()
        want = [a.stepped.get(int(actions[g])) for g, a in enumerate(ans)]
        for g in on:
            assert want[g][0] == oz.OK and int(st[g]) == oz.OK, (_id(cfg), g, k)
        same_records(env, [w and w[1] for w in want], on, (_id(cfg), "overflow", k))
        same_streams(env, want, on, (_id(cfg), "overflow", k))


# ---- score_moves / greedy_action ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_score_moves_and_greedy_action_on_257_arbitrary_records(cfg):
    from azul_deep_reinforcement_learning_amd import _lib as L
    pool = cfg[2]
    n = 257
    recs = dr.two_player(260, 4600 + pool)[:n]
    assert (dr.tiles_in_play(recs, 2) <= dr.CLOSURE).all()
    env = make_env(cfg, n)
    env.set_records(recs)
    for persp in (0, 1, sm.PERSP_CURRENT):
        scores, best = env.score_moves(persp)
        scores, best = scores.cpu().numpy().astype(np.int64), best.cpu().numpy()
        for g in range(n):
            tab = sm.table(recs[g], persp, pool)
            assert np.array_equal(scores[g], tab), (persp, g)
            assert int(best[g]) == sm.greedy(tab), (persp, g)
        if persp == sm.PERSP_CURRENT:
            assert np.array_equal(env.greedy_action().cpu().numpy(), best)
    assert L.SCORE_ILLEGAL == sm.ILLEGAL
    assert env.get_records().tobytes() == recs.tobytes()


# ---- flat self-play from handed-in records ---------------------------------------------------------------------------------------------------------------
GAMES, MOVES = 33, 64


def _spread(n, k):
    """k records spread evenly over a batch of four families."""
    return [(i * n) // k for i in range(k)]


@pytest.mark.parametrize("variant", ["records", "none"])
@pytest.mark.parametrize("cfg", dr.WIDE_CONFIGS, ids=dr.config_id)
def test_wide_selfplay_from_handed_in_arbitrary_records_equals_the_oracle(cfg, variant):
    from tests.test_gpu_wide_selfplay_edges import launch
    P, ext, pool = cfg
    recs, ans = dr.batch(cfg, N)
    pick = _spread(N, GAMES)
    wcfg = (P, ext, oz.FIRST_RANDOM, pool)
    streams = []
    for g, i in enumerate(pick):
        s = W.new_stream(8300 + g, wcfg)
        s.g = oz.unpack_np(recs[i], pool, ext)
        W.rebase(s)
        streams.append(s)
    env = make_env(cfg, GAMES)
    env.set_records(recs[pick])
    pos = np.array([s.rng_state()[1] for s in streams], np.uint32)
    assert (pos <= 624).all()
    env.set_rng_range(np.stack([s.rng_state()[0] for s in streams]), pos)
    env.reset_counters()
    got = launch(env, MOVES, variant)
    for g, s in enumerate(streams):
        W.compare(W.play_oracle(s, MOVES), got, g, (dr.config_id(cfg), variant, pick[g]))


@pytest.mark.parametrize("variant", ["records", "none"])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_two_player_selfplay_from_handed_in_arbitrary_records_equals_the_oracle(cfg, variant):
    """(the records are the first from each starting point that the oracle plays MOVES moves from: a game that a rule error stops is
    tests/test_gpu_selfplay.py's)"""
    pool = cfg[2]
    recs, ans = dr.batch(cfg, N)

    def stream(i, g):
        s = oz.Stream(8400 + g, first_player=oz.FIRST_RANDOM, tile_pool=pool)
        s.q = oz.unpack(recs[i], pool, oz.FIRST_RANDOM)
        s.stuck.value = s.episodes.value = 0
        s.stats_sum[:] = 0
        return s

    def plays_on(i, g):
        try:
            stream(i, g).advance(MOVES, want_records=False)
        except RuntimeError:
            return False
        return True

    pick = [next(i for i in range(start, N) if plays_on(i, g)) for g, start in enumerate(_spread(N, GAMES))]
    streams = [stream(i, g) for g, i in enumerate(pick)]
    env = make_env(cfg, GAMES)
    env.set_records(recs[pick])
    pos = np.array([s.rng_state()[1] for s in streams], np.uint32)
    assert (pos <= 624).all()
    env.set_rng_range(np.stack([s.rng_state()[0] for s in streams]), pos)
    env.reset_counters()
    t = env.alloc_trajectory(MOVES, with_records=True) if variant == "records" else {}
    env.selfplay(MOVES, **t)
    torch.cuda.synchronize()
    final, (mt, pos), cnt = env.get_records(), env.get_rng_range(), env.counters()
    for g, s in enumerate(streams):
        o = s.advance(MOVES)
        tag = (dr.config_id(cfg), variant, g, pick[g])
        if t:
            assert np.array_equal(t["mask"][:, g].cpu().numpy(), o["mask"]) and np.array_equal(t["action"][:, g].cpu().numpy(), o["action"]), tag
            assert np.array_equal(t["reward"][:, g].cpu().numpy(), o["reward"]) and np.array_equal(t["done"][:, g].cpu().numpy(), o["done"]), tag
            assert t["records"][:, g].cpu().numpy().tobytes() == o["rec_after"].tobytes(), tag
        assert final[g].tobytes() == s.record().tobytes(), tag
        assert np.array_equal(mt[g], s.rng_state()[0]) and int(pos[g]) == s.rng_state()[1], tag
        assert int(cnt["episodes"][g]) == s.episodes.value and int(cnt["stuck"][g]) == s.stuck.value, tag
        # (an episode that ends with no first-player count at all -- only a handed-in record can -- sums 0 / 0: NaN on both sides)
        assert np.allclose(cnt["stat_sums"][g], s.stats_sum, rtol=0, atol=1e-9, equal_nan=True), tag
        assert np.array_equal(np.isnan(cnt["stat_sums"][g]), np.isnan(s.stats_sum)), tag


# ---- set_state's refusals, wide records --------------------------------------------------------------------------------------------------------------------
def _refused(P, D):
    """(clause, edit of a record) -- one per clause of record_in_domain."""
    def player_field(r):
        r["flags"] = (P + 1) | (1 << 3)

    def next_first_player_field(r):
        r["flags"] = 1 | ((P + 1) << 3)

    def floor(r):
        r["floors"][P - 1] = 8

    def wall(r):
        r["walls"][P - 1] |= 1 << 25

    def box(r):
        r["box"] = [52, 51, 51, 51, 51]

    def lid(r):
        r["lid"] = [0, 0, 0, 1, 255]

    def players_byte(r):
        r["players"] = P + 1 if P < 4 else 3

    def displays_byte(r):
        r["n_displays"] = 7 if D != 7 else 0

    return [player_field, next_first_player_field, floor, wall, box, lid, players_byte, displays_byte]


@pytest.mark.parametrize("cfg", [dr.WIDE_CONFIGS[0], dr.WIDE_CONFIGS[3], dr.WIDE_CONFIGS[4]], ids=dr.config_id)
def test_set_state_refuses_each_clause_for_wide_records_and_leaves_the_batch_alone(cfg):
    from azul_deep_reinforcement_learning_amd import _lib as L
    P = cfg[0]
    recs = dr.batch(cfg, N)[0]
    env = make_env(cfg, 4)
    env.set_records(recs[:4])
    for edit in _refused(P, dr.displays(cfg)):
        bad = recs[4:8].copy()
        edit(bad[2])                                     # the third of four: nothing of the call may land
        rc = L.lib.azul_batch_set_state(env._h, 0, 4, bad.ctypes.data_as(C.c_void_p), env._stream())
        assert rc == L.ERR_RANGE, (edit.__name__, rc)
        assert env.get_records().tobytes() == recs[:4].tobytes(), edit.__name__
        with pytest.raises(L.AzulHipError):
            env.set_records(bad)
    env.set_records(recs[4:8])                           # the same records without the edit are accepted
    assert env.get_records().tobytes() == recs[4:8].tobytes()
