"""The factory draw's window check on the MI355X, through the C ABI: the crafted draws of tests/deal_craft.py -- the K where the integer rule
P_c * 2^53 <= K * T gives another colour than CPython's fp64 arithmetic -- dealt by
  (i)  the rule kernel's new_round (two players; three and four players with 2P + 1 displays), games set with set_records + set_rng_range,
       a crafted game next to a plain one, a plain one next to a crafted one and two crafted ones in the waves;
  (ii) the benchmarked self-play kernel, default instantiation (seed + runner_init only): the 40 words of one round's factory draw
       overwritten in each game's start state, selfplay run past that round -- then once more through set_records (the marking
       instantiation).
Everything is compared with the oracle on the same words: records, all 624 MT words and the index, episode counters.
The CPU counterparts (and the negative control that shows the crafted draws have teeth): tests/test_hostcheck_deal_margins.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import deal_craft as dc
from tests import test_hostcheck_deal_margins as hd

pytestmark = pytest.mark.gpu

LID = {"first_player": "Random", "tile_pool": "Lid"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _plain(ndraws, seed):
    rs = np.random.RandomState(90000 + seed)
    box, lid = hd._random_box(rs, max(ndraws, 20), 200), hd._random_box(rs, 0, 40)
    mt = rs.randint(0, 2 ** 32, size=624, dtype=np.uint64).astype(np.uint32)
    pos = int(rs.randint(0, 624))
    return ("plain", box, lid, pos) + dc.plan_round(box, lid, mt, pos, ndraws, {}, seed=seed)


def _waves(cases, ndraws):
    """Two games per wave: crafted + plain, plain + crafted, crafted + crafted, in turn."""
    games = []
    for i, c in enumerate(cases):
        games += [[c, _plain(ndraws, i)], [_plain(ndraws, i), c], [c, c]][i % 3]
    return games


def _new_round_on_gpu(env, recs, games):
    env.set_records(recs)
    env.set_rng_range(np.stack([g[4] for g in games]), np.array([g[3] for g in games], np.uint32))
    st = env.new_round().cpu().numpy()
    mt, pos = env.get_rng_range()
    return st, env.get_records(), mt, pos


def test_rule_kernel_new_round_on_crafted_draws(torch_cuda):
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    games = _waves(hd.catalogue(20), 20)
    assert len(games) >= 64
    recs = np.array([hd._two_player_record(g[1], g[2]) for g in games], dtype=oz.RECORD_DTYPE)
    st, got, mt, pos = _new_round_on_gpu(BatchedAzul(len(games), rules=LID), recs, games)
    for i, (name, box, lid, p, gmt, draws) in enumerate(games):
        want = hd.oracle_new_round(recs[i], gmt, p)
        assert st[i] == want[0] == 0, (i, name)
        assert got[i].tobytes() == want[1], (i, name)
        assert np.array_equal(mt[i], want[2]) and int(pos[i]) == want[3], (i, name)


@pytest.mark.parametrize("players", [3, 4])
def test_rules_x_new_round_on_crafted_draws(torch_cuda, players):
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    from azul_deep_reinforcement_learning_amd import _lib as L
    ext = oz.EXT_DISPLAYS_2P1
    ndraws = 4 * (2 * players + 1)
    games = _waves(hd.catalogue(ndraws), ndraws)
    s = oz.StreamX(60 + players, players, oz.FIRST_RANDOM, oz.POOL_LID, ext)
    s.advance(3)
    base = s.record().copy()
    recs = np.array([base] * len(games), dtype=oz.RECORD_NP_DTYPE)
    recs["box"] = [g[1] for g in games]
    recs["lid"] = [g[2] for g in games]
    env = BatchedAzul(len(games), rules=LID, players=players, ext_rules=L.RULE_DISPLAYS_2P1)
    st, got, mt, pos = _new_round_on_gpu(env, recs, games)
    for i, (name, box, lid, p, gmt, draws) in enumerate(games):
        g, r = oz.unpack_np(recs[i], oz.POOL_LID, ext), hd._rng(gmt, p)
        assert oz.lib().oz_new_round(C.byref(g), C.byref(r)) == 0 == st[i], (i, name)
        assert got[i].tobytes() == oz.pack_np(g).tobytes(), (i, name)
        assert np.array_equal(mt[i], np.ctypeslib.as_array(r.mt)) and int(pos[i]) == r.idx, (i, name)


# ---- the benchmarked self-play kernel -----------------------------------------------------------------------------------------------------
TARGETS = [{0: None}, {}, {}, {19: None}, {9: None}, {14: None}]     # per game, in turn: crafted / plain siblings, both crafted


def _crafted_starts(seed_base, n):
    """Per game: the start state of oz.Stream(seed_base + g) with the 40 words of one later round's factory draw crafted (a round whose
    words lie in the same generation of the state as the start, so that nothing drawn earlier changes); the move count that ends it."""
    mts, ends, carries = [], [], []
    for g in range(n):
        s = oz.Stream(seed_base + g)
        mt0, idx0 = s.rng_state()
        targets, c, moves = TARGETS[g % len(TARGETS)], hd._clone(s), 0
        while True:
            p = hd._probe(c)
            if p is not None and c.r.words - s.r.words + idx0 + p[0] + 40 <= 624:
                try:
                    mt, draws = hd._plan(p[1], p[2], np.ctypeslib.as_array(c.r.mt), int(c.r.idx), 20, targets, skip=p[0], control=bool(targets))
                    break
                except dc.NoDisagreement:
                    pass
            c.advance(1, want_records=False)
            moves += 1
            assert moves < 400
        first = int(c.r.idx) + p[0]
        assert np.array_equal(np.ctypeslib.as_array(c.r.mt), mt0)           # the same generation as the start
        assert np.array_equal(mt[:first], mt0[:first]) and np.array_equal(mt[first + 40:], mt0[first + 40:])
        mts.append(mt)
        ends.append(moves + 1)
        carries.append(bool(dc.disagreeing(draws)))
    return np.stack(mts), ends, carries


def _oracle_streams(seed_base, mts, steps):
    """The oracle's streams on the crafted start states after `steps` moves, and their records after every move."""
    out, recs = [], []
    for g, mt in enumerate(mts):
        s = oz.Stream(seed_base + g)
        np.ctypeslib.as_array(s.r.mt)[:] = mt
        recs.append(s.advance(steps)["rec_after"])
        out.append(s)
    return out, recs


def _compare(env, streams, tag):
    recs, (mt, pos), cnt = env.get_records(), env.get_rng_range(), env.counters()
    for g, s in enumerate(streams):
        assert recs[g].tobytes() == s.record().tobytes(), (tag, g)
        assert np.array_equal(mt[g], s.rng_state()[0]) and int(pos[g]) == s.rng_state()[1], (tag, g)
        assert int(cnt["episodes"][g]) == s.episodes.value and int(cnt["stuck"][g]) == s.stuck.value, (tag, g)
        assert np.allclose(cnt["stat_sums"][g], s.stats_sum, rtol=0, atol=1e-9), (tag, g)


def test_selfplay_kernel_deals_crafted_draws_like_the_oracle(torch_cuda):
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    n, base = 64, 8800
    mts, ends, carries = _crafted_starts(base, n)
    assert sum(carries) >= 40
    steps = max(ends) + 4
    streams, orecs = _oracle_streams(base, mts, steps)

    env = BatchedAzul(n, rules=LID)                     # default instantiation: nothing handed in
    env.seed(seed_base=base)
    env.runner_init()
    env.runner_init()
    _, pos0 = env.get_rng_range()
    env.set_rng_range(mts, pos0)
    t = env.alloc_trajectory(steps, with_records=True)
    env.selfplay(steps, **t)
    torch_cuda.cuda.synchronize()
    _compare(env, streams, "default")
    recs = t["records"].cpu().numpy()
    for g in range(n):                                  # the record right after the crafted round's deal (a later game end would hide it)
        assert recs[ends[g] - 1, g].tobytes() == orecs[g][ends[g] - 1].tobytes(), g
        assert recs[:, g].tobytes() == orecs[g].tobytes(), g

    env2 = BatchedAzul(n, rules=LID)                    # records handed in: the marking instantiation
    env2.set_records(np.array([oz.Stream(base + g).record() for g in range(n)], dtype=oz.RECORD_DTYPE))
    env2.set_rng_range(mts, pos0)
    env2.selfplay(steps)
    torch_cuda.cuda.synchronize()
    _compare(env2, streams, "marking")
