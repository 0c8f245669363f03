"""Arbitrary in-domain records (tests/domain_records.py: states no game reaches) through the kernels' own code under the lockstep
emulation, against the oracle:
  * azul_x_op_kernel (csrc/azul_rules_x.hpp) on the wide record, for the five (P, D) instantiations and the four rule switches: query (mask,
    flags, the observation from every seat and from the mover's), count_score, move, step incl. the deal (status, record, all 624 words, the
    index), new_round on the record as it is (rule errors incl.), next_player, the RandomAgent sampler on the record's own and on a foreign
    mask, the statistics;
  * azul_op_kernel (two players) for what tests/test_random_states.py leaves out: step, new_round, the sampler, the statistics;
  * azul_score_moves_kernel against tests/score_moves_model.py: three perspectives, both pools, batches of 1, 2, 3 and 7 records;
  * flat self-play from handed-in records, both record formats, the record-snapshot and the padded / packed variant;
  * the overflow records (box = 0, lid = [51] * 5, scoring pushes the lid past 255 tiles before the refill): the oracle's answer.
The GPU runs the same comparisons on whole batches: tests/test_gpu_domain_records.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr
from tests import score_moves_model as sm
from tests import test_hostcheck_rules_x as hx
from tests import test_hostcheck_score_moves as hs
from tests import test_hostcheck_selfplay2 as h2
from tests.hostcheck import hostcheck as hc

N = dr.CPU_N


def _bytes(rec):
    return np.frombuffer(np.asarray(rec).tobytes(), np.uint8).copy()


def _stats_equal(got, want):
    return np.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(want))


# ---- the wide rule book ------------------------------------------------------------------------------------------------------------------------
class WideCall:
    """One emulated azul_x_op_kernel call on a fresh copy of a record and of its stream."""

    def __init__(self, cfg, rec, a):
        self.cfg, self.buf, self.mt, self.pos = cfg, _bytes(rec), a.mt.copy(), np.array([a.pos], np.uint32)

    def __call__(self, op, action=0, **kw):
        P, ext, pool = self.cfg
        return hc.x_op(self.buf, P, oz.FIRST_RANDOM, pool, ext, op, action, self.mt, self.pos, **kw)

    def state(self):
        return self.buf.tobytes(), self.mt, int(self.pos[0])


def check_wide_record(cfg, rec, a, tag):
    P = cfg[0]
    raw = _bytes(rec).tobytes()
    c = WideCall(cfg, rec, a)
    o = c("query", want_mask=True, want_flags=True, want_stats=True, want_obs=0)
    assert np.array_equal(o["mask"].astype(bool), a.mask), tag
    assert (o["flags"] & 3) == a.flags, tag
    assert np.array_equal(o["obs"].astype(np.int64), a.obs[0]), tag
    assert _stats_equal(o["stats"], a.stats), tag
    for p in range(1, P):
        assert np.array_equal(c("query", want_obs=p)["obs"].astype(np.int64), a.obs[p]), tag + (p,)
    assert np.array_equal(c("query", want_obs=P)["obs"].astype(np.int64), a.obs_mover), tag          # (a seat >= P: the player to move)
    assert c.state()[0] == raw and c.state()[2] == a.pos, tag                                         # queries leave the game alone
    c = WideCall(cfg, rec, a)
    c("count_score")
    assert c.state()[0] == a.scored.tobytes(), tag
    for act in a.picks:
        c = WideCall(cfg, rec, a)
        c("move", act)
        assert c.state()[0] == a.moved[act].tobytes(), tag + (act,)
        check_wide_step(cfg, rec, a, act, tag)
    c = WideCall(cfg, rec, a)
    st, want, mt, pos = a.dealt
    assert c("new_round")["status"] == st, tag
    assert c.state()[0] == want.tobytes() and np.array_equal(c.mt, mt) and c.state()[2] == pos, tag
    c = WideCall(cfg, rec, a)
    c("next_player")
    assert c.state()[0] == a.passed.tobytes(), tag
    c = WideCall(cfg, rec, a)
    act, mt, pos = a.action
    assert c("random_action")["action"] == act and np.array_equal(c.mt, mt) and c.state()[2] == pos and c.state()[0] == raw, tag
    c = WideCall(cfg, rec, a)
    act, mt, pos = a.sampled
    assert c("sample_mask", mask_in=a.sample_mask)["action"] == act and np.array_equal(c.mt, mt) and c.state()[2] == pos and c.state()[0] == raw, tag


def check_wide_step(cfg, rec, a, act, tag):
    c = WideCall(cfg, rec, a)
    st, want, mt, pos = a.stepped[act]
    got = c("step", act)["status"]
    assert got == st, tag + (act, got, st)
    assert c.state()[0] == want.tobytes(), tag + (act, "record")
    assert np.array_equal(c.mt, mt) and c.state()[2] == pos, tag + (act, "stream")


@pytest.mark.parametrize("cfg", dr.WIDE_CONFIGS, ids=dr.config_id)
def test_wide_rule_calls_on_arbitrary_records_equal_the_oracle(cfg):
    recs, ans = dr.batch(cfg, N)
    for i, (rec, a) in enumerate(zip(recs, ans)):
        check_wide_record(cfg, rec, a, (dr.config_id(cfg), dr.family_of(i, N), i))


@pytest.mark.parametrize("cfg", dr.WIDE_CONFIGS, ids=dr.config_id)
def test_wide_step_refills_the_bag_with_more_than_255_tiles_like_the_oracle(cfg):
    """Regression: the documented domain is not closed under one step.  box = 0, lid = [51] * 5 is accepted (255 tiles); the round's scoring
    returns 4 tiles per player, the refill (azul.py:81-83) finds 255 + 4 P.  The deal kept the bag's total in eight bits (az::byte_sum5 and
    the byte-wise prefix sums of the sequential draws): ST_BOX_EMPTY or other tiles than the oracle's, without an error.  The totals are plain
    sums now, and a batch of draws from more than 255 tiles is decided by the literal fp64 code (the margin argument of az2::deal_batch2 is for
    T <= 255).  Acceptance is unchanged: records the existing deal tests hand in lie outside the closure bound."""
    P, ext, pool = cfg
    recs = dr.overflow(10, P, dr.displays(cfg), 77)
    for i, (rec, a) in enumerate(zip(recs, dr.answers(recs, cfg, 900))):
        assert a.picks
        for act in a.picks:
            assert a.stepped[act][0] == oz.OK
            check_wide_step(cfg, rec, a, act, (dr.config_id(cfg), "overflow", i))


# ---- the two-player rule kernel: what tests/test_random_states.py leaves out ------------------------------------------------------------------------
def _emu2(pool, rec, a):
    e = hc.EmuBackend(oz.FIRST_RANDOM, pool)
    e.put(rec)
    e.mt[:] = a.mt
    e.pos[0] = a.pos
    return e


def check_two_player_step(pool, rec, a, act, tag):
    e = _emu2(pool, rec, a)
    st, want, mt, pos = a.stepped[act]
    got = e.op_step(act)
    assert got == st, tag + (act, got, st)
    assert e.rec.tobytes() == want.tobytes(), tag + (act, "record")
    assert np.array_equal(e.mt, mt) and int(e.pos[0]) == pos, tag + (act, "stream")


@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_two_player_step_new_round_sampler_and_statistics_equal_the_oracle(cfg):
    pool = cfg[2]
    recs, ans = dr.batch(cfg, N)
    for i, (rec, a) in enumerate(zip(recs, ans)):
        tag = (dr.config_id(cfg), dr.family_of(i, N), i)
        raw = _bytes(rec).tobytes()
        for act in a.picks:
            check_two_player_step(pool, rec, a, act, tag)
        e = _emu2(pool, rec, a)
        st, want, mt, pos = a.dealt
        assert e.op_new_round() == st, tag
        assert e.rec.tobytes() == want.tobytes() and np.array_equal(e.mt, mt) and int(e.pos[0]) == pos, tag
        e = _emu2(pool, rec, a)
        act, mt, pos = a.action
        assert e._op("random_action")["action"] == act and np.array_equal(e.mt, mt) and int(e.pos[0]) == pos and e.rec.tobytes() == raw, tag
        e = _emu2(pool, rec, a)
        act, mt, pos = a.sampled
        assert e.op_sample_mask(a.sample_mask) == act and np.array_equal(e.mt, mt) and int(e.pos[0]) == pos and e.rec.tobytes() == raw, tag
        assert _stats_equal(_emu2(pool, rec, a).op_statistics(), a.stats), tag


def test_two_player_step_refills_the_bag_with_more_than_255_tiles_like_the_oracle():
    """The two-player kernels deal through the same az2::deal_lid2: the equivalent record, the same finding, the same fix."""
    cfg = dr.TWO_CONFIGS[0]
    recs = dr.overflow(10, 2, 5, 77, wide_record=False)
    for i, (rec, a) in enumerate(zip(recs, dr.answers(recs, cfg, 900))):
        assert a.picks
        for act in a.picks:
            assert a.stepped[act][0] == oz.OK
            check_two_player_step(cfg[2], rec, a, act, ("overflow", i))


# ---- azul_score_moves_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persp", [0, 1, sm.PERSP_CURRENT])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_score_moves_on_arbitrary_records_equals_the_model(cfg, persp):
    pool = cfg[2]
    recs = dr.batch(cfg, N)[0]
    raw = np.stack([_bytes(r) for r in recs])
    i = k = 0
    seen = set()
    while i < N:
        n = min((1, 2, 3, 7)[k % 4], N - i)
        k += 1
        scores, best = hs.run(raw[i:i + n], pool, persp)           # (asserts that the records stay unchanged)
        for j in range(n):
            tab = sm.table(raw[i + j], persp, pool)
            assert np.array_equal(scores[j].astype(np.int64), tab), (i + j, n)
            assert int(best[j]) == sm.greedy(tab), (i + j, n)
        seen.add(n)
        i += n
    assert seen >= {1, 2, 3, 7}


# ---- flat self-play from handed-in arbitrary records ---------------------------------------------------------------------------------------------------
GAMES, MOVES = 6, 60


def _spread(n):
    """Six records of a batch: one scattered, one on dense walls, two round ends, two pool edges."""
    q = n // 4
    return [1, q + 1, 2 * q, 2 * q + 3, 3 * q, 3 * q + 4]


@pytest.mark.parametrize("variant", [3, 0], ids=["records", "padded-bits"])
@pytest.mark.parametrize("cfg", dr.WIDE_CONFIGS, ids=dr.config_id)
def test_wide_selfplay_from_handed_in_arbitrary_records_equals_the_oracle(cfg, variant):
    P, ext, pool = cfg
    recs = dr.batch(cfg, N)[0]
    pick = _spread(N)

    def hand_in(streams):
        for s, i in zip(streams, pick):
            s.g = oz.unpack_np(recs[i], pool, ext)

    hx.check_streams(hx.load(), P, oz.FIRST_RANDOM, pool, ext, n=GAMES, T=MOVES, variant=variant, seed0=8100, prepare=hand_in)


@pytest.mark.parametrize("variant", [3, 0], ids=["records", "padded-bits"])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_two_player_selfplay_from_handed_in_arbitrary_records_equals_the_oracle(cfg, variant):
    """(the default instantiation writes nothing for a game a rule error stops, and the oracle's stream raises there: the six records are the
    first of each family pair that the oracle plays MOVES moves from -- the stop itself is tests/test_hostcheck_selfplay2.py's)"""
    pool = cfg[2]
    recs = dr.batch(cfg, N)[0]

    def plays_on(i, g):
        s = oz.Stream(8200 + g, first_player=oz.FIRST_RANDOM, tile_pool=pool)
        s.q = oz.unpack(recs[i], pool, oz.FIRST_RANDOM)
        try:
            s.advance(MOVES, want_records=False)
        except RuntimeError:
            return False
        return True

    pick = []
    for g, start in enumerate(_spread(N)):
        pick.append(next(i for i in range(start, N) if plays_on(i, g)))
    assert len(set(pick)) == GAMES

    def hand_in(streams):
        for s, i in zip(streams, pick):
            s.q = oz.unpack(recs[i], pool, oz.FIRST_RANDOM)

    h2.check_case(h2.load(), oz.FIRST_RANDOM, pool, n=GAMES, T=MOVES, variant=variant, seed0=8200, prepare=hand_in)
