"""The playout kernels under a playout policy on CPU: csrc/azul_selfplay_kernels.hpp (on azul_ops2.hpp -> azul_env2.hpp -> azul_selfplay2.hpp,
with azul_policy.hpp's Philox block, all UNMODIFIED) compiled by g++ and run under the lockstep 64-lane emulation
(tests/hostcheck/simt_playout_policy.cpp, the instantiation taken from the library's selector) against the host model
(tests/playout_policy_model.py).

The states: the shared states of three oracle streams cut into consecutive batches of 1, 2, 3 and 7 records, every run of four batches
given to one of the six (pool, perspective) combinations in turn (playout_moves_model.emulation_chunks) -- ALL 360 at (explore 0, K 1),
each run once, and a fixed subset of 156 at (explore 64, K 2): the first two runs of every combination, all four batch sizes in each
(the emulation at -O0 takes about a second per state there; a test below asserts that the subset holds every class); the 160 arbitrary
in-domain records of tests/domain_records.py per pool and nine `ended` records at (64, 2) in the same batch sizes; the crafted stuck record
in either half beside a game that plays on, and the crafted record whose greedy ply is decided by the action order; an `active` mask with
holes and a canary, each output optional, record bytes unchanged; the same record at two batch positions with equal global id; and the
uniform policy through the new selector against the old model.  The `-m gpu` tests repeat it on the real kernel
(tests/test_gpu_playout_policy.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import domain_records as dr
from tests import playout_moves_model as pm
from tests import playout_policy_model as pp
from tests import score_moves_model as sm
from tests.hostcheck import hostcheck as hc

CANARY = 0x5EED5EED
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(hc.build("libsimt_playout_policy.so"))
        _lib.shp_playout_policy.restype = C.c_int
        _lib.shp_playout_policy.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint32] + [C.c_int] * 4 + [C.c_uint64, C.c_uint32] + [C.c_void_p] * 3
    return _lib


def run(recs, pool, persp, id_base, explore, playouts, policy=pp.GREEDY, active=None, want_sums=True, want_best=True, seed=pp.SEED, call=pp.CALL):
    n = len(recs)
    buf = np.ascontiguousarray(recs, np.uint8).copy()
    keep = buf.copy()
    sums = np.full((n, 180), CANARY, np.int32) if want_sums else None
    best = np.full(n, CANARY, np.int32) if want_best else None
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    assert lib().shp_playout_policy(n, hc.ptr(buf), pool, id_base, persp, playouts, policy, explore, seed, call, hc.ptr(act), hc.ptr(sums),
                                    hc.ptr(best)) == 0
    assert np.array_equal(buf, keep), "the kernel wrote to a record"
    return sums, best


def chunks_of(combo, explore):
    """The batches of a combination: all of pm.emulation_chunks' at explore 0 (the 360 states), the first two runs of four batches (26
    states) at explore 64, where a playout draws and the emulation at -O0 takes about a second per state: 156 states over the six."""
    chunks = pp.emulation_chunks(combo)
    return chunks if explore == 0 else chunks[:8]


@pytest.mark.parametrize("explore,K", pp.CONFIGS)
@pytest.mark.parametrize("combo", range(len(pp.EMULATION_COMBOS)))
def test_table_and_best_equal_the_model(combo, explore, K):
    pool, persp = pp.EMULATION_COMBOS[combo]
    recs = sm.stream_states()[0]
    tabs, best = pp.stream_tables(explore, K, persp)
    chunks = chunks_of(combo, explore)
    assert {n for _, n in chunks} >= {1, 2, 3, 7} and sum(n for _, n in chunks) >= 26
    for lo, n in chunks:
        s, b = run(recs[lo:lo + n], pool, persp, pp.GBASE + lo, explore, K)
        assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]), (lo, n)
        assert np.array_equal(b, best[lo:lo + n]), (lo, n)


def test_the_states_the_emulation_runs_hold_every_class():
    """A condition of the test above: at (0, 1) the six combinations run every shared state once; at (64, 2) their 156 states hold every
    class, a playout with both an explored and a greedy ply among them."""
    states = lambda explore: sorted(i for combo in range(len(pp.EMULATION_COMBOS)) for lo, n in chunks_of(combo, explore) for i in range(lo, lo + n))
    assert states(0) == list(range(360))
    subset = states(64)
    assert len(subset) == len(set(subset)) == 156
    total = pp.census(64, 2, subset)
    assert all(total[name] >= 1 for name in pp.PLY_CLASSES + pp.PLAYOUT_CLASSES + pp.STATE_CLASSES), total


@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_table_and_best_on_arbitrary_in_domain_records_equal_the_model(cfg):
    """The 160 records of tests/domain_records.py (states no game reaches) and 9 `ended` records at (explore 64, K 2), in consecutive batches
    of 1, 2, 3 and 7: greedy_pick2 runs on a register copy that only do_move2 has advanced -- whatif_after2 must price from the copy's own
    lines, floor, wall and score, and score_key must stay monotone for every in-domain score."""
    explore, K = 64, 2
    raw = pp.domain_values(cfg, dr.CPU_N, explore, K)[0]
    tabs, best = pp.domain_tables(cfg, dr.CPU_N, explore, K)
    assert len(raw) == dr.CPU_N + pm.DOMAIN_ENDED and (best[dr.CPU_N:] == -1).any()
    lo, j = 0, 0
    while lo < len(raw):
        n = min(pp.EMULATION_SIZES[j % 4], len(raw) - lo)
        s, b = run(raw[lo:lo + n], cfg[2], pp.PERSP_CURRENT, pp.DOMAIN_GBASE + lo, explore, K)
        assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]), (lo, n, [dr.family_of(i, dr.CPU_N) for i in range(lo, min(lo + n, dr.CPU_N))])
        assert np.array_equal(b, best[lo:lo + n]), (lo, n)
        lo, j = lo + n, j + 1


@pytest.mark.parametrize("n,holes", [(1, [0]), (2, [1]), (3, [0, 2]), (7, [1, 2, 6])])
def test_inactive_rows_keep_the_canary_and_each_output_is_optional(n, holes):
    lo, (explore, K) = 40, (64, 2)
    recs = sm.stream_states()[0][lo:lo + n]
    tabs, best = pp.stream_tables(explore, K)
    tabs, best = tabs[lo:lo + n], best[lo:lo + n]
    active = np.ones(n, np.uint8)
    active[holes] = 0
    on = active != 0
    for want_sums, want_best in ((True, True), (True, False), (False, True)):
        s, b = run(recs, pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + lo, explore, K, active=active, want_sums=want_sums, want_best=want_best)
        if want_sums:
            assert np.array_equal(s[on].astype(np.int64), tabs[on]) and (s[~on] == CANARY).all()
        if want_best:
            assert np.array_equal(b[on], best[on]) and (b[~on] == CANARY).all()


def _want(actions, K, sign=1):
    want = np.full(180, pp.ILLEGAL, np.int64)
    for a, v in actions.items():
        want[a] = sign * K * v
    return want


@pytest.mark.parametrize("explore,K", pp.CONFIGS)
@pytest.mark.parametrize("pool", [pm.oz.POOL_LID, pm.oz.POOL_RANDOM])
def test_the_stuck_record_in_either_half_beside_a_game_that_plays_on(pool, explore, K):
    """Every playout of the stuck record stops at ply 0 (the next player has nothing legal: greedy_pick2 sees an empty mask for that half)
    while the other half of the wave plays on."""
    other = sm.stream_states()[0][3]
    tab_o, best_o = pp.stream_tables(explore, K)[0][3], pp.stream_tables(explore, K)[1][3]
    want = _want(pm.STUCK_ACTIONS, K)
    s, b = run(pm.stuck_record()[None], pool, pp.PERSP_CURRENT, 1, explore, K)
    assert np.array_equal(s[0].astype(np.int64), want) and b[0] == pm.STUCK_BEST
    s, b = run(np.stack([pm.stuck_record(), other]), pool, pp.PERSP_CURRENT, pp.GBASE + 2, explore, K)      # the other state is game GBASE + 3
    assert np.array_equal(s[0].astype(np.int64), want) and b[0] == pm.STUCK_BEST
    assert np.array_equal(s[1].astype(np.int64), tab_o) and b[1] == best_o
    s, b = run(np.stack([other, pm.stuck_record()]), pool, 1, pp.GBASE + 3, explore, K)
    assert np.array_equal(s[1].astype(np.int64), _want(pm.STUCK_ACTIONS, K, -1))
    assert np.array_equal(s[0].astype(np.int64), pp.stream_tables(explore, K, 1)[0][3])


@pytest.mark.parametrize("pool", [pm.oz.POOL_LID, pm.oz.POOL_RANDOM])
def test_the_crafted_records_by_hand(pool):
    """The record whose one greedy ply has six equal values (the first, the floor row, is played), the stuck record and the record one move
    from the end of the round, in one batch of three: the tables derived by hand in the models' docstrings, K = 3 at explore 0."""
    s, b = run(np.stack([pp.tie_ply_record(), pm.last_move_record(), pm.stuck_record()]), pool, pp.PERSP_CURRENT, 9, 0, 3)
    for row, (acts, best) in enumerate(((pp.TIE_PLY_ACTIONS, pp.TIE_PLY_BEST), (pm.LAST_MOVE_ACTIONS, pm.LAST_MOVE_BEST),
                                        (pm.STUCK_ACTIONS, pm.STUCK_BEST))):
        assert np.array_equal(s[row].astype(np.int64), _want(acts, 3)) and b[row] == best, row
    s, b = run(pp.tie_ply_record()[None], pool, 1, 9, 0, 1)
    assert np.array_equal(s[0].astype(np.int64), _want(pp.TIE_PLY_ACTIONS, 1, -1)) and b[0] == 1


def test_a_games_row_follows_its_global_id_not_its_place_in_the_batch():
    recs = sm.stream_states()[0]
    i, (explore, K) = 100, (64, 2)                # (a state whose table the model changes with the global id)
    tabs, best = pp.stream_tables(explore, K)
    # state i as row 0 of a batch of 3 with id_base GBASE + i, and as row 4 of a batch of 7 with id_base GBASE + i - 4: global id GBASE + i both times
    s0, b0 = run(recs[[i, 10, 11]], pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + i, explore, K)
    s1, b1 = run(recs[[20, 21, 22, 23, i, 24, 25]], pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + i - 4, explore, K)
    assert np.array_equal(s0[0], s1[4]) and b0[0] == b1[4]
    assert np.array_equal(s0[0].astype(np.int64), tabs[i]) and b0[0] == best[i]
    # ... another global id gives the state another table where draws decide, and the same table at explore 0
    s2, _ = run(recs[[i]], pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + i + 1, explore, K)
    assert not np.array_equal(s2[0], s0[0])
    s3, _ = run(recs[[i]], pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + i, 0, 1)
    s4, _ = run(recs[[i]], pm.oz.POOL_LID, pp.PERSP_CURRENT, pp.GBASE + i + 1, 0, 1, seed=1, call=2)
    assert np.array_equal(s3, s4) and np.array_equal(s3[0].astype(np.int64), pp.stream_tables(0, 1)[0][i])


@pytest.mark.parametrize("pool", [pm.oz.POOL_LID, pm.oz.POOL_RANDOM])
def test_the_uniform_policy_through_the_new_selector_is_the_old_model(pool):
    """playout_moves_kernel(lid, AZUL_PLAYOUT_UNIFORM) at K = 2: tests/playout_moves_model.py's tables, on 39 shared states in batches of 1, 2,
    3 and 7 (three runs of four batches)."""
    recs = sm.stream_states()[0]
    tabs, best = pm.stream_tables(2)
    lo = 100
    for n in pp.EMULATION_SIZES * 3:
        s, b = run(recs[lo:lo + n], pool, pp.PERSP_CURRENT, pp.GBASE + lo, 0, 2, policy=pp.UNIFORM)
        assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]) and np.array_equal(b, best[lo:lo + n]), (lo, n)
        lo += n
