"""azul_playout_moves_kernel on CPU: csrc/azul_selfplay_kernels.hpp (on azul_ops2.hpp -> azul_env2.hpp -> azul_selfplay2.hpp, with
azul_policy.hpp's Philox block, all UNMODIFIED) compiled by g++ and run under the lockstep 64-lane emulation
(tests/hostcheck/simt_playout_moves.cpp) against the host model (tests/playout_moves_model.py) at K = 2 playouts per move.

The states: ALL 360 shared states of three oracle streams, each run once -- cut into consecutive batches of 1, 2, 3 and 7 records (odd
counts leave the last wave one game), every run of four batches given to one of the six (pool, perspective) combinations in turn
(playout_moves_model.emulation_chunks; tests/test_playout_moves_model.py asserts that they hold every playout class) -- plus the crafted
stuck record; the 160 arbitrary in-domain records of tests/domain_records.py per pool and nine `ended` records, in the same batch sizes
(states no game reaches: an error of the rule book on one of them inside a playout shows only here); then an `active` mask with holes and a canary, each output optional, record bytes unchanged, and the same record at two
batch positions with id_base chosen so that its global id is the same.  The `-m gpu` tests repeat it on the real kernel
(tests/test_gpu_playout_moves.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import domain_records as dr
from tests import playout_moves_model as pm
from tests import score_moves_model as sm
from tests.hostcheck import hostcheck as hc

CANARY = 0x5EED5EED
K = 2
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(hc.build("libsimt_playout_moves.so"))
        _lib.shp_playout_moves.restype = C.c_int
        _lib.shp_playout_moves.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint32] + [C.c_void_p] * 3
    return _lib


def run(recs, pool, persp, id_base, active=None, want_sums=True, want_best=True, playouts=K, seed=pm.SEED, call=pm.CALL):
    n = len(recs)
    buf = np.ascontiguousarray(recs, np.uint8).copy()
    keep = buf.copy()
    sums = np.full((n, 180), CANARY, np.int32) if want_sums else None
    best = np.full(n, CANARY, np.int32) if want_best else None
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    assert lib().shp_playout_moves(n, hc.ptr(buf), pool, id_base, persp, playouts, seed, call, hc.ptr(act), hc.ptr(sums), hc.ptr(best)) == 0
    assert np.array_equal(buf, keep), "the kernel wrote to a record"
    return sums, best


@pytest.mark.parametrize("combo", range(len(pm.EMULATION_COMBOS)))
def test_table_and_best_equal_the_model(combo):
    pool, persp = pm.EMULATION_COMBOS[combo]
    recs = sm.stream_states()[0]
    tabs, best = pm.stream_tables(K, persp)
    chunks = pm.emulation_chunks(combo)
    assert {n for _, n in chunks} >= {1, 2, 3, 7} and sum(n for _, n in chunks) >= 52
    for lo, n in chunks:
        s, b = run(recs[lo:lo + n], pool, persp, pm.GBASE + lo)
        assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]), (lo, n)
        assert np.array_equal(b, best[lo:lo + n]), (lo, n)


@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_table_and_best_on_arbitrary_in_domain_records_equal_the_model(cfg):
    """The 160 records of tests/domain_records.py (mixed and overfull lines, floors at 7, dense walls, round-ending tables, box / lid edges:
    states no game reaches) and 9 `ended` records, in consecutive batches of 1, 2, 3 and 7: the kernel runs do_move2, legal_mask2 and
    count_score2 on a register copy for up to 13 plies from each.  The census is a condition on the oracle's side."""
    raw = pm.domain_values(cfg, dr.CPU_N)[0]
    census = pm.domain_census(cfg, dr.CPU_N, K)
    assert all(census[c] >= 1 for c in pm.DOMAIN_CLASSES), census
    tabs, best = pm.domain_tables(cfg, dr.CPU_N, K)
    assert len(raw) == dr.CPU_N + pm.DOMAIN_ENDED and (best[dr.CPU_N:] == -1).any()
    lo, j = 0, 0
    while lo < len(raw):
        n = min(pm.EMULATION_SIZES[j % 4], len(raw) - lo)
        s, b = run(raw[lo:lo + n], cfg[2], pm.PERSP_CURRENT, pm.DOMAIN_GBASE + lo)          # (run asserts that the records are unchanged)
        assert np.array_equal(s.astype(np.int64), tabs[lo:lo + n]), (lo, n, [dr.family_of(i, dr.CPU_N) for i in range(lo, min(lo + n, dr.CPU_N))])
        assert np.array_equal(b, best[lo:lo + n]), (lo, n)
        lo, j = lo + n, j + 1


@pytest.mark.parametrize("n,holes", [(1, [0]), (2, [1]), (3, [0, 2]), (7, [1, 2, 6])])
def test_inactive_rows_keep_the_canary_and_each_output_is_optional(n, holes):
    lo = 40
    recs = sm.stream_states()[0][lo:lo + n]
    tabs, best = pm.stream_tables(K)
    tabs, best = tabs[lo:lo + n], best[lo:lo + n]
    active = np.ones(n, np.uint8)
    active[holes] = 0
    on = active != 0
    for want_sums, want_best in ((True, True), (True, False), (False, True)):
        s, b = run(recs, pm.oz.POOL_LID, pm.PERSP_CURRENT, pm.GBASE + lo, active, want_sums, want_best)
        if want_sums:
            assert np.array_equal(s[on].astype(np.int64), tabs[on]) and (s[~on] == CANARY).all()
        if want_best:
            assert np.array_equal(b[on], best[on]) and (b[~on] == CANARY).all()


@pytest.mark.parametrize("pool", [pm.oz.POOL_LID, pm.oz.POOL_RANDOM])
def test_the_stuck_record(pool):
    """Every playout stops at ply 0 with the next player unable to move, and is scored there; beside a game that plays on (the two halves of
    the wave stop at different plies), in either half."""
    other = sm.stream_states()[0][3]
    tab_o, best_o = pm.stream_tables(K)[0][3], pm.stream_tables(K)[1][3]
    want = np.full(180, pm.ILLEGAL, np.int64)
    for a, v in pm.STUCK_ACTIONS.items():
        want[a] = K * v
    s, b = run(pm.stuck_record()[None], pool, pm.PERSP_CURRENT, 1)
    assert np.array_equal(s[0].astype(np.int64), want) and b[0] == pm.STUCK_BEST
    s, b = run(np.stack([pm.stuck_record(), other]), pool, pm.PERSP_CURRENT, pm.GBASE + 2)            # the other state is game GBASE + 3
    assert np.array_equal(s[0].astype(np.int64), want) and b[0] == pm.STUCK_BEST
    assert np.array_equal(s[1].astype(np.int64), tab_o) and b[1] == best_o
    s, b = run(np.stack([other, pm.stuck_record()]), pool, 1, pm.GBASE + 3)
    assert np.array_equal(s[1].astype(np.int64), np.where(want == pm.ILLEGAL, pm.ILLEGAL, -want)) and np.array_equal(s[0].astype(np.int64), pm.stream_tables(K, 1)[0][3])


def test_a_games_row_follows_its_global_id_not_its_place_in_the_batch():
    recs = sm.stream_states()[0]
    i = 150
    tabs, best = pm.stream_tables(K)
    # state i as row 0 of a batch of 3 with id_base GBASE + i, and as row 4 of a batch of 7 with id_base GBASE + i - 4: global id GBASE + i both times
    s0, b0 = run(recs[[i, 10, 11]], pm.oz.POOL_LID, pm.PERSP_CURRENT, pm.GBASE + i)
    s1, b1 = run(recs[[20, 21, 22, 23, i, 24, 25]], pm.oz.POOL_LID, pm.PERSP_CURRENT, pm.GBASE + i - 4)
    assert np.array_equal(s0[0], s1[4]) and b0[0] == b1[4]
    assert np.array_equal(s0[0].astype(np.int64), tabs[i]) and b0[0] == best[i]
    # ... and another global id gives the state another table (the draws are keyed by it)
    s2, _ = run(recs[[i]], pm.oz.POOL_LID, pm.PERSP_CURRENT, pm.GBASE + i + 1)
    assert not np.array_equal(s2[0], s0[0])
