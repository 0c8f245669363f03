"""The arbitrary in-domain records of tests/domain_records.py, checked on the oracle alone: what they exercise (the census), that each is a
record (round trip), that no oracle post-state of a call the tests make falls outside the record (nothing is left out), and two negative
controls that show the records tell the rule switches apart.  The kernels meet these records in tests/test_hostcheck_domain_records.py (lockstep
emulation) and tests/test_gpu_domain_records.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr

ALL = dr.WIDE_CONFIGS + dr.TWO_CONFIGS
MIN_PER_CLASS = 8


def _id(cfg):
    return ("two-" if cfg in dr.TWO_CONFIGS else "wide-") + dr.config_id(cfg)


@pytest.mark.parametrize("n", [dr.CPU_N, dr.GPU_N])
@pytest.mark.parametrize("cfg", ALL, ids=_id)
def test_census_round_trip_and_nothing_left_out(cfg, n):
    P, ext, pool = cfg
    recs, ans = dr.batch(cfg, n)                       # (dr.answer raises LeftOut on a record or a post-state that does not pack)
    assert len(recs) == len(ans) == n
    wide = cfg not in dr.TWO_CONFIGS
    assert recs.dtype == (oz.RECORD_NP_DTYPE if wide else oz.RECORD_DTYPE)
    for i, r in enumerate(recs):
        g = dr.Game(r, cfg)
        assert g.pack().tobytes() == r.tobytes(), (i, dr.family_of(i, n))
    if wide:
        D = dr.displays(cfg)
        assert (recs["players"] == P).all() and (recs["n_displays"] == (0 if D == 5 else D)).all()
        assert not recs["xdisplays"][:, max(D - 5, 0):].any() and not recs["reserved0"].any() and not recs["pad"].any()
        for name in ("pattern_lines", "floors", "walls", "score", "first_player_stats", "floor_penalty", "max_combo", "completed_lines"):
            assert not recs[name][:, P:].any(), name
    assert (dr.tiles_in_play(recs, P) <= dr.CLOSURE).all()
    assert (recs["box"].sum(1) <= 255).all() and (recs["lid"].sum(1) <= 255).all() and (recs["floors"] <= 7).all()
    census = dr.census(recs, cfg, ans=ans)
    print(_id(cfg), n, census)
    assert census["left_out"] == 0
    for k in dr.CLASSES:
        if k in dr.unreachable(cfg):
            assert census[k] == 0, k
        else:
            assert census[k] >= MIN_PER_CLASS, (k, census[k])
    # the families are what they say: a round-ending table ends the round on every legal move
    for i in range(n // 2, 3 * n // 4):
        assert not recs[i]["displays"].any() and int((recs[i]["center"][:5] != 0).sum()) == 1
        for act in ans[i].picks:
            g = dr.Game(recs[i], cfg)
            g.move(act)
            assert g.flags() & 1, i


@pytest.mark.parametrize("cfg", ALL, ids=_id)
def test_overflow_records_are_in_the_documented_domain_and_outside_the_closure_bound(cfg):
    P, ext, pool = cfg
    recs = dr.overflow(10, P, dr.displays(cfg), 77, cfg not in dr.TWO_CONFIGS)
    assert (recs["box"].sum(1) == 0).all() and (recs["lid"] == 51).all() and (dr.tiles_in_play(recs, P) > dr.CLOSURE).all()
    ans = dr.answers(recs, cfg, 900)                   # every post-state packs: each colour's lid count stays below 256
    if dr.tracks(cfg):
        refills = sum(int(s[0] == oz.OK and int(s[1]["box"].sum()) + int(s[1]["displays"].sum()) > 255) for a in ans for s in a.stepped.values())
        assert refills >= 8                            # the bag was refilled with more than 255 tiles


def test_negative_control_end_bonus_switch_changes_scores_on_dense_walls():
    cfg = dr.WIDE_CONFIGS[0]
    P, ext, pool = cfg
    recs, ans = dr.batch(cfg, dr.CPU_N)
    differ = 0
    for i in range(dr.CPU_N // 4, dr.CPU_N // 2):      # the dense-wall family
        g = dr.Game(recs[i], (P, ext | dr.END_BONUS, pool))
        g.count_score()
        differ += int(not np.array_equal(g.pack()["score"], ans[i].scored["score"]))
    assert differ >= MIN_PER_CLASS


def test_negative_control_lid_and_random_pool_deal_differently_on_round_ends():
    cfg = dr.WIDE_CONFIGS[0]
    P, ext, pool = cfg
    recs, ans = dr.batch(cfg, dr.CPU_N)
    differ = dealt = 0
    for i in range(dr.CPU_N // 2, 3 * dr.CPU_N // 4):  # the round-end family
        a = ans[i]
        act = a.picks[0]
        st, rec, mt, pos = a.stepped[act]
        if st != oz.OK or (int(rec["flags"]) >> 6) & 1:
            continue
        dealt += 1
        g = dr.Game(recs[i], (P, ext, oz.POOL_RANDOM))
        r = oz.Rng()
        oz.lib().oz_rng_set(C.byref(r), a.mt.ctypes.data_as(C.POINTER(C.c_uint32)), a.pos)
        assert g.step(act, r) == oz.OK
        differ += int(not np.array_equal(g.pack()["displays"], rec["displays"]))
    assert dealt >= MIN_PER_CLASS and differ >= MIN_PER_CLASS
