"""The ARENA inside the wide window kernel on CPU: azul_x_policy_rollout_vs_kernel<3, 5, true, true> (csrc/azul_rollout2.hpp, compiled
UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_x_rollout_arena.cpp) against the single-opponent
kernel (simt_x_rollout_vs.cpp: sxv_rollout) run once per ordered pair with that pair's weights.  Three players on five displays, 19 games -- a
full 16-game group and a ragged group of three -- five steps, general weights, a pool of two, pairs (agent, opponent) [(1, 0), (0, 1)]: every
output buffer, record, MT19937 state, counter and trace of the games of a group must equal its pair's single-opponent run BYTE FOR BYTE.
Also: a pool of one equals the single-opponent kernel on all games; a member named by no group is never read (NaN poison); a member past the
pool is read as the last one."""
import ctypes as C

import numpy as np
import pytest

from tests.hostcheck import hostcheck
from tests.test_hostcheck_x_rollout import ptr
from tests.test_hostcheck_x_rollout_league import (CASES, GROUP, KEYS, N, fresh, games, head_args, load_vs, member_weights, pointers,
                                                   tail_args)

PAIRS = [(1, 0), (0, 1)]


def load_arena():
    L = C.CDLL(hostcheck.build("libsimt_x_rollout_arena.so"))
    L.sxa_rollout_arena.restype = C.c_longlong
    L.sxa_rollout_arena.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_uint, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
                                    + [C.c_void_p] * 13 + [C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_int])
    L.sxa_buffer_oob.restype = C.c_ulonglong
    return L


_VS = {}


def vs_reference(case, a, o):
    """The single-opponent run of agent = member a against opponent = member o: computed once per case and pair, shared, never modified."""
    if (case, a, o) not in _VS:
        L = load_vs()
        pool, argmax = CASES[case]
        r = fresh(pool)
        wa, wo = member_weights(a), member_weights(o)       # (kept alive: pointers() holds addresses only)
        wp, wop = pointers(wa), pointers(wo)
        assert L.sxv_rollout(*head_args(r, pool), wp, wop, *tail_args(r, argmax)) > 0
        _VS[case, a, o] = r
    return _VS[case, a, o]


def run_arena(case, pool_weights, pairs):
    L = load_arena()
    pool, argmax = CASES[case]
    r = fresh(pool)
    stacked = {k: np.ascontiguousarray(np.stack([x[k] for x in pool_weights])) for k in KEYS}
    pp = pointers(stacked)
    am = np.asarray([p[0] for p in pairs], np.uint8)
    om = np.asarray([p[1] for p in pairs], np.uint8)
    assert am.size == (N + GROUP - 1) // GROUP
    oob0 = L.sxa_buffer_oob()
    assert L.sxa_rollout_arena(*head_args(r, pool), pp, len(pool_weights), ptr(am), ptr(om), *tail_args(r, argmax)) > 0
    assert L.sxa_buffer_oob() == oob0
    return r


def assert_groups_equal(r, case, pairs):
    for grp, (a, o) in enumerate(pairs):
        idx = np.arange(grp * GROUP, min(N, (grp + 1) * GROUP))
        ref = vs_reference(case, a, o)
        for k in r:
            assert games(r, k, idx) == games(ref, k, idx), (case, grp, a, o, k)


@pytest.mark.parametrize("case", list(CASES))
def test_every_group_equals_the_single_opponent_kernel_with_its_pair(case):
    r = run_arena(case, [member_weights(0), member_weights(1)], PAIRS)
    assert_groups_equal(r, case, PAIRS)
    x, y = vs_reference(case, 1, 0), vs_reference(case, 0, 1)
    assert x["action"].tobytes() != y["action"].tobytes()               # two pairs do play differently: the comparison can fail
    assert (r["opp_replies"] > 0).any()


def test_a_pool_of_one_is_the_single_opponent_kernel():
    case = "lid_distribution"
    r = run_arena(case, [member_weights(1)], [(0, 0), (0, 0)])
    ref = vs_reference(case, 1, 1)
    for k in r:
        assert r[k].tobytes() == ref[k].tobytes(), k


def test_an_unnamed_member_is_never_read_and_a_member_past_the_pool_is_the_last_one():
    case = "lid_distribution"
    poison = {k: np.full_like(v, np.nan) for k, v in member_weights(0).items()}
    r = run_arena(case, [member_weights(0), member_weights(1), poison], PAIRS)
    assert_groups_equal(r, case, PAIRS)
    r = run_arena(case, [member_weights(0), member_weights(1)], [(7, 0), (0, 9)])     # 7, 9 >= K = 2 read as member 1
    assert_groups_equal(r, case, PAIRS)
