"""The LEAGUE inside the wide window kernel on CPU: azul_x_policy_rollout_vs_kernel<3, 5, true> (csrc/azul_rollout2.hpp, compiled UNMODIFIED by
g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_x_rollout_league.cpp) against the single-opponent kernel
(simt_x_rollout_vs.cpp: sxv_rollout) run once per pool member with that member's weights.  Three players on five displays, 19 games -- a full
16-game group and a ragged group of three -- five steps, general weights, groups assigned [1, 0] of a pool of two: every output buffer, record,
MT19937 state, counter and trace of the games of a member's group must equal that member's single-opponent run BYTE FOR BYTE.  Also: a pool
of one equals the single-opponent kernel on all games; an unused member's weights are never read (NaN poison); a member value past the pool is
read as the last member."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as oz
from tests.hostcheck import hostcheck
from tests.mp_net_model import MPNetRunner
from tests.test_hostcheck_x_rollout import ptr, weights
from tests.test_hostcheck_x_rollout_vs import load as load_vs

P, D, N, T, SLOTS, SEED, COUNTER, ID_BASE, GROUP = 3, 5, 19, 5, 64, 0x5EED + 3, 40, 1000, 16
NA, OBS = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
KEYS = ("w1t", "b1", "w2c", "b2c", "w2a_t", "b2a")
ARGMAX = 0xFFFFFFFFFFFFFFFF
CASES = {"lid_distribution": (oz.POOL_LID, False), "random_max": (oz.POOL_RANDOM, True)}
OUT = ("obs", "mask", "player", "action", "reward", "done", "value", "logp", "entropy", "status", "opp_action", "opp_logp", "opp_replies")


def load_league():
    L = C.CDLL(hostcheck.build("libsimt_x_rollout_league.so"))
    L.sxl_rollout_league.restype = C.c_longlong
    L.sxl_rollout_league.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
                                     + [C.c_void_p] * 13 + [C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_int])
    L.sxl_buffer_oob.restype = C.c_ulonglong
    return L


_START, _VS = {}, {}


def start(pool):
    """Games part-way through their episodes (GameRunner() + reset() with a random stand-in opponent, then some agent steps)."""
    if pool not in _START:
        rnd = random.Random(100 * P + pool)

        def rand_answer(obs, mask, player):
            legal = np.flatnonzero(mask)
            return int(rnd.choice(list(legal))) if len(legal) else -1

        models = [MPNetRunner(P, oz.FIRST_RANDOM, pool, 0, seed=4000 + 17 * P + g) for g in range(N)]
        for m in models:
            m.runner_init()
            m.reset_with(rand_answer)
            for _ in range(rnd.randrange(0, 45)):
                m.step_with(rand_answer(*m.opp_view()), rand_answer)
        _START[pool] = {"state": np.stack([m.record() for m in models]), "mt": np.stack([m.rng_state()[0] for m in models]).astype(np.uint32),
                        "pos": np.array([m.rng_state()[1] for m in models], np.uint32), "ep": np.array([m.episodes for m in models], np.uint64),
                        "stuck": np.array([m.stuck for m in models], np.uint32), "ss": np.stack([m.stat_sum for m in models]).astype(np.float64)}
    return {k: v.copy() for k, v in _START[pool].items()}


def fresh(pool):
    o = start(pool)
    for k, shape, dt, fill in (("obs", (T + 1, N, OBS), np.float32, -99), ("mask", (T + 1, N, NA), np.uint8, 0xEE), ("player", (T + 1, N), np.uint8, 9),
                               ("action", (T, N), np.int32, -7), ("reward", (T, N), np.int32, -7777), ("done", (T, N), np.uint8, 9),
                               ("value", (T, N), np.float32, np.nan), ("logp", (T, N), np.float32, np.nan), ("entropy", (T, N), np.float32, np.nan),
                               ("status", (N,), np.uint8, 99), ("opp_action", (T, SLOTS, N), np.int32, -5), ("opp_logp", (T, SLOTS, N), np.float32, 55.0),
                               ("opp_replies", (T, N), np.uint8, 201)):
        o[k] = np.full(shape, fill, dt)
    return o


GAME_AXIS = {"state": 0, "mt": 0, "pos": 0, "ep": 0, "stuck": 0, "ss": 0, "status": 0, "opp_action": 2, "opp_logp": 2}    # (the others: axis 1)


def games(o, k, idx):
    return np.ascontiguousarray(np.take(o[k], idx, axis=GAME_AXIS.get(k, 1))).tobytes()


def pointers(w):
    return (C.c_void_p * 6)(*[w[k].ctypes.data for k in KEYS])


def member_weights(m):
    return weights(OBS, NA, SEED + 1 + m)


def head_args(o, pool):
    return (N, P, D, ptr(o["state"]), ptr(o["mt"]), ptr(o["pos"]), ptr(o["ep"]), ptr(o["stuck"]), ptr(o["ss"]), oz.FIRST_RANDOM,
            1 if pool == oz.POOL_LID else 0, 0, 0, ID_BASE)


def tail_args(o, argmax):
    return (T, *[ptr(o[k]) for k in OUT], SLOTS, SEED, ARGMAX if argmax else 0x0770 + P, COUNTER, 512)


def vs_reference(case, m):
    """The single-opponent run against member m: computed once per case and member, shared, never modified."""
    if (case, m) not in _VS:
        L = load_vs()
        pool, argmax = CASES[case]
        o, w, wo = fresh(pool), weights(OBS, NA, SEED), member_weights(m)
        wp, wop = pointers(w), pointers(wo)
        assert L.sxv_rollout(*head_args(o, pool), wp, wop, *tail_args(o, argmax)) > 0
        _VS[case, m] = o
    return _VS[case, m]


def run_league(case, pool_weights, members):
    L = load_league()
    pool, argmax = CASES[case]
    o, w = fresh(pool), weights(OBS, NA, SEED)
    stacked = {k: np.ascontiguousarray(np.stack([x[k] for x in pool_weights])) for k in KEYS}
    wp, pp = pointers(w), pointers(stacked)
    mem = np.asarray(members, np.uint8)
    assert mem.size == (N + GROUP - 1) // GROUP
    oob0 = L.sxl_buffer_oob()
    assert L.sxl_rollout_league(*head_args(o, pool), wp, pp, len(pool_weights), ptr(mem), *tail_args(o, argmax)) > 0
    assert L.sxl_buffer_oob() == oob0
    return o


def assert_groups_equal(o, case, members):
    for grp, m in enumerate(members):
        idx = np.arange(grp * GROUP, min(N, (grp + 1) * GROUP))
        ref = vs_reference(case, m)
        for k in o:
            assert games(o, k, idx) == games(ref, k, idx), (case, grp, m, k)


@pytest.mark.parametrize("case", list(CASES))
def test_every_group_equals_the_single_opponent_kernel_against_its_member(case):
    o = run_league(case, [member_weights(0), member_weights(1)], [1, 0])
    assert_groups_equal(o, case, [1, 0])
    a, b = vs_reference(case, 0), vs_reference(case, 1)
    assert a["opp_action"].tobytes() != b["opp_action"].tobytes()       # the members do answer differently: the comparison can fail
    assert (o["opp_replies"] > 0).any()


def test_a_pool_of_one_is_the_single_opponent_kernel():
    case = "lid_distribution"
    o = run_league(case, [member_weights(1)], [0, 0])
    ref = vs_reference(case, 1)
    for k in o:
        assert o[k].tobytes() == ref[k].tobytes(), k


def test_an_unused_member_is_never_read_and_a_member_past_the_pool_is_the_last_one():
    case = "lid_distribution"
    poison = {k: np.full_like(v, np.nan) for k, v in member_weights(0).items()}
    o = run_league(case, [member_weights(0), member_weights(1), poison], [1, 0])
    assert_groups_equal(o, case, [1, 0])
    o = run_league(case, [member_weights(0), member_weights(1)], [7, 0])              # 7 >= K = 2 reads as member 1
    assert_groups_equal(o, case, [1, 0])
