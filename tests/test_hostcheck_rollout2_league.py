"""The LEAGUE inside the two-player window kernel on CPU: azul_policy_rollout2_kernel<LID, 2> with RolloutArgs::opp_member set
(csrc/azul_rollout2.hpp, compiled UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_rollout2_league.cpp)
against the SAME kernel with a single opponent (simt_rollout2.cpp: sr2_rollout_vs) run once per pool member with that member's weights.
35 games -- two full 16-game groups and a ragged group of three -- five steps, general weights, groups assigned [1, 0, 1] of a pool of two:
every output buffer, record, MT19937 state, counter and trace of the games of a member's groups must equal that member's single-opponent
run BYTE FOR BYTE (a game's trajectory is keyed by its global id, not by what its neighbours play against).  Also: a pool of one equals the
single-opponent kernel on all games; an unused member's weights are never read (poisoned with NaN, nothing changes); a member value past the
pool is read as the last member and no weight fragment is requested outside its matrix."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as oz
from tests.hostcheck import hostcheck
from tests.test_hostcheck_env2 import RULES, ptr, start_batch
from tests.test_hostcheck_rollout2 import load_vs, to_agent_decision, weights

N, T, SLOTS, SEED0, WARM = 35, 5, 8, 300, 40
GROUP = 16
KEYS = ("w1t", "b1", "w2c", "b2c", "w2a_t", "b2a")
ARGMAX = 0xFFFFFFFFFFFFFFFF
CASES = {"lid_distribution": ("lid_randomfirst", False), "lid_max": ("lid_randomfirst", True),
         "random_distribution": ("random_first1", False), "random_max": ("random_first1", True)}


def load_league():
    L = C.CDLL(hostcheck.build("libsimt_rollout2_league.so"))
    L.sr2l_rollout_league.restype = C.c_longlong
    L.sr2l_rollout_league.argtypes = ([C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
                                      + [C.c_void_p] * 11 + [C.c_float, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong] + [C.c_void_p] * 3 + [C.c_int])
    L.sr2l_buffer_oob.restype = C.c_ulonglong
    return L


_START, _VS = {}, {}


def start(ruleset):
    """The batch every run of a rule set starts from: games part-way through their episodes, at an agent decision."""
    if ruleset not in _START:
        first, pool = RULES[ruleset]
        state, mt, pos = start_batch(N, SEED0, first, pool, WARM)
        rng = np.random.default_rng(SEED0)
        for g in range(N):
            state[g], mt[g], pos[g] = to_agent_decision(state[g].view(oz.RECORD_DTYPE)[0], mt[g], pos[g], first, pool, rng)
        _START[ruleset] = (state, mt, pos)
    return tuple(x.copy() for x in _START[ruleset])


def fresh(ruleset):
    state, mt, pos = start(ruleset)
    o = {"state": state, "mt": mt, "pos": pos, "ep": np.zeros(N, np.uint64), "stuck": np.zeros(N, np.uint32), "ss": np.zeros((N, 10)),
         "obs": np.full((T + 1, N, 136), -99, np.float32), "mask": np.full((T + 1, N, 180), 0xEE, np.uint8),
         "player": np.full((T + 1, N), 9, np.uint8), "action": np.full((T, N), -7, np.int32), "reward": np.full((T, N), -7777, np.int32),
         "done": np.full((T, N), 9, np.uint8), "value": np.full((T, N), np.nan, np.float32), "logp": np.full((T, N), np.nan, np.float32),
         "entropy": np.full((T, N), np.nan, np.float32), "status": np.full(N, 99, np.uint8), "returns": np.full((T, N), np.nan, np.float32),
         "opp_action": np.full((T, SLOTS, N), -9, np.int32), "opp_logp": np.full((T, SLOTS, N), np.nan, np.float32),
         "opp_replies": np.full((T, N), 200, np.uint8)}
    return o


GAME_AXIS = {"state": 0, "mt": 0, "pos": 0, "ep": 0, "stuck": 0, "ss": 0, "status": 0, "opp_action": 2, "opp_logp": 2}    # (the others: axis 1)


def games(o, k, idx):
    return np.ascontiguousarray(np.take(o[k], idx, axis=GAME_AXIS.get(k, 1))).tobytes()


def pointers(w):
    return (C.c_void_p * 6)(*[w[k].ctypes.data for k in KEYS])


def run_vs(ruleset, argmax, wo):
    L = load_vs()
    first, pool = RULES[ruleset]
    o, wa = fresh(ruleset), weights(SEED0)
    pa, po = pointers(wa), pointers(wo)
    oob0 = L.sr2_buffer_oob()
    ops = L.sr2_rollout_vs(N, ptr(o["state"]), ptr(o["mt"]), ptr(o["pos"]), ptr(o["ep"]), ptr(o["stuck"]), ptr(o["ss"]), first, pool, 1000,
                           C.cast(pa, C.c_void_p), C.cast(po, C.c_void_p), T, ptr(o["obs"]), ptr(o["mask"]), ptr(o["player"]), ptr(o["action"]),
                           ptr(o["reward"]), ptr(o["done"]), ptr(o["value"]), ptr(o["logp"]), ptr(o["entropy"]), ptr(o["status"]), ptr(o["returns"]),
                           0.9, 4242, ARGMAX if argmax else 777, 17, ptr(o["opp_action"]), ptr(o["opp_logp"]), ptr(o["opp_replies"]), SLOTS)
    assert ops > 0 and L.sr2_buffer_oob() == oob0
    return o


def member_weights(m):
    return weights(SEED0 + 1 + m)


def vs_reference(case, m):
    """The single-opponent run against member m: computed once per case and member, shared, never modified."""
    if (case, m) not in _VS:
        ruleset, argmax = CASES[case]
        _VS[case, m] = run_vs(ruleset, argmax, member_weights(m))
    return _VS[case, m]


def run_league(case, pool_weights, members):
    L = load_league()
    ruleset, argmax = CASES[case]
    first, pool = RULES[ruleset]
    o, wa = fresh(ruleset), weights(SEED0)
    stacked = {k: np.ascontiguousarray(np.stack([w[k] for w in pool_weights])) for k in KEYS}
    pa, pp = pointers(wa), pointers(stacked)
    mem = np.asarray(members, np.uint8)
    assert mem.size == (N + GROUP - 1) // GROUP
    oob0 = L.sr2l_buffer_oob()
    ops = L.sr2l_rollout_league(N, ptr(o["state"]), ptr(o["mt"]), ptr(o["pos"]), ptr(o["ep"]), ptr(o["stuck"]), ptr(o["ss"]), first, pool, 1000,
                                C.cast(pa, C.c_void_p), C.cast(pp, C.c_void_p), len(pool_weights), ptr(mem), T, ptr(o["obs"]), ptr(o["mask"]),
                                ptr(o["player"]), ptr(o["action"]), ptr(o["reward"]), ptr(o["done"]), ptr(o["value"]), ptr(o["logp"]),
                                ptr(o["entropy"]), ptr(o["status"]), ptr(o["returns"]), 0.9, 4242, ARGMAX if argmax else 777, 17,
                                ptr(o["opp_action"]), ptr(o["opp_logp"]), ptr(o["opp_replies"]), SLOTS)
    assert ops > 0
    assert L.sr2l_buffer_oob() == oob0                      # no weight fragment was requested outside its member's matrix
    return o


def assert_groups_equal(o, case, members):
    for grp, m in enumerate(members):
        idx = np.arange(grp * GROUP, min(N, (grp + 1) * GROUP))
        ref = vs_reference(case, m)
        for k in o:
            assert games(o, k, idx) == games(ref, k, idx), (case, grp, m, k)


@pytest.mark.parametrize("case", list(CASES))
def test_every_group_equals_the_single_opponent_kernel_against_its_member(case):
    o = run_league(case, [member_weights(0), member_weights(1)], [1, 0, 1])
    assert_groups_equal(o, case, [1, 0, 1])
    a, b = vs_reference(case, 0), vs_reference(case, 1)
    assert a["opp_action"].tobytes() != b["opp_action"].tobytes()       # the members do answer differently: the comparison can fail
    assert (o["opp_replies"] > 0).any() and (o["opp_replies"] <= SLOTS).all()


def test_a_pool_of_one_is_the_single_opponent_kernel():
    case = "lid_distribution"
    o = run_league(case, [member_weights(0)], [0, 0, 0])
    ref = vs_reference(case, 0)
    for k in o:
        assert o[k].tobytes() == ref[k].tobytes(), k


def test_an_unused_member_is_never_read_and_a_member_past_the_pool_is_the_last_one():
    case = "lid_distribution"
    poison = {k: np.full_like(v, np.nan) for k, v in member_weights(0).items()}
    o = run_league(case, [member_weights(0), member_weights(1), poison], [1, 0, 1])
    assert_groups_equal(o, case, [1, 0, 1])
    o = run_league(case, [member_weights(0), member_weights(1)], [7, 0, 7])          # 7 >= K = 2 reads as member 1 (run_league checks the loads)
    assert_groups_equal(o, case, [1, 0, 1])
