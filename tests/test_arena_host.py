"""The arena without a device: the schedule (round_robin_pairs), the book-keeping kernel azul_arena_tally_kernel (csrc/azul_policy.hpp,
compiled UNMODIFIED by g++ under the lockstep emulation: tests/hostcheck/simt_arena_tally.cpp) against a NumPy recount in the stated order,
the rating (bradley_terry), Arena's refusals before anything is allocated, and the three C entries (declared, exported, bound, refusing
their arguments on the host)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.hostcheck import hostcheck
from tests.pool_tally_ref import arena_tally_ref as tally_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("azul_batch_policy_rollout_arena", "azul_batch_mp_policy_rollout_arena", "azul_arena_tally")
GROUP = 16


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,groups,mirror", [(2, 1, False), (3, 4, False), (4, 5, False), (4, 3, True), (5, 256, False), (16, 256, False)])
def test_round_robin_plays_every_ordered_pair_evenly_over_one_cycle(K, groups, mirror):
    from azul_deep_reinforcement_learning_amd.arena import round_robin_pairs, rounds_per_cycle
    want = set((i, j) for i in range(K) for j in range(K) if mirror or i != j)
    counts = {}
    for r in range(rounds_per_cycle(K, groups, mirror)):
        a = round_robin_pairs(K, groups, r, mirror)
        assert a.shape == (groups, 2) and a.dtype.kind == "i"
        for i, j in a.tolist():
            counts[i, j] = counts.get((i, j), 0) + 1
    assert set(counts) == want                                           # every ordered pair, and nothing else (no (i, i) without mirror)
    assert max(counts.values()) - min(counts.values()) <= 1


def test_round_robin_order_mirror_a_pool_of_one_and_a_ragged_last_group():
    from azul_deep_reinforcement_learning_amd.arena import round_robin_pairs
    assert round_robin_pairs(3, 6, 0).tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1]]          # lexicographic
    assert round_robin_pairs(3, 4, 1).tolist() == [[2, 0], [2, 1], [0, 1], [0, 2]]                          # pair (r * groups + g) mod P
    assert round_robin_pairs(2, 5, 0, mirror=True).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [0, 0]]
    assert round_robin_pairs(1, 3, 7).tolist() == [[0, 0]] * 3 and round_robin_pairs(1, 2, 0, mirror=True).tolist() == [[0, 0]] * 2
    n = 40                                                               # groups of 16, 16 and 8: the ragged group is a group like any other
    assert round_robin_pairs(2, (n + GROUP - 1) // GROUP, 0).tolist() == [[0, 1], [1, 0], [0, 1]]
    with pytest.raises(ValueError):
        round_robin_pairs(0, 4, 0)


# ---- the tally kernel -----------------------------------------------------------------------------------------------------------------
def load_tally():
    L = C.CDLL(hostcheck.build("libsimt_arena_tally.so"))
    L.sat_tally.restype = C.c_longlong
    L.sat_tally.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    return L


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_arena_tally_kernel_matches_the_numpy_recount_bit_for_bit():
    L = load_tally()
    n, K = 35, 3
    rs = np.random.RandomState(35)
    agent, opp = np.array([2, 0, 2], np.uint8), np.array([1, 2, 9], np.uint8)      # (2, 1), (0, 2), (2, 9 -> 2); every other pair is absent
    ep = rs.randint(0, 50, n).astype(np.uint64)
    ss = rs.randn(n, 10) * 100.0                                         # general doubles: the ORDER of the additions shows in the bits
    mark_ep, mark_ss = np.zeros(n, np.uint64), np.zeros((n, 10))
    results = rs.randn(K, K, 11)                                         # what earlier calls left
    sentinel = results.copy()
    want = tally_ref(ep, ss, mark_ep, mark_ss, agent, opp, K, results)
    assert L.sat_tally(ptr(ep), ptr(ss), ptr(mark_ep), ptr(mark_ss), ptr(agent), ptr(opp), n, K, ptr(results)) > 0
    assert results.tobytes() == want.tobytes()
    assert np.array_equal(mark_ep, ep) and mark_ss.tobytes() == ss.tobytes()       # the marks moved up
    used = {(2, 1), (0, 2), (2, 2)}
    for a in range(K):
        for o in range(K):
            if (a, o) in used:
                assert results[a, o].tobytes() != sentinel[a, o].tobytes()
            else:
                assert results[a, o].tobytes() == sentinel[a, o].tobytes()         # a cell whose pair has no group is not written
    before = results.copy()                                              # a second call with counters that have not moved adds nothing
    assert L.sat_tally(ptr(ep), ptr(ss), ptr(mark_ep), ptr(mark_ss), ptr(agent), ptr(opp), n, K, ptr(results)) > 0
    assert results.tobytes() == before.tobytes()
    # two groups of one pair: the cell takes both in ascending game order; only the change since the marks is booked, to the NEW pairs
    ep2 = ep + rs.randint(0, 4, n).astype(np.uint64)
    ss2 = ss + rs.randn(n, 10)
    agent2, opp2 = np.array([1, 0, 1], np.uint8), np.array([0, 0, 0], np.uint8)
    want = tally_ref(ep2, ss2, mark_ep, mark_ss, agent2, opp2, K, results)
    assert L.sat_tally(ptr(ep2), ptr(ss2), ptr(mark_ep), ptr(mark_ss), ptr(agent2), ptr(opp2), n, K, ptr(results)) > 0
    assert results.tobytes() == want.tobytes()
    assert np.array_equal(mark_ep, ep2) and mark_ss.tobytes() == ss2.tobytes()


# ---- the rating -----------------------------------------------------------------------------------------------------------------------
def test_bradley_terry_recovers_known_strengths_from_exact_expected_counts():
    from azul_deep_reinforcement_learning_amd.arena import bradley_terry
    p = np.array([4.0, 2.0, 1.0, 0.5, 0.25])
    p = p / np.exp(np.log(p).mean())                                     # geometric mean 1: ratings of mean 0
    K, n = len(p), 1000.0
    episodes = np.full((K, K), n) - np.diag(np.full(K, n))
    wins = np.array([[n * p[i] / (p[i] + p[j]) if i != j else 0.0 for j in range(K)] for i in range(K)])     # agent seat i against j
    out = bradley_terry(episodes, wins, prior=0)
    # the maximum-likelihood estimate of exact expectations is the truth, and the iteration stops at a relative change of 1e-13
    assert np.abs(out["rating"] - 400.0 * np.log10(p)).max() < 1e-6
    assert abs(out["rating"].mean()) < 1e-9 and 0 < out["iterations"] < 10000
    assert np.allclose(out["strength"], p, rtol=1e-8, atol=0)
    # only one direction played: the opponent seat's wins are episodes - wins
    one_way = np.triu(episodes, 1)
    out = bradley_terry(one_way, np.triu(wins, 1), prior=0)
    assert np.abs(out["rating"] - 400.0 * np.log10(p)).max() < 1e-6


def test_bradley_terry_prior_keeps_an_unbeaten_member_finite():
    from azul_deep_reinforcement_learning_amd.arena import bradley_terry
    episodes = np.array([[0, 10, 10], [10, 0, 10], [10, 10, 0]], float)
    wins = np.array([[np.nan, 10, 10], [0, np.nan, 6], [0, 5, np.nan]])  # member 0 wins every game, in either seat
    out = bradley_terry(episodes, wins, prior=1.0)
    assert np.isfinite(out["rating"]).all() and out["rating"][0] == out["rating"].max()
    assert abs(out["rating"].mean()) < 1e-9
    free = bradley_terry(episodes, wins, prior=0, max_iter=200)
    assert free["rating"][0] > out["rating"][0]                          # without the prior its strength runs away
    with pytest.raises(ValueError):
        bradley_terry(np.zeros((2, 3)), np.zeros((2, 3)))


# ---- Arena's refusals and the C entries -----------------------------------------------------------------------------------------------
def _net(obs=136, act=180, hidden=180):
    from azul_deep_reinforcement_learning_amd import BatchedActorCritic
    return BatchedActorCritic(obs, act, hidden)


def test_arena_refusals_come_before_any_allocation():
    from azul_deep_reinforcement_learning_amd import Arena
    with pytest.raises(ValueError, match="pool of 1..255"):
        Arena([], n_games=16)
    with pytest.raises(ValueError, match="pool of 1..255"):
        Arena([_net()] * 256, n_games=16)
    with pytest.raises(ValueError, match="ONE shape"):
        Arena([_net(), _net(hidden=64)], n_games=16)
    with pytest.raises(ValueError, match="ONE shape"):
        Arena([_net(), _net(188)], n_games=16)
    with pytest.raises(ValueError, match=r"ActorCritic\(136, 180, hidden 180\)"):
        Arena([_net(hidden=64)] * 2, n_games=16)                          # the window kernels' hidden size
    with pytest.raises(ValueError, match=r"ActorCritic\(136, 180, hidden 180\)"):
        Arena([_net(188), _net(188)], n_games=16)                         # a wide shape on a two-player batch
    with pytest.raises(ValueError, match=r"ActorCritic\(188, 180, hidden 180\)"):
        Arena([_net(), _net()], n_games=16, players=3)                    # ... and the reverse
    with pytest.raises(ValueError, match="four layers"):
        Arena([_net(), "random"], n_games=16)
    with pytest.raises(ValueError, match="selection"):
        Arena([_net()], n_games=16, selection="Greedy")
    with pytest.raises(ValueError, match="shape"):
        Arena([_net(), _net()], n_games=16, pairs=[[0, 1]])
    with pytest.raises(ValueError, match="pool members 0..1"):
        Arena([_net(), _net()], n_games=16, pairs=[[[0, 2]]])


def test_arena_entries_are_declared_exported_bound_and_refuse_on_the_host():
    import azul_deep_reinforcement_learning_amd as pkg
    from azul_deep_reinforcement_learning_amd import _lib as L
    assert pkg.Arena is not None and pkg.round_robin_pairs is not None and pkg.bradley_terry is not None
    header = open(os.path.join(ROOT, "include", "azul_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in L.SIGNATURES and hasattr(L.lib, name)
    one, f32 = C.c_void_p(16), C.c_float
    wts, bufs = L.NetWeights(*[one] * 6), L.RolloutBuffers(*[one] * 14, 0)
    wr, br = C.byref(wts), C.byref(bufs)
    # without a batch nothing else is looked at, under the entry's own name
    assert L.lib.azul_batch_policy_rollout_arena(None, 4, wr, 2, one, one, 136, 180, 180, 1, 2, 0, None, br, f32(0.9), None) == L.ERR_INVALID
    assert L.lib.azul_last_error_string().decode().startswith("azul_batch_policy_rollout_arena")
    assert L.lib.azul_batch_mp_policy_rollout_arena(None, 4, wr, 2, one, one, 188, 180, 180, 1, 2, 0, None, 8, br, f32(0.9), None) == L.ERR_INVALID
    assert L.lib.azul_last_error_string().decode().startswith("azul_batch_mp_policy_rollout_arena")
    ok = (one, one, one, one, one, one, 35, 3, one, None)
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (8, None), (6, 0), (7, 0), (7, 256)):
        args = list(ok)
        args[i] = bad
        assert L.lib.azul_arena_tally(*args) == L.ERR_INVALID
        assert L.lib.azul_last_error_string().decode().startswith("azul_arena_tally")
