"""GPU: the edges of the pool behind the league's and the arena's window kernels, on the two-player batch and on the wide shape with the
largest strides (four players on nine displays: 260 inputs, 300 actions) -- 35 games (groups of 16, 16 and 3), two windows of 8 steps, every
comparison of bits:

  * a pool of ONE equals the plain single-opponent entry on all games;
  * a pool of 255 (the limit: a member is one byte) in which only members 0, 127 and 254 are nets and every other slot is NaN: each group
    equals the single-opponent run of its nets, and every float the run writes is finite;
  * members that no seat names are never read: a pool of four, two of them NaN, equals the pool of the other two;
  * a seat byte at or past pool_size is read as pool_size - 1 (league_member_of_block, arena_agent_of_block; the host validators refuse
    such bytes, so they are written on the device): the entry is launched with pool_size = 2 on stacks of 255 allocated slots, slots 2..254
    NaN, and bytes 2 and 254 must play member 1 -- a clamp that did not work would read allocated NaN weights and fail BY VALUE; the
    highest byte stays below the number of allocated slots, so nothing is read outside an allocation whether the clamp works or not.
    The tally afterwards books those groups to member 1, as a host recount from the done flags says.

The pool, its size and the seat bytes are swapped on the rollout's own objects from inside the tests: production code has no switch for it."""
import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd.records import STAT_KEYS
from tests.test_gpu_arena import _arena
from tests.test_gpu_arena_shapes import compare_arena_with_singles
from tests.test_gpu_league import GROUP, _eq_games, _eq_state, _play, _rollout
from tests.test_gpu_league_shapes import CASE_IDS, CASES, N, T, W, _all_finite, _differ, _entries, _league, _nets, compare_league_with_singles

pytestmark = pytest.mark.gpu

BATCHES = [CASES[0], CASES[-1]]
BATCH_IDS = [CASE_IDS[0], CASE_IDS[-1]]
batches = pytest.mark.parametrize("players,rules", BATCHES, ids=BATCH_IDS)
SLOTS = 255
ALL = np.arange(N)
LONG = 14                      # further windows before the tally: 128 agent steps in all, so that episodes end in every 16-game group


def _nan_net(players, rules):
    net = _nets(players, rules, 0, 1)[0]
    with torch.no_grad():
        for prm in net.parameters():
            prm.fill_(float("nan"))
    return net


def _same_run(a, b, what):
    """Two runs (_play's windows and state) agree bit for bit on every game."""
    for w in range(W):
        _eq_games(a[0][w], b[0][w], ALL, "%s window %d" % (what, w))
    _eq_state(a[1], b[1], ALL, what)


# ---- a pool of one ------------------------------------------------------------------------------------------------------------------------
@batches
def test_a_league_of_one_equals_the_single_opponent_entry(players, rules):
    policy, net = _nets(players, rules, 81, 2)
    league_entry, vs_entry = _entries(players, rules)
    ro = _rollout(policy, [net], N, T, players, rules)
    assert ro.window_entry == league_entry and ro.pool_size == 1 and ro.assignment().tolist() == [[0, 0, 0]]
    single = _rollout(policy, net, N, T, players, rules)
    assert single.window_entry == vs_entry
    lg = _play(ro, W)
    _same_run(lg, _play(single, W), "a league of one")
    assert int(lg[0][0]["opp_replies"].sum()) > N * T // 2


@batches
def test_an_arena_of_one_equals_the_net_against_itself(players, rules):
    compare_arena_with_singles(_nets(players, rules, 82, 1), [(0, 0)] * 3, players, rules)


# ---- 255 members ----------------------------------------------------------------------------------------------------------------------------
def _pool_of_255(players, rules, seed):
    real = _nets(players, rules, seed, 3)
    pool = [_nan_net(players, rules)] * SLOTS                            # ONE module for every slot that is no net
    pool[0], pool[127], pool[254] = real
    return pool


@batches
def test_a_league_of_255_reads_the_seated_members_at_both_ends_of_the_pool(players, rules):
    policy = _nets(players, rules, 83, 1)[0]
    lg, singles = compare_league_with_singles(policy, _pool_of_255(players, rules, 84), [254, 0, 127], players, rules)
    assert _all_finite(lg)
    assert _differ(singles[254], singles[0]) and _differ(singles[0], singles[127])


@batches
def test_an_arena_of_255_reads_the_seated_members_at_both_ends_of_the_pool(players, rules):
    got, singles = compare_arena_with_singles(_pool_of_255(players, rules, 85), [(254, 0), (0, 127), (127, 254)], players, rules)
    assert _all_finite(got)
    assert _differ(singles[254, 0], singles[0, 127]) and _differ(singles[0, 127], singles[127, 254])


# ---- members without a seat are never read --------------------------------------------------------------------------------------------------
@batches
def test_a_league_never_reads_a_member_without_a_seat(players, rules):
    policy, a, b = _nets(players, rules, 86, 3)
    nan = _nan_net(players, rules)
    ro = _league(policy, [nan, a, nan, b], [3, 1, 3], players, rules)
    assert ro.window_entry == _entries(players, rules)[0] and ro.pool_size == 4
    got = _play(ro, W)
    _same_run(got, _play(_league(policy, [a, b], [1, 0, 1], players, rules), W), "members 1 and 3 of four")
    assert _all_finite(got[0]) and int(got[0][0]["opp_replies"].sum()) > N * T // 2


@batches
def test_an_arena_never_reads_a_member_without_a_seat(players, rules):
    a, b = _nets(players, rules, 87, 2)
    nan = _nan_net(players, rules)
    ar = _arena([nan, a, nan, b], N, T, [[(3, 1), (1, 3), (3, 3)]], players, rules)
    assert ar.arena_entry == _entries(players, rules, "arena")[0] and ar.pool.size == 4
    got = _play(ar, W)
    _same_run(got, _play(_arena([a, b], N, T, [[(1, 0), (0, 1), (1, 1)]], players, rules), W), "members 1 and 3 of four")
    assert _all_finite(got[0]) and int(got[0][0]["opp_replies"].sum()) > N * T // 2


# ---- seat bytes past the pool ---------------------------------------------------------------------------------------------------------------
def _overallocate(ro):
    """Hand the window entry stacks of SLOTS member slots while the pool's size stays what it is: the members in front, NaN behind."""
    pool, big = ro.pool, {}
    for k, v in pool.stacks.items():
        big[k] = torch.full((SLOTS,) + tuple(v.shape[1:]), float("nan"), dtype=v.dtype, device=v.device)
        big[k][:pool.size].copy_(v)
    pool.stacks = big
    assert pool.size == 2 and pool.weights().w1t == big["w1t"].data_ptr()


def _write_seat(ro, role, group, byte):
    assert 0 <= byte < SLOTS                                             # the byte names an ALLOCATED slot: nothing can fault
    ro.pool.seats[0, role, group] = byte                                 # on the device, behind the host validators


def _done_per_group(windows):
    """Episodes that ended (done == 1) in the 16-game groups, over `windows`."""
    done = sum((tr["done"] == 1).sum(dim=0) for tr in windows).numpy()
    return [int(done[g * GROUP:(g + 1) * GROUP].sum()) for g in range((N + GROUP - 1) // GROUP)]


def _sums_in_tally_order(ro, groups):
    """The statistic sums of `groups` (ascending) from the per-game counters, added game by game from zero as ONE tally adds them."""
    ss = ro.envs[0].counters()["stat_sums"]
    acc = np.zeros(10)
    for g in groups:
        for i in range(g * GROUP, min(N, (g + 1) * GROUP)):
            acc = acc + (ss[i] - 0.0)
    return acc


@batches
def test_league_seat_bytes_past_the_pool_play_the_last_member(players, rules):
    policy, a, b = _nets(players, rules, 88, 3)
    want = _play(_league(policy, [a, b], [1, 0, 1], players, rules), W)
    ro = _league(policy, [a, b], [1, 0, 1], players, rules)             # the same seats: the same openings at construction
    _overallocate(ro)
    _write_seat(ro, 0, 0, 2)
    _write_seat(ro, 0, 2, 254)
    got = _play(ro, W)
    assert ro.pool.seats[0, 0].tolist() == [2, 0, 254] and ro.pool_size == 2
    _same_run(got, want, "bytes 2 and 254 in a pool of two")
    assert _all_finite(got[0])
    # member 0 in those groups would have played otherwise: the trace's log-probabilities are another net's
    zero = _play(_league(policy, [a, b], [0, 0, 0], players, rules), W)
    for g in (0, 2):
        idx = slice(g * GROUP, min(N, (g + 1) * GROUP))
        assert not torch.equal(zero[0][0]["opp_logp"][:, :, idx], want[0][0]["opp_logp"][:, :, idx]), g
    # the tally reads the same bytes: groups 0 and 2 are booked to member 1, group 1 to member 0
    more, _ = _play(ro, LONG)
    done = _done_per_group(got[0] + more)
    res = ro.league_results()
    print("episodes per group:", done)
    assert [r["episodes"] for r in res] == [done[1], done[0] + done[2]]
    assert done[0] > 0 and done[1] > 0                                   # both members finished episodes (group 2 has three games only)
    for m, groups in ((0, [1]), (1, [0, 2])):
        ss = _sums_in_tally_order(ro, groups)
        for i, k in enumerate(STAT_KEYS):
            assert res[m][k] == ss[i] / res[m]["episodes"], (m, k)


@batches
def test_arena_seat_bytes_past_the_pool_play_the_last_member(players, rules):
    a, b = _nets(players, rules, 89, 2)
    pairs = [[(1, 0), (0, 1), (1, 1)]]
    want = _play(_arena([a, b], N, T, pairs, players, rules), W)
    ar = _arena([a, b], N, T, pairs, players, rules)
    _overallocate(ar)
    _write_seat(ar, 0, 0, 254)                                           # group 0's agent
    _write_seat(ar, 1, 1, 2)                                             # group 1's opponent
    got = _play(ar, W)
    assert ar.pool.seats[0].tolist() == [[254, 0, 1], [0, 2, 1]] and ar.pool.size == 2
    _same_run(got, want, "bytes 254 and 2 in a pool of two")
    assert _all_finite(got[0])
    # member 0 in those seats would have played otherwise: group 0's values are another critic's, group 1 meets another opponent
    zero = _play(_arena([a, b], N, T, [[(0, 0), (0, 0), (1, 1)]], players, rules), W)
    assert not torch.equal(zero[0][0]["value"][:, :GROUP], want[0][0]["value"][:, :GROUP])
    assert any(not torch.equal(zero[0][w][k][:, GROUP:2 * GROUP], want[0][w][k][:, GROUP:2 * GROUP]) for w in range(W) for k in ("obs", "action"))
    # the tally reads the same bytes: group 0 is cell [1][0], group 1 cell [0][1], group 2 cell [1][1]
    more, _ = _play(ar, LONG)
    done = _done_per_group(got[0] + more)
    res = ar.results()
    print("episodes per group:", done)
    assert res["episodes"].tolist() == [[0, done[1]], [done[0], done[2]]]
    assert done[0] > 0 and done[1] > 0                                   # the two clamped cells hold episodes (group 2 has three games only)
    for (x, o), g in (((1, 0), 0), ((0, 1), 1), ((1, 1), 2)):
        if not done[g]:
            continue
        ss = _sums_in_tally_order(ar, [g])
        for i, k in enumerate(STAT_KEYS):
            assert res["mean"][k][x, o] == ss[i] / done[g], (x, o, k)
