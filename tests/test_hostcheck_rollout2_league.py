"""The LEAGUE inside the two-player window kernel on CPU: azul_policy_rollout2_kernel<LID, 2> with RolloutArgs::opp_member set
(csrc/azul_rollout2.hpp, compiled UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_rollout2.cpp, sr2_window
with opp 2 and the member array) against the SAME kernel with a single opponent (the same entry without the array) run once per pool member with that member's weights.
35 games -- two full 16-game groups and a ragged group of three -- five steps, general weights, groups assigned [1, 0, 1] of a pool of two:
every output buffer, record, MT19937 state, counter and trace of the games of a member's groups must equal that member's single-opponent
run BYTE FOR BYTE (a game's trajectory is keyed by its global id, not by what its neighbours play against).  Also: a pool of one equals the
single-opponent kernel on all games; an unused member's weights are never read (poisoned with NaN, nothing changes); a member value past the
pool is read as the last member and no weight fragment is requested outside its matrix."""
import numpy as np
import pytest

from tests.hostcheck import window
from tests.hostcheck.window import CASES2 as CASES, GROUP, KEYS, N2 as N, SEED0, SLOTS2 as SLOTS, games
from tests.hostcheck.window import fresh2 as fresh, load2 as load, member_weights2 as member_weights, weights2 as weights, window_fields2

_VS = {}


def run_vs(ruleset, argmax, wo):
    L = load()
    o, wa = fresh(ruleset), weights(SEED0)
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **window_fields2(o, ruleset, 4242, argmax), opp=2, agent=wa, opponent=wo)
    assert ops > 0 and L.sr2_buffer_oob() == oob0
    return o


def vs_reference(case, m):
    """The single-opponent run against member m: computed once per case and member, shared, never modified."""
    if (case, m) not in _VS:
        ruleset, argmax = CASES[case]
        _VS[case, m] = run_vs(ruleset, argmax, member_weights(m))
    return _VS[case, m]


def run_league(case, pool_weights, members):
    L = load()
    ruleset, argmax = CASES[case]
    o, wa = fresh(ruleset), weights(SEED0)
    stacked = {k: np.ascontiguousarray(np.stack([w[k] for w in pool_weights])) for k in KEYS}
    mem = np.asarray(members, np.uint8)
    assert mem.size == (N + GROUP - 1) // GROUP
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **window_fields2(o, ruleset, 4242, argmax), opp=2, agent=wa, opponent=stacked, pool_size=len(pool_weights), opp_member=mem)
    assert ops > 0
    assert L.sr2_buffer_oob() == oob0                       # no weight fragment was requested outside its member's matrix
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
