"""The ARENA inside the two-player window kernel on CPU: azul_policy_rollout2_kernel<LID, 2, true> (csrc/azul_rollout2.hpp, compiled
UNMODIFIED by g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_rollout2.cpp, sr2_window with opp 2 and both member
arrays) against the single-opponent kernel (the same entry without the arrays) run once per ordered pair with that pair's weights.  35 games -- two full 16-game groups and a
ragged group of three -- five steps, general weights, a pool of two, pairs (agent, opponent) [(1, 0), (0, 1), (1, 1)]: every output buffer,
record, MT19937 state, counter and trace of the games of a group must equal its pair's single-opponent run BYTE FOR BYTE.  Also: a pool of
one equals the single-opponent kernel on all games; a member named by no group is never read (poisoned with NaN in all six arrays, nothing
changes); an agent member past the pool is read as the last member and no weight fragment is requested outside its matrix."""
import numpy as np
import pytest

from tests.hostcheck import window
from tests.hostcheck.window import ARGMAX, CASES2 as CASES, GROUP, KEYS, N2 as N, SLOTS2 as SLOTS, games
from tests.hostcheck.window import fresh2 as fresh, load2 as load, member_weights2 as member_weights, window_fields2

PAIRS = [(1, 0), (0, 1), (1, 1)]
_VS = {}


def vs_reference(case, a, o):
    """The single-opponent run of agent = member a against opponent = member o: computed once per case and pair, shared, never modified."""
    if (case, a, o) not in _VS:
        L = load()
        ruleset, argmax = CASES[case]
        r = fresh(ruleset)
        oob0 = L.sr2_buffer_oob()
        ops = window.run(L, **window_fields2(r, ruleset, ARGMAX if argmax else 4242, argmax), opp=2, agent=member_weights(a),
                         opponent=member_weights(o))
        assert ops > 0 and L.sr2_buffer_oob() == oob0
        _VS[case, a, o] = r
    return _VS[case, a, o]


def run_arena(case, pool_weights, pairs):
    L = load()
    ruleset, argmax = CASES[case]
    r = fresh(ruleset)
    stacked = {k: np.ascontiguousarray(np.stack([w[k] for w in pool_weights])) for k in KEYS}
    am = np.asarray([p[0] for p in pairs], np.uint8)
    om = np.asarray([p[1] for p in pairs], np.uint8)
    assert am.size == (N + GROUP - 1) // GROUP
    oob0 = L.sr2_buffer_oob()
    ops = window.run(L, **window_fields2(r, ruleset, ARGMAX if argmax else 4242, argmax), opp=2, agent=stacked, pool_size=len(pool_weights),
                     agent_member=am, opp_member=om)
    assert ops > 0
    assert L.sr2_buffer_oob() == oob0                       # no weight fragment was requested outside its member's matrix
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
    assert (r["opp_replies"] > 0).any() and (r["opp_replies"] <= SLOTS).all()


def test_a_pool_of_one_is_the_single_opponent_kernel():
    case = "lid_distribution"
    r = run_arena(case, [member_weights(0)], [(0, 0)] * 3)
    ref = vs_reference(case, 0, 0)
    for k in r:
        assert r[k].tobytes() == ref[k].tobytes(), k


def test_an_unnamed_member_is_never_read_and_an_agent_past_the_pool_is_the_last_one():
    case = "lid_distribution"
    poison = {k: np.full_like(v, np.nan) for k, v in member_weights(0).items()}
    r = run_arena(case, [member_weights(0), member_weights(1), poison], PAIRS)
    assert_groups_equal(r, case, PAIRS)
    r = run_arena(case, [member_weights(0), member_weights(1)], [(7, 0), (0, 1), (7, 7)])     # 7 >= K = 2 reads as member 1 (run_arena checks the loads)
    assert_groups_equal(r, case, PAIRS)
