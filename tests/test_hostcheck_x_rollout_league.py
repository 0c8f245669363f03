"""The LEAGUE inside the wide window kernel on CPU: azul_x_policy_rollout_vs_kernel<3, 5, true> (csrc/azul_rollout2.hpp, compiled UNMODIFIED by
g++ and run as workgroups of eight emulated wavefronts: tests/hostcheck/simt_x_rollout.cpp, sxr_window with opp 2 and the member array) against the
single-opponent kernel (the same entry without the array) run once per pool member with that member's weights.  Three players on five displays, 19 games -- a full
16-game group and a ragged group of three -- five steps, general weights, groups assigned [1, 0] of a pool of two: every output buffer, record,
MT19937 state, counter and trace of the games of a member's group must equal that member's single-opponent run BYTE FOR BYTE.  Also: a pool
of one equals the single-opponent kernel on all games; an unused member's weights are never read (NaN poison); a member value past the pool is
read as the last member."""
import numpy as np
import pytest

from tests.hostcheck import window
from tests.hostcheck.window import CASES_X as CASES, GROUP, KEYS, NA, NX as N, OBS, SEED, games, head_fields, tail_fields
from tests.hostcheck.window import fresh_x as fresh, load_x as load, member_weights_x as member_weights, weights_x as weights

_VS = {}


def vs_reference(case, m):
    """The single-opponent run against member m: computed once per case and member, shared, never modified."""
    if (case, m) not in _VS:
        L = load()
        pool, argmax = CASES[case]
        o = fresh(pool)
        assert window.run(L, **head_fields(o, pool), opp=2, agent=weights(OBS, NA, SEED), opponent=member_weights(m), **tail_fields(o, argmax)) > 0
        _VS[case, m] = o
    return _VS[case, m]


def run_league(case, pool_weights, members):
    L = load()
    pool, argmax = CASES[case]
    o = fresh(pool)
    stacked = {k: np.ascontiguousarray(np.stack([x[k] for x in pool_weights])) for k in KEYS}
    mem = np.asarray(members, np.uint8)
    assert mem.size == (N + GROUP - 1) // GROUP
    oob0 = L.sxr_buffer_oob()
    assert window.run(L, **head_fields(o, pool), opp=2, agent=weights(OBS, NA, SEED), opponent=stacked, pool_size=len(pool_weights), opp_member=mem,
                      **tail_fields(o, argmax)) > 0
    assert L.sxr_buffer_oob() == oob0
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
