"""GPU: the arena's window kernels at EVERY compiled shape -- azul_policy_rollout2_kernel<LID, 2, true> under both tile pools and
azul_x_policy_rollout_vs_kernel<P, D, true, true> for the five wide shapes -- by the argument of tests/test_gpu_arena.py: the games of a
group seated (a, o) equal, BIT FOR BIT, the same games of PolicyRollout(net_a, opponent=net_o) on the single-opponent window kernel of the
shape.  Three general-weight members; 35 games = groups of 16, 16 and 3; pairs (2, 0), (0, 2), (1, 1): with the league's seats [2, 0, 1]
(tests/test_gpu_league_shapes.py) every member index 0, 1 and 2 is read as opponent and as agent, the agent's critic (b2c + m) included,
and no group's agent sits on the member of the group's own index.  An arena keeps no trace of the opponent's answers (opp_replies only):
what the opponent played shows in what the agent observes next."""
import pytest

from tests.test_gpu_arena import _compare_with_singles
from tests.test_gpu_league_shapes import CASE_IDS, CASES, N, T, W, _differ, _entries, _nets

pytestmark = pytest.mark.gpu

PAIRS = [(2, 0), (0, 2), (1, 1)]


def compare_arena_with_singles(nets, pairs, players, rules, selection="Distribution"):
    return _compare_with_singles(nets, N, T, W, pairs, players, rules, selection, _entries(players, rules, "arena"))


@pytest.mark.parametrize("players,rules", CASES, ids=CASE_IDS)
def test_arena_of_every_shape_equals_the_single_opponent_rollout_of_every_pair(players, rules):
    got, singles = compare_arena_with_singles(_nets(players, rules, 72, 3), PAIRS, players, rules)
    for a, b in (((2, 0), (0, 2)), ((2, 0), (1, 1)), ((0, 2), (1, 1))):  # the pairs do play differently: the equality says something
        assert _differ(singles[a], singles[b]), (a, b)


def test_two_player_random_pool_arena_takes_the_first_maximum_of_every_pair():
    """action_selection "Max" (both seats) shares the member lookup: <false, 2, true> once on the argmax path."""
    players, rules = CASES[1]
    got, singles = compare_arena_with_singles(_nets(players, rules, 73, 3), PAIRS, players, rules, "Max")
    assert _differ(singles[2, 0], singles[0, 2])
