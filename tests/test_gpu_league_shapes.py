"""GPU: the league's window kernels at EVERY compiled shape -- the two-player kernel under both tile pools (azul_policy_rollout2_kernel<LID, 2>
with opp_member set, LID true and false) and azul_x_policy_rollout_vs_kernel<P, D, true> for the five wide shapes.

league_member<IN, NA> computes a member's base address from the compiled shape, so a wrong stride for NA = 240 / 300 or IN = 198 / 240 / 260
does not show at (188, 180).  The argument is the one of tests/test_gpu_league.py: a game's trajectory is keyed by its global id, so the
games of a group seated on member m equal, BIT FOR BIT, the same games of PolicyRollout(policy, opponent=member m) on the single-opponent
window kernel of the shape (itself pinned to the per-cut path and the oracle in tests/test_gpu_mp_fused_vs.py and
tests/test_policy_vs_policy_gpu.py).  General weights; three members; 35 games = groups of 16, 16 and 3 (a ragged last workgroup); seats
[2, 0, 1], so that no group sits on the member of its own index and a zero offset, a swapped offset or an error of one stride cannot
cancel (tests/test_gpu_arena_shapes.py seats the complementary pairs)."""
import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.pool import checked_seats
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from tests.test_gpu_league import GROUP, R, RULES2, _eq_games, _eq_state, _groups, _play, _rollout, _wide
from tests.test_gpu_mp_fused_rollout import SHAPES, SHAPE_IDS, _dims

pytestmark = pytest.mark.gpu

# two players on the reference's records with either tile pool (a fixed first player: <LID = false> without "Random" twice), then the wide shapes
CASES = [(2, RULES2), (2, {"first_player": 2, "tile_pool": "Random"})] + SHAPES
CASE_IDS = ["two_lid", "two_random"] + SHAPE_IDS
N, T, W = 35, 8, 2
SEATS = [2, 0, 1]


def _nets(players, rules, seed, count):
    torch.manual_seed(seed)
    n_obs, n_act = _dims(players, rules)
    return [BatchedActorCritic(n_obs, n_act, 180).cuda() for _ in range(count)]


def _entries(players, rules, pool="league"):
    mp = "mp_" if _wide(players, rules) else ""
    return "azul_batch_%spolicy_rollout_%s" % (mp, pool), "azul_batch_%spolicy_rollout_vs" % mp


class SeatedLeague(PolicyRollout):
    """A league whose groups are seated AT construction.  PolicyRollout seats group i on member i % K and takes no argument for it, and the
    openings at construction are played by the seated member: after a set_assignment() the games of a group would not be the games of a
    single-opponent rollout any more.  The seats go where an arena's first pairs go (NetPool, before the parts open their games)."""

    def __init__(self, *args, seats, **kw):
        self._first_seats = np.asarray([seats])
        super().__init__(*args, **kw)

    def _stage_weights(self, kweights, seats=None):
        G = (self.h + GROUP - 1) // GROUP
        super()._stage_weights(kweights, checked_seats(self._first_seats, (1, G), len(self.opp_pool), "seats are", "[1][G]", "seats name"))


def _league(policy, pool, seats, players, rules, selection="Distribution", n=N):
    sw = dict(fused_wide=True, fused_opponent=True) if _wide(players, rules) else dict(persistent=True)
    return SeatedLeague(policy, seats=seats, n_games=n, rules=rules, seed_base=11, window=T, opponent=pool, players=players, opponent_trace=R,
                        action_selection=selection, opponent_selection=selection, sample_seed=0x1234, use_graph=False, **sw)


def _differ(a, b):
    """Two runs' first windows differ in what was played (the agent's actions, or the opponent's where they are traced)."""
    return any(not torch.equal(a[0][0][k], b[0][0][k]) for k in ("action", "opp_action") if k in a[0][0])


def _all_finite(trajs):
    return all(bool(torch.isfinite(v).all()) for tr in trajs for v in tr.values() if v.is_floating_point())


def compare_league_with_singles(policy, pool, seats, players, rules, selection="Distribution"):
    """The league seated `seats` against the single-opponent rollout of every member it names: entry, seats read back, every group, window
    and trajectory array, and the games' state after the last window.  Returns the league's windows and the singles by member."""
    league_entry, vs_entry = _entries(players, rules)
    ro = _league(policy, pool, seats, players, rules, selection)
    assert ro.window_entry == league_entry and ro.pool_size == len(pool) and ro.assignment().tolist() == [seats]
    lg, slg = _play(ro, W)
    singles = {}
    for m in sorted(set(seats)):
        single = _rollout(policy, pool[m], N, T, players, rules, selection=selection)
        assert single.window_entry == vs_entry
        singles[m] = _play(single, W)
    for m, idx in _groups(N, seats):                                     # (the openings at construction included: slot 0 of window 0)
        for w in range(W):
            _eq_games(lg[w], singles[m][0][w], idx, "member %d window %d" % (m, w))
        _eq_state(slg, singles[m][1], idx, "member %d" % m)
    assert int(lg[0]["opp_replies"].sum()) > N * T // 2
    return lg, singles


@pytest.mark.parametrize("players,rules", CASES, ids=CASE_IDS)
def test_league_of_every_shape_equals_the_single_opponent_rollouts_per_group(players, rules):
    policy, *pool = _nets(players, rules, 71, 4)
    lg, singles = compare_league_with_singles(policy, pool, SEATS, players, rules)
    for a, b in ((0, 1), (0, 2), (1, 2)):                                # the members do answer differently: the equality says something
        assert _differ(singles[a], singles[b]), (a, b)
