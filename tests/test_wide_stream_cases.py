"""The inputs of the wide self-play edge cases (tests/wide_stream_cases.py) satisfy their preconditions ON THE ORACLE ALONE -- no GPU, no
emulation: enough games of the regeneration sweep wrap inside each kind of step, the stopping seeds stop, the three sibling placements are
present -- and the shared comparison objects to a perturbed expectation (the negative controls of cases 1 and 5)."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests import wide_stream_cases as W


@pytest.mark.parametrize("cfg", W.CONFIGS, ids=W.config_id)
def test_regeneration_sweep_wraps_inside_every_kind_of_step(cfg):
    starts = [W.sweep_start(g) for g in range(W.SWEEP_N)]
    assert starts[0] == 624 and starts[1] == 623 and min(starts) == 624 - W.SWEEP_SPAN and max(starts[2:]) == 622
    census = W.sweep_census(W.sweep_streams(cfg, 5100), W.sweep_steps(cfg))
    print(W.config_id(cfg), census)
    assert min(census.values()) >= W.SWEEP_MIN, census


def test_a_sweep_started_one_index_off_fails_the_comparison():
    cfg = W.CONFIGS[0]
    es = [W.play_oracle(s, 60) for s in W.sweep_streams(cfg, 5100)[:8]]
    got = W.expectation_as_batch(es)
    for g, s in enumerate(W.sweep_streams(cfg, 5100, shift=1)[:8]):
        W.compare(es[g], got, g)
        W.must_differ(W.play_oracle(s, 60), got, g)


@pytest.mark.parametrize("which", sorted(W.STOP_CONFIGS))
def test_stopping_seeds_stop_in_all_three_sibling_placements(which):
    cfg, seeds, slots = W.stop_seeds(which)
    oks = [W.moves_until_stop(W.new_stream(int(sd), cfg), W.STOP_T) for sd in seeds]
    stopped = [g for g, ok in enumerate(oks) if ok < W.STOP_T]
    print(which, dict(zip(seeds.tolist(), oks)))
    assert stopped == sorted(slots) and len(stopped) >= 4
    assert all(0 < oks[g] < W.STOP_T - 2 for g in stopped)
    assert W.sibling_placements(stopped, len(seeds)) == {"half0", "half1", "pair"}
    # the expectation of a stopped game: marked slots after the stop, `stuck` raised by exactly their number; one slot off is caught
    es = [W.play_oracle(W.new_stream(int(sd), cfg), W.STOP_T) for sd in seeds]
    got = W.expectation_as_batch(es)
    for g in stopped:
        e = es[g]
        assert (e.action[e.ok + 1:] == -1).all() and (e.done[e.ok + 1:] == 2).all() and e.action[e.ok] >= 0 and e.mask[e.ok].any()
        assert (W.packed_words(e.action, e.done)[e.ok + 1:] == 0xFFFF02FF).all()
        W.compare(e, got, g)
        W.must_differ(W.shifted_stop(e, 1), got, g)
        W.must_differ(W.shifted_stop(e, -1), got, g)


def test_a_stopped_game_continues_from_its_post_failure_state_like_a_handed_in_one():
    """What the second launch is compared with: the oracle's stream goes on from the state its failing call left."""
    cfg, seeds, slots = W.stop_seeds("lid")
    s = W.new_stream(int(seeds[slots[0]]), cfg)
    e1 = W.play_oracle(s, W.STOP_T)
    e2 = W.play_oracle(s, 100)
    assert e1.ok < W.STOP_T and e2.stuck >= e1.stuck and (e2.action >= 0).any()


@pytest.mark.parametrize("players", [3, 4])
def test_flags_off_the_extended_stream_is_the_players_stream(players):
    a, b = oz.StreamX(77, players), oz.StreamNP(77, players)
    oa, ob = a.advance(500), b.advance(500)
    for k in ("mask", "action", "done"):
        assert np.array_equal(oa[k], ob[k])
    assert oa["rec_after"].tobytes() == ob["rec_after"].tobytes() and a.rng_state()[1] == b.rng_state()[1]


@pytest.mark.parametrize("cfg", [W.CONFIGS[0], W.CONFIGS[3]], ids=W.config_id)
def test_handed_in_finished_and_stuck_slots_restart_and_count_as_stuck(cfg):
    streams = W.hand_in_streams(cfg, 6200)
    for g in W.HAND_IN_ENDED + W.HAND_IN_STUCK:
        e = W.play_oracle(streams[g], 50)
        assert e.action[0] == -1 and e.done[0] == 2 and not e.mask[0].any() and e.stuck >= 1 and e.action[1] >= 0
    assert {g % 2 for g in W.HAND_IN_ENDED} == {0, 1} == {g % 2 for g in W.HAND_IN_STUCK}
