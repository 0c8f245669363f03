"""The wide self-play kernels (csrc/azul_rules_x.hpp: azul_x_selfplay_kernel<P, D, OUT, PAD, BITS>, two games per wavefront) ON THE GPU at
the edges the two-player kernel is pinned at (tests/test_gpu_selfplay.py): the MT19937 regeneration inside a move, a deal and a restart; odd
batches (the last wave plays one game) through every output instantiation; launches cut around the 128-move priority block; games handed in
mid-play, finished and stuck; games a rule error stops (OZ_BOX_EMPTY) and what the next launch does with them; the fp64 draw path; a soak.

Every case ends at the oracle: the cases and the comparison live in tests/wide_stream_cases.py, shared with the lockstep CPU emulation
(tests/test_hostcheck_rules_x.py), and tests/test_wide_stream_cases.py shows on the oracle alone that their preconditions hold.  The extended
rules are BEYOND THE REFERENCE, PARITY UNPINNED (tests/test_gpu_ext_rules.py): the reference there is the oracle's OZ_EXT_* restatement."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as oz
from tests import wide_stream_cases as W

pytestmark = pytest.mark.gpu

FP64_MARGIN = 0x7fffffff            # every draw within 2^31 of a multiple of 2^32: always the literal fp64 decision
VARIANTS = ("records", "padded+packed+bits", "padded+packed", "wide pitch", "dense", "subset+records", "none")
NO_STOP_49 = (4, oz.EXT_DISPLAYS_2P1 | oz.EXT_SHORT_DEAL | oz.EXT_END_BONUS) + W.LID        # nine displays, no game ever stops


def make_env(cfg, n, seed0=0, seeds=None, margin=0):
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    P, ext, first, pool = cfg
    env = BatchedAzul(n, rules=W.device_rules(first, pool), players=P, ext_rules=ext)
    assert env.wide and env.num_actions == W.num_actions(P, ext) and env.displays == W.displays(P, ext)
    if margin:
        env.set_draw_margin(margin)
    env.seed(seed0, seeds=seeds)
    env.init()
    assert (env.new_round().cpu().numpy() == 0).all()
    return env


def hand_over(env, streams):
    """The oracle's games and streams into the batch (azul_batch_set_state + azul_batch_set_rng), counters from zero."""
    rec = env.get_records()
    for g, s in enumerate(streams):
        rec[g] = np.frombuffer(s.record().tobytes(), dtype=rec.dtype)[0]
    env.set_records(rec)
    env.set_rng_range(np.stack([s.rng_state()[0] for s in streams]), np.array([s.rng_state()[1] for s in streams], np.uint32))
    env.reset_counters()


def launch(env, T, variant, parts=None):
    """One launch of T moves (or `parts`, for the variant without outputs) through the named output variant -> what it wrote, in the layout
    tests/wide_stream_cases.compare reads.  Every buffer is prefilled with junk except the record snapshots (bytes of absent players and the
    reserved tail of a wide record are not written)."""
    pad = W.PAD_PITCH[env.displays]
    if variant == "none":
        for k in parts or (T,):
            env.selfplay(k)
        tr, keys = {}, ()
    else:
        kw = {"records": dict(with_records=True),
              "padded+packed+bits": dict(packed_mask=True, mask_pitch=pad),
              "padded+packed": dict(packed_mask=True, mask_pitch=pad, mask_bits=False),
              "wide pitch": dict(packed_mask=True, mask_pitch=pad + 64),
              "dense": dict(packed_mask=True),
              "subset+records": dict(with_records=True, packed_mask=True)}[variant]
        tr = env.alloc_trajectory(T, **kw)
        for k in ("mask", "action", "reward", "done", "packed", "maskbits"):
            if k in tr:
                tr[k].fill_(0x6E if tr[k].dtype == torch.uint8 else -7)
        if variant == "subset+records":         # a run-time subset: no reward, no compact record
            env.selfplay(T, tr["mask"], tr["action"], None, tr["done"], records=tr["records"], maskbits=tr["maskbits"])
            keys = ("mask", "action", "done", "records", "maskbits")
        else:
            env.selfplay(T, tr["mask"], tr["action"], tr["reward"], tr["done"], records=tr.get("records"), maskbits=tr.get("maskbits"),
                         packed=tr.get("packed"))
            keys = tuple(tr)
    torch.cuda.synchronize()
    got = {("rec" if k == "records" else k): tr[k].cpu().numpy() for k in keys}
    got["final"] = env.get_records()
    got["mt"], got["pos"] = env.get_rng_range()
    cnt = env.counters()
    got.update(episodes=cnt["episodes"], stuck=cnt["stuck"], stat_sums=cnt["stat_sums"])
    return got


# ---- 1. the regeneration sweep ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_census(cfg):
    return W.sweep_census(W.sweep_streams(cfg, 5100), W.sweep_steps(cfg))


@pytest.mark.parametrize("margin", [0, FP64_MARGIN], ids=["integer", "fp64"])
@pytest.mark.parametrize("cfg", W.CONFIGS, ids=W.config_id)
def test_regeneration_inside_a_move_a_deal_and_a_restart(cfg, margin):
    """CPython's index placed at 624, 623 and over the last 150 words of the state when the run starts (96 games): the speculative two-word
    fetch takes its `hard` path (index 623 / 624), the parallel deal (deal_tiles2 / deal_parallel_x) and the restart fetch their words across
    the regeneration -- for at least 8 games each, counted on the oracle.  Records variant; with the integer draw and the literal fp64 one."""
    census = sweep_census(cfg)
    assert min(census.values()) >= W.SWEEP_MIN, census
    T = W.sweep_steps(cfg)
    streams = W.sweep_streams(cfg, 5100)
    env = make_env(cfg, W.SWEEP_N, 5100, margin=margin)
    mt, pos = env.get_rng_range()
    assert all(np.array_equal(mt[g], s.rng_state()[0]) for g, s in enumerate(streams))
    for g, s in enumerate(streams):
        env.set_rng(g, s.rng_state()[0], s.rng_state()[1])
    got = launch(env, T, "records")
    for g, s in enumerate(streams):
        W.compare(W.play_oracle(s, T), got, g, (W.config_id(cfg), margin))
    for g, s in enumerate(W.sweep_streams(cfg, 5100, shift=1)[:4]):          # negative control: the oracle started one index off
        W.must_differ(W.play_oracle(s, T), got, g)


# ---- 2. odd batches through every instantiation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 129])
@pytest.mark.parametrize("cfg", W.CONFIGS[:5] + [W.CONFIGS[7]], ids=W.config_id)
def test_odd_batches_write_the_oracles_bytes_through_every_instantiation(cfg, n):
    """OUT 0 (two launches), OUT 1 / PAD / BITS, OUT 1 / PAD, OUT 2 (dense rows; a run-time subset + record snapshots), a pitch larger than
    needed: every variant writes the oracle's bytes -- hence the same bytes -- for every game, the last one included, whose wave plays ONE game."""
    T, seed = 150, 4711
    parts = (T // 2, T - T // 2)
    want = [W.play_oracle(W.new_stream(seed + g, cfg), T) for g in range(n)]
    in_parts = []                                        # two launches: a game that stops in the first is played on by the second
    for g in range(n):
        s = W.new_stream(seed + g, cfg)
        in_parts.append([W.play_oracle(s, k) for k in parts][-1])
    for variant in VARIANTS:
        got = launch(make_env(cfg, n, seed), T, variant, parts=parts)
        for g in range(n):
            W.compare(in_parts[g] if variant == "none" else want[g], got, g, (W.config_id(cfg), n, variant))


# ---- 3. launches cut around the 128-move priority block -----------------------------------------------------------------------------------------
CHUNKS = (1, 3, 127, 128, 129, 62)


@pytest.mark.parametrize("cfg", [W.CONFIGS[2], NO_STOP_49], ids=W.config_id)
def test_launch_lengths_around_the_priority_block_are_invisible_wide(cfg):
    n, seed, T = 66, 811, sum(CHUNKS)
    one = launch(make_env(cfg, n, seed), T, "padded+packed+bits")
    streams = [W.new_stream(seed + g, cfg) for g in range(n)]
    for g, s in enumerate(streams):
        e = W.play_oracle(s, T)
        assert e.ok == T                                 # (no game of these stops: a stopped game is played on by the next launch, case 5)
        W.compare(e, one, g, (W.config_id(cfg), "one launch"))
    env = make_env(cfg, n, seed)
    streams = [W.new_stream(seed + g, cfg) for g in range(n)]
    for k in CHUNKS:
        part = launch(env, k, "padded+packed+bits")
        for g, s in enumerate(streams):
            W.compare(W.play_oracle(s, k), part, g, (W.config_id(cfg), "chunk", k))
    assert part["final"].tobytes() == one["final"].tobytes() and np.array_equal(part["mt"], one["mt"])


def test_launch_lengths_around_the_priority_block_are_invisible_two_players():
    """The same for azul_selfplay2_kernel (128-byte record), against oz.Stream: one launch of T and launches of 1, 3, 127, 128, 129, 62."""
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    n, seed, T = 66, 811, sum(CHUNKS)

    def start():
        env = BatchedAzul(n)
        env.seed(seed)
        env.runner_init()
        env.runner_init()
        return env, [oz.Stream(seed + g) for g in range(n)]

    def play(env, streams, k):
        t = env.alloc_trajectory(k)
        env.selfplay(k, t["mask"], t["action"], t["reward"], t["done"])
        torch.cuda.synchronize()
        out = {key: t[key].cpu().numpy() for key in ("mask", "action", "reward", "done")}
        final, cnt = env.get_records(), env.counters()
        mts, poss = env.get_rng_range()
        for g, s in enumerate(streams):
            o = s.advance(k, want_records=False)
            for key in out:
                assert np.array_equal(o[key], out[key][:, g]), (k, g, key)
            assert s.record().tobytes() == final[g].tobytes(), (k, g)
            assert np.array_equal(s.rng_state()[0], mts[g]) and s.rng_state()[1] == int(poss[g]), (k, g)
            assert int(cnt["episodes"][g]) == int(s.episodes.value) and int(cnt["stuck"][g]) == int(s.stuck.value), (k, g)
            assert np.array_equal(cnt["stat_sums"][g], s.stats_sum), (k, g)
        return final

    a = play(*start(), T)
    env, streams = start()
    for k in CHUNKS:
        b = play(env, streams, k)
    assert a.tobytes() == b.tobytes()


# ---- 4. games handed in mid-play, finished and stuck --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", W.CONFIGS, ids=W.config_id)
def test_games_handed_in_mid_play_finished_and_stuck_continue_like_the_oracle(cfg):
    """The wide counterpart of test_games_handed_in_mid_play_continue_exactly_like_the_oracle: the oracle plays g * 11 + 3 moves of game g, the
    state goes in with set_records + set_rng, counters are reset, 400 moves follow.  In the same batch a record with the ended flag and a stuck
    state (displays empty, only the first-player token in the centre), each once in half 0 and once in half 1 of a wave: action -1, done 2, an
    empty mask row, a restart and one more in `stuck`, as the oracle's stream does from that state."""
    streams = W.hand_in_streams(cfg, 6200)
    env = make_env(cfg, W.HAND_IN_N, 1)
    hand_over(env, streams)
    got = launch(env, W.HAND_IN_T, "padded+packed+bits")
    for g, s in enumerate(streams):
        e = W.play_oracle(s, W.HAND_IN_T)
        if g in W.HAND_IN_ENDED + W.HAND_IN_STUCK:
            assert e.action[0] == -1 and e.done[0] == 2 and not e.mask[0].any() and e.stuck >= 1
            assert got["action"][0, g] == -1 and got["done"][0, g] == 2 and int(got["stuck"][g]) >= 1
        W.compare(e, got, g, (W.config_id(cfg),))
    assert {g % 2 for g in W.HAND_IN_ENDED} == {0, 1} == {g % 2 for g in W.HAND_IN_STUCK}


# ---- 5. games a rule error stops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["records", "padded+packed", "padded+packed+bits"])
@pytest.mark.parametrize("which", sorted(W.STOP_CONFIGS))
def test_stopped_games_are_marked_exactly_and_the_next_launch_plays_them_on(which, variant):
    """OZ_BOX_EMPTY (bag and lid empty without the short-deal rule) in half 0 beside a live sibling, in half 1 beside a live sibling and
    beside another stopped game: the exact pin of tests/wide_stream_cases.py -- slots before the stop, the stopping slot, the marked slots
    (into junk-filled buffers), final record, stream, `stuck` = the oracle's + T - ok - 1, the live siblings to the end.  Then ~100 more
    moves: the stopped games play on from their records like the oracle from its own post-failure state (a finding either way is recorded in
    DESIGN.md and include/azul_hip.h)."""
    cfg, seeds, slots = W.stop_seeds(which)
    n, T = len(seeds), W.STOP_T
    env = make_env(cfg, n, seeds=seeds)
    streams = [W.new_stream(int(sd), cfg) for sd in seeds]
    got = launch(env, T, variant)
    es = [W.play_oracle(s, T) for s in streams]
    stopped = [g for g, e in enumerate(es) if e.ok < T]
    assert len(stopped) >= 4 and stopped == sorted(slots)
    assert W.sibling_placements(stopped, n) == {"half0", "half1", "pair"}
    for g, e in enumerate(es):
        W.compare(e, got, g, (which, variant))
    for g in stopped:                                    # negative controls: the stop believed one slot later / earlier
        W.must_differ(W.shifted_stop(es[g], 1), got, g)
        W.must_differ(W.shifted_stop(es[g], -1), got, g)
    again = launch(env, 100, variant)
    for g, s in enumerate(streams):
        W.compare(W.play_oracle(s, 100), again, g, (which, variant, "second launch"))


# ---- 6. the fp64 draw path in self-play ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [W.CONFIGS[0], W.CONFIGS[2], NO_STOP_49], ids=W.config_id)
def test_fp64_draw_path_plays_the_integer_paths_bytes(cfg):
    n, T, seed = 64, 400, 321
    a = launch(make_env(cfg, n, seed), T, "none")
    b = launch(make_env(cfg, n, seed, margin=FP64_MARGIN), T, "none")
    assert a["final"].tobytes() == b["final"].tobytes() and np.array_equal(a["mt"], b["mt"]) and np.array_equal(a["pos"], b["pos"])
    assert np.array_equal(a["episodes"], b["episodes"]) and np.array_equal(a["stat_sums"], b["stat_sums"])
    for g in range(0, n, 7):
        e = W.play_oracle(W.new_stream(seed + g, cfg), T)
        W.compare(e, a, g, (W.config_id(cfg), "integer"))
        W.compare(e, b, g, (W.config_id(cfg), "fp64"))


# ---- 7. soak ------------------------------------------------------------------------------------------------------------------------------------
# episodes of games 0 / 101 / 255 (seeds 31337 + g) after 65,536 moves, READ OFF THE ORACLE (oz.StreamX(...).advance(65536); episodes):
#   three players, five displays, reference rules: 1038 / 1041 / 1043;  four players, nine displays, short deal + end bonus: 750 / 754 / 755.
# The bound asked of every sampled game is the smallest of its three counts, rounded down to the hundred.
SOAK_EPISODES = {W.CONFIGS[0]: (1038, 1041, 1043), NO_STOP_49: (750, 754, 755)}


@pytest.mark.parametrize("cfg", [W.CONFIGS[0], NO_STOP_49], ids=W.config_id)
def test_long_run_soak_wide(cfg):
    """65,536 moves per game in 4096-move launches on 256 games: three sampled games equal the oracle -- final record, all 624 words + index,
    `episodes`, `stuck` and the statistics sums."""
    n, steps, seed = 256, 65536, 31337
    floor = min(SOAK_EPISODES[cfg]) // 100 * 100
    assert floor >= 300
    env = make_env(cfg, n, seed)
    got = launch(env, steps, "none", parts=(4096,) * (steps // 4096))
    for i, g in enumerate((0, 101, 255)):
        s = W.new_stream(seed + g, cfg)
        s.advance(steps, want_records=False)
        assert int(s.episodes.value) == SOAK_EPISODES[cfg][i]
        e = W.Expect()
        e.T, e.ok, e.mask = 0, 0, np.zeros((0, s.num_actions), np.uint8)
        e.final, (e.mt, e.pos) = W.record_bytes(s), s.rng_state()
        e.episodes, e.stuck, e.stat_sums = int(s.episodes.value), int(s.stuck.value), s.stats_sum
        W.compare(e, got, g, (W.config_id(cfg),))
        assert int(got["episodes"][g]) > floor
