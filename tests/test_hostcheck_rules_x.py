"""The P-player / D-display rules on CPU: csrc/azul_rules_x.hpp (two games per wavefront; the bodies of azul_x_op_kernel and
azul_x_selfplay_kernel) compiled UNMODIFIED by g++ and run under the lockstep 64-lane emulation of tests/hostcheck/simt, against the
oracle -- masks, actions, done flags, 256-byte record snapshots, final records, all 624 MT19937 words + positions, episode / stuck
counters, statistics sums.

  * flags off, five displays, P = 3, 4: the reference's own behaviour (azulnet/azul.py:18-33, 64-89, 118-313; game_runner.py:87-97),
    PINNED -- the same streams tests/golden/traj_players_selfplay.npz records from the real reference are replayed.
  * each extended rule on (2P+1 displays, end-of-game bonuses, short deal, finite bag): BEYOND THE REFERENCE, PARITY UNPINNED -- the
    oracle's OZ_EXT_* restatement of the rulebook (cross-checked by tests/ext_rules_model.py) is the comparison."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as oz
from tests import wide_stream_cases as W
from tests.hostcheck import hostcheck

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
XOP = {"query": 0, "init": 1, "new_round": 2, "move": 3, "next_player": 4, "count_score": 5, "step": 6, "random_action": 7, "sample_mask": 8}


def load(name=None):
    name = name or os.environ.get("AZUL_SIMT_X_LIB", "libsimt_rules_x.so")        # run_sanitizers.sh: the _ubsan / _asan builds
    L = C.CDLL(hostcheck.build(name))
    L.shx_selfplay.restype = C.c_longlong
    L.shx_selfplay.argtypes = ([C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_ulonglong, C.c_int, C.c_int, C.c_void_p, C.c_int]
                               + [C.c_void_p] * 6)
    L.shx_op.restype = C.c_int
    L.shx_op.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_ulonglong, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def split_ext(pool, ext):
    """(device pool code, end_bonus, short_deal, displays rule) from the oracle's tile_pool + OZ_EXT_* flags."""
    xpool = 2 if ext & oz.EXT_FINITE_BAG else (1 if pool == oz.POOL_LID else 0)
    return xpool, int(bool(ext & oz.EXT_END_BONUS)), int(bool(ext & oz.EXT_SHORT_DEAL))


class Emulated:
    """A batch under the emulation: the arrays a device batch keeps (records, MT19937 states + indices, counters) live here across launches."""

    def __init__(self, L, cfg, streams, margin=0):
        self.L, self.cfg, self.margin, self.n = L, cfg, margin, len(streams)
        P, ext, first, pool = cfg
        self.D = W.displays(P, ext)
        self.NA = W.num_actions(P, ext)
        n = self.n
        self.state = np.stack([W.record_bytes(s) for s in streams]).copy()
        self.mt = np.stack([s.rng_state()[0] for s in streams]).astype(np.uint32).copy()
        self.pos = np.array([s.rng_state()[1] for s in streams], dtype=np.uint32)
        self.ep, self.stuck, self.ss = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, 10))

    def launch(self, T, variant):
        """-> what the launch wrote, in the layout tests/wide_stream_cases.compare reads; every buffer is prefilled with junk except the
        record snapshots (a wide record's absent players and reserved tail are not written)."""
        P, ext, first, pool = self.cfg
        n, NA, D = self.n, self.NA, self.D
        pitch = W.PAD_PITCH[D] if variant in (0, 1) else NA
        NL = (NA + 63) // 64
        out = {}
        if variant != 4:
            out = {"mask": np.full((T, n, pitch), 0xEE, np.uint8), "action": np.full((T, n), -7, np.int32), "reward": np.full((T, n), -7, np.int32),
                   "done": np.full((T, n), 9, np.uint8)}
            if variant == 0:
                out["maskbits"] = np.full((T, n, NL), 0x5A5A5A5A5A5A5A5A, np.uint64)
            if variant != 3:
                out["packed"] = np.full((T, n), 0x77777777, np.uint32)
            else:
                out["rec"] = np.zeros((T, n, 256), np.uint8)
                out["maskbits"] = np.full((T, n, NL), 0x5A5A5A5A5A5A5A5A, np.uint64)
        xpool, eb, sd = split_ext(pool, ext)
        ops = self.L.shx_selfplay(n, P, D, ptr(self.state), ptr(self.mt), ptr(self.pos), ptr(self.ep), ptr(self.stuck), ptr(self.ss), first, xpool, eb,
                                  sd, self.margin, T, variant, ptr(out.get("mask")), pitch, ptr(out.get("maskbits")), ptr(out.get("action")),
                                  ptr(out.get("reward")), ptr(out.get("done")), ptr(out.get("packed")), ptr(out.get("rec")))
        assert ops > 0
        out.update(final=self.state, mt=self.mt, pos=self.pos, episodes=self.ep, stuck=self.stuck, stat_sums=self.ss)
        return out


def run_streams(L, P, first, pool, ext, n, T, variant, seed0, margin=0, prepare=None):
    cfg = (P, ext, first, pool)
    streams = [W.new_stream(seed0 + g, cfg) for g in range(n)]
    if prepare:
        prepare(streams)
    emu = Emulated(L, cfg, streams, margin)
    out = emu.launch(T, variant)
    return streams, emu.state, emu.mt, emu.pos, emu.ep, emu.stuck, emu.ss, out, emu.NA


def check_streams(L, P, first, pool, ext, n, T, variant, seed0, margin=0, prepare=None):
    """Every game against the shared expectation (tests/wide_stream_cases.py) -- a game that stops on OZ_BOX_EMPTY included, exactly: the
    slots before the stop, the stopping slot, the marked slots after it, final record, stream, counters."""
    streams, state, mt, pos, ep, stuck, ss, out, NA = run_streams(L, P, first, pool, ext, n, T, variant, seed0, margin, prepare)
    stopped = 0
    for g, s in enumerate(streams):
        e = W.play_oracle(s, T)
        if e.ok < T:
            assert not ext & oz.EXT_SHORT_DEAL, (P, first, pool, ext, variant, g)
            stopped += 1
        W.compare(e, out, g, (P, first, pool, ext, variant))
    check_streams.stopped = stopped
    return int(ep.sum())


@pytest.mark.parametrize("players", [3, 4])
def test_flags_off_replays_the_reference_generated_streams(players):
    """PINNED: tests/golden/traj_players_selfplay.npz holds what the REAL reference plays (Azul(players=P) + its RandomAgent on the global
    stream); the emulated kernel body must produce those masks / actions / done flags from the same seeds."""
    L = load()
    gold = np.load(os.path.join(GOLDEN, "traj_players_selfplay.npz"))
    seen = 0
    for i, key in enumerate(gold["index_key"]):
        if int(gold["index_players"][i]) != players:
            continue
        key, seed, first, pool = str(key), int(gold["index_seed"][i]), int(gold["index_first"][i]), int(gold["index_pool"][i])
        if seed % 3:                                             # every third stream: the emulation runs a fiber per lane
            continue
        T = min(len(gold[key + "_action"]), 220)
        streams, state, mt, pos, ep, stuck, ss, out, NA = run_streams(L, players, first if first >= 0 else 1, pool, 0, 1, T, 3, seed)
        assert np.array_equal(np.packbits(out["mask"][:, 0, :180].astype(bool), axis=1, bitorder="little"), gold[key + "_mask"][:T]), key
        assert np.array_equal(out["action"][:, 0], gold[key + "_action"][:T]), key
        assert np.array_equal(out["done"][:, 0], gold[key + "_done"][:T]), key
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("players", [2, 3, 4])
def test_flags_off_two_games_per_wave_equals_the_oracle(players):
    L = load()
    eps = 0
    for (first, pool) in ((oz.FIRST_RANDOM, oz.POOL_LID), (1, oz.POOL_RANDOM), (2, oz.POOL_LID)):
        for variant in (0, 3, 4):
            eps += check_streams(L, players, first, pool, 0, n=3, T=150, variant=variant, seed0=40 + variant)
    assert eps > 0


EXT_CASES = [oz.EXT_END_BONUS, oz.EXT_SHORT_DEAL, oz.EXT_FINITE_BAG, oz.EXT_DISPLAYS_2P1,
             oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS | oz.EXT_SHORT_DEAL, oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS | oz.EXT_SHORT_DEAL | oz.EXT_FINITE_BAG]


@pytest.mark.parametrize("players", [2, 3, 4])
@pytest.mark.parametrize("ext", EXT_CASES)
def test_beyond_the_reference_parity_unpinned_each_flag_equals_the_oracle(players, ext):
    L = load()
    for (first, pool) in ((oz.FIRST_RANDOM, oz.POOL_LID), (1, oz.POOL_RANDOM)):
        if pool == oz.POOL_LID and ext & oz.EXT_FINITE_BAG:
            continue
        for variant in (1, 3):
            check_streams(L, players, first, pool, ext, n=3, T=140, variant=variant, seed0=900 + ext)


def dense_walls(streams):
    """Crafted states: every wall almost full (every row misses one cell), so that rows, columns and colours complete within a few
    moves and the bonus arithmetic -- per round (reference) or at the end (beyond the reference) -- is exercised hard."""
    rng = np.random.default_rng(7)
    for s in streams:
        s.advance(6)
        w = s.g.arr("walls")
        for p in range(s.g.players):
            w[p] = 1
            for r in range(5):
                w[p, r, rng.integers(5)] = 0
            if p == 0:
                w[p, :, 3] = 1                        # player 0: colour 3 complete already
        s.g.arr("score")[: s.g.players] = rng.integers(0, 40, s.g.players)


@pytest.mark.parametrize("players", [2, 3, 4])
@pytest.mark.parametrize("ext", [0, oz.EXT_END_BONUS, oz.EXT_END_BONUS | oz.EXT_DISPLAYS_2P1])
def test_line_bonuses_on_dense_walls_per_round_and_at_the_end(players, ext):
    """ext = 0: azul.py:266-295 (bonuses in the round the tile lands, pinned through the oracle); with the end-of-game switch: BEYOND
    THE REFERENCE, PARITY UNPINNED.  Also a negative control: the two rules really differ on these states."""
    L = load()
    eps = check_streams(L, players, oz.FIRST_RANDOM, oz.POOL_LID, ext, n=4, T=60, variant=3, seed0=77, prepare=dense_walls)
    assert eps >= 4
    if ext == oz.EXT_END_BONUS:
        a = [oz.StreamX(77 + g, players, ext=0) for g in range(4)]
        b = [oz.StreamX(77 + g, players, ext=ext) for g in range(4)]
        dense_walls(a)
        dense_walls(b)
        ra = np.stack([s.advance(60)["rec_after"]["score"] for s in a])
        rb = np.stack([s.advance(60)["rec_after"]["score"] for s in b])
        assert not np.array_equal(ra, rb)


def near_the_end_of_the_state(streams):
    """Stream positions spread over the last hundred words of the MT19937 state: the round that is dealt after the first ~11 moves then
    fetches its 40 / 56 / 72 words across a regeneration for several of the games."""
    for i, s in enumerate(streams):
        s.r.idx = 624 - 100 + 6 * i


@pytest.mark.parametrize("players,ext", [(3, 0), (3, oz.EXT_DISPLAYS_2P1), (4, oz.EXT_DISPLAYS_2P1 | oz.EXT_SHORT_DEAL)])
def test_factory_draw_across_a_regeneration_and_through_the_fp64_path(players, ext):
    """The parallel draw (five displays: az2::deal_tiles2; seven / nine: deal_parallel_x, 28 or 32 + 4 draws) with its words straddling an
    MT19937 regeneration, and -- with a draw margin that covers every draw -- the literal fp64 decision on the fetched words."""
    L = load()
    check_streams(L, players, oz.FIRST_RANDOM, oz.POOL_LID, ext, n=16, T=40, variant=3, seed0=300, prepare=near_the_end_of_the_state)
    check_streams(L, players, oz.FIRST_RANDOM, oz.POOL_LID, ext, n=4, T=60, variant=3, seed0=310, margin=0x7fffffff)
    check_streams(L, players, oz.FIRST_RANDOM, oz.POOL_LID, ext, n=8, T=30, variant=3, seed0=320, margin=0x7fffffff, prepare=near_the_end_of_the_state)


@pytest.mark.parametrize("players,ext,n", [(3, 0, n) for n in (1, 2, 15, 16, 17, 19)] + [(4, oz.EXT_DISPLAYS_2P1, 17)],
                         ids=lambda v: str(v))
def test_the_kernels_own_grid_plays_every_game_once(players, ext, n):
    """azul_x_selfplay_kernel's XCD placement (blockIdx.x -> the wave's pair of games) under the emulation, launched with the true grid of
    ceil(n / 2) blocks: 1, 1, 8, 8, 9 and 10 blocks -- a grid below eight, exactly eight, and the remainders 1 and 2 of the split over the
    eight XCDs.  Every game's slots, record, stream and counters equal the oracle's stream of its GLOBAL id (seed0 + g), which holds only if
    the placement is a permutation that plays each game once.  (4, 9) beside (3, 5): the 51-row and the 31-row sampling table, each in the
    LDS the kernel itself declares for its shape."""
    check_streams(load(), players, oz.FIRST_RANDOM, oz.POOL_LID, ext, n=n, T=30, variant=3, seed0=500)


# ---- the edges of the wide self-play kernels, stated once in tests/wide_stream_cases.py (the GPU runs the same cases on whole batches:
# tests/test_gpu_wide_selfplay_edges.py) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(W.STOP_CONFIGS))
def test_a_stopped_game_is_pinned_exactly_and_a_second_launch_plays_it_on(which):
    """OZ_BOX_EMPTY: slots before the stop, the stopping slot, the marked slots, final record = the oracle's after its failing call, all 624
    words + index, `stuck` = the oracle's + exactly T - ok - 1; a stopped game beside a live sibling in either half and beside another stopped
    game.  `dead` is a local of one launch: the next launch plays the record on like any handed-in state -- the oracle continued from its own
    post-failure state."""
    L = load()
    cfg, seeds, slots = W.stop_seeds(which)
    oks = {g: W.moves_until_stop(W.new_stream(int(seeds[g]), cfg), W.STOP_T) for g in slots}
    first = sorted(slots, key=lambda g: oks[g])[:3]              # the three earliest stops (the emulation runs a fiber per lane)
    T = max(oks[g] for g in first) + 12
    pick = [first[0], 1, 2, first[1], first[2], first[1]]        # X. | .X | XX : half 0 / half 1 beside a live sibling, a stopped pair
    pick[1], pick[2] = [g for g in range(len(seeds)) if g not in slots][:2]
    for variant in (3, 1, 0):
        streams = [W.new_stream(int(seeds[g]), cfg) for g in pick]
        emu = Emulated(L, cfg, streams)
        out = emu.launch(T, variant)
        es = [W.play_oracle(s, T) for s in streams]
        stopped = [g for g, e in enumerate(es) if e.ok < T]
        assert stopped == [0, 3, 4, 5] and W.sibling_placements(stopped, 6) == {"half0", "half1", "pair"}
        for g, e in enumerate(es):
            W.compare(e, out, g, (which, variant))
        W.must_differ(W.shifted_stop(es[0], 1), out, 0)
        W.must_differ(W.shifted_stop(es[0], -1), out, 0)
        if variant == 3:
            out2 = emu.launch(40, variant)
            for g, s in enumerate(streams):
                W.compare(W.play_oracle(s, 40), out2, g, (which, variant, "second launch"))


@pytest.mark.parametrize("cfg", [W.CONFIGS[0], W.CONFIGS[3]], ids=W.config_id)
def test_handed_in_games_finished_and_stuck_slots_continue_like_the_oracle(cfg):
    L = load()
    keep = [0, 1, 2, 3, W.HAND_IN_ENDED[0], W.HAND_IN_ENDED[1], W.HAND_IN_STUCK[0] - 1, W.HAND_IN_STUCK[0], W.HAND_IN_STUCK[1], W.HAND_IN_STUCK[1] + 1]
    allg = W.hand_in_streams(cfg, 6200)
    streams = [allg[g] for g in keep]                    # ended flag in half 0 and half 1, stuck in half 1 and half 0
    emu = Emulated(L, cfg, streams)
    out = emu.launch(60, 3)
    for g, s in enumerate(streams):
        e = W.play_oracle(s, 60)
        if keep[g] in W.HAND_IN_ENDED + W.HAND_IN_STUCK:
            assert e.action[0] == -1 and e.done[0] == 2 and e.stuck >= 1
        W.compare(e, out, g, (W.config_id(cfg), keep[g]))
