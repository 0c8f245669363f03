"""What a wide self-play stream (csrc/azul_rules_x.hpp: azul_x_selfplay_kernel<P, D, OUT, PAD, BITS>, two games per wavefront) must
write, stated ONCE on the oracle's side: the GPU tests (tests/test_gpu_wide_selfplay_edges.py, tests/test_gpu_ext_rules.py) and the
lockstep CPU emulation (tests/test_hostcheck_rules_x.py) build their cases here and compare through `compare`, so both ask the same.

The reference of every case is oz.StreamX (oz_stream_x_*; with ext == 0 it plays oz.StreamNP's loop, which tests/test_wide_stream_cases.py
checks) on the same seeds or the same handed-in state.  No torch, no GPU: everything here runs on the oracle alone.

A game that a rule error STOPS (bag and lid empty without the short-deal rule: OZ_BOX_EMPTY, where the reference raises inside
random.choices, azul.py:86-87) is pinned exactly, after include/azul_hip.h (azul_batch_selfplay).  With `ok` = the moves the oracle completes:
  * slots < ok     the oracle's;
  * slot ok        the mask of the state before the failing step, the RandomAgent's pick on it, done 0 (the move is played, the game has not
                   ended; its next round cannot be dealt), the record snapshot = the final record;
  * slots > ok     action -1, done 2, reward 0, an empty mask row, the compact word of a stuck slot, zero mask bits, snapshot = final record;
  * final record, all 624 MT19937 words and the index: the oracle's after its failing call (the step mutates the game in place);
  * `stuck` = the oracle's + exactly T - ok - 1; `episodes` and the statistics sums: the oracle's.
A LATER launch plays the stopped game on from that record like any handed-in state (`dead` is a local of one launch): the oracle continued
from its own post-failure state is the reference."""
import copy
import ctypes as C

import numpy as np

from oracle import oracle as oz

LID = (oz.FIRST_RANDOM, oz.POOL_LID)
RND = (1, oz.POOL_RANDOM)
BAG = oz.EXT_DISPLAYS_2P1 | oz.EXT_FINITE_BAG
# (players, ext): five displays with 3 and 4 players, 2P+1 displays (7 / 9), and the wide record with two players
SHAPES = [(3, 0), (4, 0), (3, oz.EXT_DISPLAYS_2P1), (4, oz.EXT_DISPLAYS_2P1), (2, oz.EXT_END_BONUS)]
# (players, ext, first_player, tile_pool): "Lid" + first player Random for every shape, the Random pool, the finite bag on nine displays
CONFIGS = [s + LID for s in SHAPES] + [(3, 0) + RND, (4, oz.EXT_DISPLAYS_2P1) + RND, (4, BAG) + RND]
PAD_PITCH = {5: 192, 7: 256, 9: 320}

# Seeds whose games stop on OZ_BOX_EMPTY within 700 moves (found with the oracle; tests/test_wide_stream_cases.py rechecks every one):
# P = 4, nine displays, "Lid" pool, first player Random / the same with the finite bag on the Random pool.
# name: (config, seeds that stop, seeds that play on)
STOP_CONFIGS = {
    "lid": ((4, oz.EXT_DISPLAYS_2P1) + LID, [5108, 5109, 5114, 5130], [7000, 7001, 7002, 7003, 7004, 7005, 7006, 7008]),
    "bag": ((4, BAG) + RND, [5918, 5920, 5926, 7001, 7004, 7009], [7000, 7002, 7003, 7006, 7007, 7008]),
}
STOP_T = 700


def config_id(cfg):
    P, ext, first, pool = cfg
    return "p%dd%d-%s%s" % (P, displays(P, ext), "bag" if ext & oz.EXT_FINITE_BAG else ("lid" if pool == oz.POOL_LID else "rnd"),
                            "".join(t for f, t in ((oz.EXT_END_BONUS, "-endbonus"), (oz.EXT_SHORT_DEAL, "-short")) if ext & f))


def displays(P, ext):
    return 2 * P + 1 if ext & oz.EXT_DISPLAYS_2P1 else 5


def num_actions(P, ext):
    return (displays(P, ext) + 1) * 30


def device_rules(first, pool):
    return {"first_player": "Random" if first == oz.FIRST_RANDOM else first, "tile_pool": "Lid" if pool == oz.POOL_LID else "Random"}


def new_stream(seed, cfg):
    P, ext, first, pool = cfg
    s = oz.StreamX(seed, P, first_player=first, tile_pool=pool, ext=ext)
    s.marked = 0                    # slots a stopped game was marked for: the device counts them in `stuck`, the oracle has no such slots
    return s


def clone(s):
    c = object.__new__(oz.StreamX)
    c.g, c.r = oz.Game(), oz.Rng()
    C.memmove(C.byref(c.g), C.byref(s.g), C.sizeof(oz.Game))
    C.memmove(C.byref(c.r), C.byref(s.r), C.sizeof(oz.Rng))
    c.first, c.num_actions = s.first, s.num_actions
    c.stuck, c.episodes = C.c_uint64(s.stuck.value), C.c_uint64(s.episodes.value)
    c.stats_sum = s.stats_sum.copy()
    c.marked = getattr(s, "marked", 0)
    return c


def rebase(s):
    """azul_batch_reset_counters on the oracle's side."""
    s.stuck.value = s.episodes.value = 0
    s.stats_sum[:] = 0
    s.marked = 0


def record_bytes(s):
    return np.frombuffer(s.record().tobytes(), np.uint8).copy()


def moves_until_stop(s, T):
    """How many of the next T moves the oracle completes (T: no rule error), played on a copy in ONE C call: the done flag of a move is
    written only once its step has succeeded."""
    c = clone(s)
    done = np.full(T, 0xFF, np.uint8)
    rc = oz.lib().oz_stream_x_advance(C.byref(c.g), C.byref(c.r), c.first, T, None, None, done.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None, None)
    if rc == 0:
        return T
    assert rc == oz.BOX_EMPTY, rc
    return int(np.argmax(done == 0xFF))


def packed_words(action, done):
    """The compact record of a wide batch (csrc/azul_rules_x.hpp outputs_x): action | done << 8 for actions below 255, else
    0xff | done << 8 | action << 16 with 0xffff for "none" (the reward half is free: a wide stream's reward is all zero)."""
    a, d = action.astype(np.int64), done.astype(np.int64)
    small = (a >= 0) & (a < 255)
    return np.where(small, a | (d << 8), 0xFF | (d << 8) | (np.where(a >= 0, a, 0xFFFF) << 16)).astype(np.uint32)


class Expect:
    """T slots of one game: mask [T][NA], action, done, rec [T][256], ok (T: not stopped), final [256], mt, pos, episodes, stuck, stat_sums."""


def play_oracle(s, T, may_stop=True):
    """Advance `s` by T slots (in place) and return what the device must have written for them."""
    NA = s.num_actions
    ok = moves_until_stop(s, T) if may_stop else T
    e = Expect()
    e.T, e.ok = T, ok
    e.mask = np.zeros((T, NA), np.uint8)
    e.action = np.full(T, -1, np.int32)
    e.done = np.full(T, 2, np.uint8)
    e.rec = np.zeros((T, 256), np.uint8)
    if ok:
        o = s.advance(ok)
        e.mask[:ok], e.action[:ok], e.done[:ok] = o["mask"], o["action"], o["done"]
        e.rec[:ok] = o["rec_after"].view(np.uint8).reshape(ok, 256)
        # a slot that plays no move reports an EMPTY row: a stuck game has no legal move anyway, and a finished game handed in takes none
        # (oz_check_all_valid_x does not look at the ended flag; the stream plays -1 there all the same)
        e.mask[:ok][o["done"] == 2] = 0
    if ok < T:
        stop_mask = oz.check_all_valid_x(s.g).astype(np.uint8)
        r2 = oz.Rng()
        C.memmove(C.byref(r2), C.byref(s.r), C.sizeof(oz.Rng))
        stop_action = oz.lib().oz_random_agent_x(stop_mask.ctypes.data_as(C.POINTER(C.c_uint8)), NA, C.byref(r2))
        assert stop_action >= 0
        try:
            s.advance(1)
        except RuntimeError:
            pass
        else:
            raise AssertionError("the oracle was expected to stop here")
        e.mask[ok], e.action[ok], e.done[ok] = stop_mask, stop_action, 0
        e.rec[ok:] = record_bytes(s)
        s.marked += T - ok - 1
    e.final = record_bytes(s)
    e.mt, e.pos = s.rng_state()
    e.episodes, e.stuck, e.stat_sums = int(s.episodes.value), int(s.stuck.value) + s.marked, s.stats_sum.copy()
    return e


def shifted_stop(e, d):
    """NEGATIVE CONTROL for the comparison: the same expectation with the stop believed one slot later (d = 1) or earlier (d = -1)."""
    assert e.ok < e.T and d in (1, -1) and 0 < e.ok + d < e.T - 1
    c = copy.deepcopy(e)
    if d > 0:
        c.mask[e.ok + 1], c.action[e.ok + 1], c.done[e.ok + 1] = e.mask[e.ok], e.action[e.ok], 0
    else:
        c.mask[e.ok], c.action[e.ok], c.done[e.ok] = 0, -1, 2
    c.ok, c.stuck = e.ok + d, e.stuck - d
    return c


def compare(e, got, g, tag=()):
    """Everything the launch(es) wrote for game `g` of a batch against the expectation.  `got`: time-major arrays [T][n]... under "mask"
    (rows of any pitch), "action", "reward", "done", "packed", "maskbits", "rec" -- each optional -- and per game "final" [n][256] bytes, "mt"
    [n][624], "pos", "episodes", "stuck", "stat_sums" [n][10]."""
    T, NA = e.mask.shape
    tag = tuple(tag) + (g,)

    def same(name, want, have):
        want, have = np.atleast_1d(want), np.atleast_1d(have)
        assert want.shape == have.shape, (name, want.shape, have.shape) + tag
        if not np.array_equal(want, have):
            raise AssertionError((name, "first difference at", tuple(int(i[0]) for i in np.nonzero(want != have)), "stop", e.ok) + tag)

    have = lambda k: got.get(k) is not None
    if have("mask"):
        same("mask", e.mask, got["mask"][:, g, :NA])
    if have("action"):
        same("action", e.action, got["action"][:, g])
    if have("done"):
        same("done", e.done, got["done"][:, g])
    if have("reward"):
        same("reward", np.zeros(T, np.int32), got["reward"][:, g])          # GameRunner's shaped reward is two-player (game_runner.py:50)
    if have("packed"):
        same("packed", packed_words(e.action, e.done), np.ascontiguousarray(got["packed"][:, g]).view(np.uint32))
    if have("maskbits"):
        bits = np.ascontiguousarray(got["maskbits"][:, g]).view(np.uint8).reshape(T, -1)
        nb = (NA + 7) // 8
        same("maskbits", np.packbits(e.mask.astype(bool), axis=1, bitorder="little"), bits[:, :nb])
        same("maskbits tail", np.zeros_like(bits[:, nb:]), bits[:, nb:])
    if have("rec"):
        same("rec", e.rec, np.ascontiguousarray(got["rec"][:, g]).view(np.uint8).reshape(T, 256))
    same("final", e.final, np.frombuffer(np.ascontiguousarray(got["final"][g]).tobytes(), np.uint8))
    same("mt", e.mt, got["mt"][g])
    same("pos", e.pos, int(got["pos"][g]))
    same("episodes", e.episodes, int(got["episodes"][g]))
    same("stuck", e.stuck, int(got["stuck"][g]))
    assert np.allclose(got["stat_sums"][g], e.stat_sums, rtol=0, atol=1e-9), ("stat_sums",) + tag


def must_differ(e, got, g):
    """The comparison side of a negative control: `e` is a perturbed expectation, so `compare` has to object."""
    try:
        compare(e, got, g)
    except AssertionError:
        return
    raise AssertionError("a perturbed expectation passed the comparison: the comparison is blind (game %d)" % g)


def expectation_as_batch(es):
    """Expectations of n games laid out like a launch's outputs: the oracle-only form of `got` (tests/test_wide_stream_cases.py feeds it to
    `compare` to show what a perturbed expectation is caught by)."""
    T = es[0].T
    return {"mask": np.stack([e.mask for e in es], 1), "action": np.stack([e.action for e in es], 1), "done": np.stack([e.done for e in es], 1),
            "reward": np.zeros((T, len(es)), np.int32), "packed": np.stack([packed_words(e.action, e.done) for e in es], 1),
            "rec": np.stack([e.rec for e in es], 1), "final": np.stack([e.final for e in es]), "mt": np.stack([e.mt for e in es]),
            "pos": np.array([e.pos for e in es]), "episodes": np.array([e.episodes for e in es]), "stuck": np.array([e.stuck for e in es]),
            "stat_sums": np.stack([e.stat_sums for e in es])}


# ---- case 1: the regeneration sweep ---------------------------------------------------------------------------------------------------------
# A fresh game cannot end within 60 moves (five rounds at least), so the sweep plays long enough for restarts to meet a regeneration:
# 360 moves (600 on nine displays, whose games last longer and, without the short deal, often stop before they end).
SWEEP_N, SWEEP_SPAN, SWEEP_MIN = 96, 150, 8


def sweep_steps(cfg):
    return 600 if displays(cfg[0], cfg[1]) == 9 else 360



def sweep_start(g, n=SWEEP_N):
    """CPython's index when game g starts: 624 and 623 (a plain move's two words across the regeneration), then the last SWEEP_SPAN words."""
    return 624 - g if g < 2 else 622 - ((g - 2) * (SWEEP_SPAN - 2)) // (n - 3)


def sweep_streams(cfg, seed0, shift=0):
    streams = [new_stream(seed0 + g, cfg) for g in range(SWEEP_N)]
    for g, s in enumerate(streams):
        s.r.idx = sweep_start(g) - shift
    return streams


def classify_wraps(s, T):
    """Which kinds of step of the next T (played on a copy) have the regeneration of the 624-word state INSIDE the words they consume:
    "move" -- between or before a move's two words (index 623 / 624 when it is fetched); "deal" -- inside the words of the round dealt after
    a move; "reset" -- inside the words of the restart (first player + deal) after a game end or a stuck slot."""
    c, seen = clone(s), set()
    for _ in range(moves_until_stop(s, T)):             # (a game that a rule error stops is classified up to its stop)
        i0, w0 = int(c.r.idx), int(c.r.words)
        o = c.advance(1, want_records=False)
        used, dn = int(c.r.words) - w0, int(o["done"][0])
        head = 0 if dn == 2 else 2                     # a stuck slot draws no move
        if head and i0 + head > 624:
            seen.add("move")
        elif used > head and i0 + used > 624:
            seen.add("reset" if dn else "deal")
    return seen


def sweep_census(streams, T):
    census = {"move": 0, "deal": 0, "reset": 0}
    for s in streams:
        for k in classify_wraps(s, T):
            census[k] += 1
    return census


# ---- case 4: games handed in mid-play, finished and stuck slots --------------------------------------------------------------------------------
HAND_IN_N, HAND_IN_T = 40, 400
HAND_IN_ENDED = (4, 11)       # half 0 of wave 2, half 1 of wave 5
HAND_IN_STUCK = (7, 16)       # half 1 of wave 3, half 0 of wave 8


def hand_in_streams(cfg, seed0):
    """Games the oracle has played g * 11 + 3 moves of; two of them with the ended flag set and two stuck (displays empty, only the
    first-player token in the centre), one of each in either half of a wave.  Counters start from zero (reset_counters)."""
    streams, seed = [], seed0
    while len(streams) < HAND_IN_N:                     # (seeds whose game a rule error stops before the hand-over are passed over)
        s, pre = new_stream(seed, cfg), len(streams) * 11 + 3
        seed += 1
        if moves_until_stop(s, pre) == pre:
            s.advance(pre, want_records=False)
            streams.append(s)
    for g, s in enumerate(streams):
        if g in HAND_IN_ENDED:
            s.g.end_of_game = 1
        if g in HAND_IN_STUCK:
            s.g.arr("displays")[:] = 0
            s.g.arr("xdisplays")[:] = 0
            s.g.arr("center")[:] = [0, 0, 0, 0, 0, 1]
        rebase(s)
    return streams


# ---- case 5: stopped games ---------------------------------------------------------------------------------------------------------------------
def stop_seeds(which):
    """An explicit seeds= array: stopped games (X) and live ones (.) laid out over waves as  X. | .X | XX | .. | X. ...  so that a stopped
    game sits in half 0 beside a live sibling, in half 1 beside a live sibling, and beside another stopped game."""
    cfg, stops, live = STOP_CONFIGS[which]
    n = len(stops) + len(live)
    slots = [0, 3, 4, 5] + [8, 11][:len(stops) - 4]
    rest = iter(live)
    seeds = np.array([stops[slots.index(i)] if i in slots else next(rest) for i in range(n)], dtype=np.uint64)
    return cfg, seeds, slots


def sibling_placements(stopped, n):
    """Which of the three placements a set of stopped slots covers."""
    st, seen = set(stopped), set()
    for g in st:
        sib = g ^ 1
        if sib >= n:
            continue
        seen.add("pair" if sib in st else ("half0" if g % 2 == 0 else "half1"))
    return seen
