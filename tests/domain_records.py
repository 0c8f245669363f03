"""TEST helper: arbitrary records INSIDE the documented record domain (players 0..P, floors 0..7, 25-bit walls, box and lid at
most 255 tiles each, cell counts at most 255 -- "incl. states no game reaches"), for the two-player and the wide record, with the oracle's
answer to every rule call the tests make on them, and a census of what the records exercise.  Plain numpy + the oracle: no project code.

Families (each generator call returns them in this order, `per` records each; FAMILIES names them):
  scatter      the distribution of tests/test_random_states.random_records, generalised to P players and D displays;
  dense        the same with about a third of the walls the OR of three random 25-bit draws: rows, columns and colours complete, games end;
  round_end    every display empty, the centre holds one colour, with and without the token: every legal move ends the round and -- unless
               the game ends -- deals; half of them on dense walls;
  pool_edge    box = lid = 0; box empty with a large lid; one or two tiles in total (the short deal); totals at the closure bound; on
               round-ending tables, so that the pools are actually looked at.
Closure bound: box + lid + displays + xdisplays + centre colours + pattern lines of the P players <= 255 in every record -- the tiles that can
still reach the bag: no refill (azul.py:81-83) can then find more than 255 tiles, whatever is played.  The exception is `overflow`: box = 0,
lid = [51] * 5 (the most the documented domain accepts) on a round-ending table whose full lines return tiles, so that the refill finds more
than 255.  `ended` is the other named generator outside the families: records at the ends of an episode (the ended flag set, an empty
table, a complete wall row with the flag clear) for the kernels that run whole windows (tests/window_domain_cases.py).

Every absent player's field and every unused xdisplays row is zero."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as oz

FAMILIES = ("scatter", "dense", "round_end", "pool_edge")
CLOSURE = 255
END_BONUS, SHORT_DEAL, DISPLAYS_2P1, FINITE_BAG = oz.EXT_END_BONUS, oz.EXT_SHORT_DEAL, oz.EXT_DISPLAYS_2P1, oz.EXT_FINITE_BAG
# (players, ext, tile_pool) of the wide rule book's instantiations under test: (3, 5), (4, 5), (2, 5), (3, 7), (4, 9) displays
WIDE_CONFIGS = [(3, 0, oz.POOL_LID), (4, 0, oz.POOL_RANDOM), (2, END_BONUS, oz.POOL_LID),
                (3, DISPLAYS_2P1 | END_BONUS | SHORT_DEAL, oz.POOL_LID), (4, DISPLAYS_2P1 | END_BONUS | SHORT_DEAL, oz.POOL_LID),
                (4, DISPLAYS_2P1 | END_BONUS | SHORT_DEAL | FINITE_BAG, oz.POOL_RANDOM), (3, SHORT_DEAL, oz.POOL_LID)]
TWO_CONFIGS = [(2, 0, oz.POOL_LID), (2, 0, oz.POOL_RANDOM)]             # the 128-byte record: both pools
CLASSES = ("deals", "ends_game", "box_empty", "short_deal", "mixed_row", "overfull_line", "floor_seven", "clamped", "bonus_paid")


def config_id(cfg):
    P, ext, pool = cfg
    return "p%dd%d-%s%s" % (P, displays(cfg), "bag" if ext & FINITE_BAG else ("lid" if pool == oz.POOL_LID else "rnd"),
                            "".join(t for f, t in ((END_BONUS, "-endbonus"), (SHORT_DEAL, "-short")) if ext & f))


def displays(cfg):
    return 2 * cfg[0] + 1 if cfg[1] & DISPLAYS_2P1 else 5


def tracks(cfg):
    return cfg[2] == oz.POOL_LID or bool(cfg[1] & FINITE_BAG)


def unreachable(cfg):
    """The census classes a config cannot reach: an untracked pool never runs dry; with the short deal no deal fails, without it none is
    short; with the end-of-game bonus switch count_score pays no line bonus (they are paid once, when the game has ended)."""
    P, ext, pool = cfg
    out = set()
    if not tracks(cfg):
        out |= {"box_empty", "short_deal"}
    elif ext & SHORT_DEAL:
        out.add("box_empty")
    else:
        out.add("short_deal")
    if ext & END_BONUS:
        out.add("bonus_paid")
    return out


# ---- the generators ----------------------------------------------------------------------------------------------------------------------------
def _lines(rs, n, P):
    lines = np.zeros((n, P, 5, 5), dtype=np.uint8)
    for g in range(n):
        for p in range(P):
            for r in range(5):
                mode = rs.rand()
                if mode < 0.25:
                    continue
                k = 1 if mode < 0.8 else rs.randint(2, 4)            # sometimes several colours on one row
                for c in rs.choice(5, size=k, replace=False):
                    lines[g, p, r, c] = rs.randint(1, r + 3) if rs.rand() < 0.2 else (r + 1 if rs.rand() < 0.5 else rs.randint(1, r + 2))
    return lines


def _scatter(rs, n, P, D, wide):
    rec = np.zeros(n, dtype=oz.RECORD_NP_DTYPE if wide else oz.RECORD_DTYPE)
    rec["displays"] = rs.randint(0, 5, size=(n, 5, 5)) * (rs.rand(n, 5, 5) < 0.4)
    if D > 5:
        rec["xdisplays"][:, :D - 5] = rs.randint(0, 5, size=(n, D - 5, 5)) * (rs.rand(n, D - 5, 5) < 0.4)
    rec["center"][:, :5] = rs.randint(0, 8, size=(n, 5)) * (rs.rand(n, 5) < 0.5)
    rec["center"][:, 5] = rs.rand(n) < 0.5
    rec["flags"] = rs.randint(1, P + 1, size=n) | (rs.randint(0, P + 1, size=n) << 3)
    rec["pattern_lines"][:, :P] = _lines(rs, n, P)
    rec["floors"][:, :P] = rs.randint(0, 8, size=(n, P))
    rec["walls"][:, :P] = rs.randint(0, 1 << 25, size=(n, P)) & rs.randint(0, 1 << 25, size=(n, P))
    rec["score"][:, :P] = rs.randint(0, 120, size=(n, P))
    rec["box"] = rs.randint(0, 21, size=(n, 5))
    rec["lid"] = rs.randint(0, 12, size=(n, 5))
    rec["turn_counter"] = rs.randint(1, 9, size=n)
    rec["first_player_stats"][:, :P] = rs.randint(0, 5, size=(n, P))
    rec["floor_penalty"][:, :P] = -rs.randint(0, 30, size=(n, P))
    rec["max_combo"][:, :P] = rs.randint(0, 8, size=(n, P))
    rec["completed_lines"][:, :P] = rs.randint(0, 3, size=(n, P, 3))
    if wide:
        rec["players"] = P
        rec["n_displays"] = 0 if D == 5 else D
    else:
        rec["player_score"] = rs.randint(-20, 20, size=n)
        rec["move_counter"] = rs.randint(0, 60, size=n)
    return rec


def _densify(rs, rec, P, share=1 / 3):
    n = len(rec)
    dense = rs.randint(0, 1 << 25, size=(n, P)) | rs.randint(0, 1 << 25, size=(n, P)) | rs.randint(0, 1 << 25, size=(n, P))
    pick = rs.rand(n, P) < share
    rec["walls"][:, :P] = np.where(pick, dense, rec["walls"][:, :P])


def _round_ending_table(rs, rec, P):
    """Displays empty, one colour in the centre, the token there in every second record."""
    n = len(rec)
    rec["displays"] = 0
    if "xdisplays" in rec.dtype.names:
        rec["xdisplays"] = 0
    rec["center"] = 0
    rec["center"][np.arange(n), rs.randint(0, 5, size=n)] = rs.randint(1, 8, size=n)
    rec["center"][:, 5] = np.arange(n) % 2
    poor = np.flatnonzero(np.arange(n) % 3 == 2)                       # every third: few points and a long floor line, so the clamp acts
    rec["score"][poor, :P] = rs.randint(0, 4, size=(len(poor), P))
    rec["floors"][poor, :P] = rs.randint(3, 8, size=(len(poor), P))


def tiles_in_play(rec, P):
    """Per record: the tiles that can still reach the bag (the closure bound's left-hand side)."""
    r = np.atleast_1d(rec)
    n = len(r)
    t = r["box"].reshape(n, -1).sum(1, dtype=np.int64) + r["lid"].reshape(n, -1).sum(1, dtype=np.int64)
    t += r["displays"].reshape(n, -1).sum(1, dtype=np.int64) + r["center"][:, :5].sum(1, dtype=np.int64)
    t += r["pattern_lines"][:, :P].reshape(n, -1).sum(1, dtype=np.int64)
    if "xdisplays" in r.dtype.names:
        t += r["xdisplays"].reshape(n, -1).sum(1, dtype=np.int64)
    return t


def _fit(rec, P):
    """Take tiles out of the box, then the lid, until a record meets the closure bound."""
    for i in np.flatnonzero(tiles_in_play(rec, P) > CLOSURE):
        over = int(tiles_in_play(rec[i:i + 1], P)[0]) - CLOSURE
        for name in ("box", "lid"):
            for c in range(5):
                take = min(over, int(rec[name][i, c]))
                rec[name][i, c] -= take
                over -= take
        assert over == 0
    return rec


def _split(rs, total):
    cuts = np.sort(rs.randint(0, total + 1, size=4))
    return np.diff(np.concatenate([[0], cuts, [total]]))


def _pool_edges(rs, rec, P):
    """Six kinds in turn: nothing anywhere; box empty and a large lid; one tile; two tiles; the closure bound exactly, all of it in the box;
    the closure bound exactly, the box empty."""
    _round_ending_table(rs, rec[: len(rec) * 3 // 4], P)                  # (the last quarter keeps its scattered table)
    for i in range(len(rec)):
        room = CLOSURE - (int(tiles_in_play(rec[i:i + 1], P)[0]) - int(rec["box"][i].sum()) - int(rec["lid"][i].sum()))
        kind = i % 6
        rec["box"][i] = rec["lid"][i] = 0
        if kind in (0, 2, 3):                                          # few full lines: scoring returns three tiles at the most
            rec["pattern_lines"][i, 1:] = 0
            rec["pattern_lines"][i, 0, 3:] = 0
        if kind == 1:
            rec["lid"][i] = _split(rs, rs.randint(room // 2, room + 1))
        elif kind in (2, 3):
            rec["box" if rs.rand() < 0.5 else "lid"][i, rs.randint(5)] = kind - 1
        elif kind == 4:
            rec["box"][i] = _split(rs, room)
        elif kind == 5:
            rec["lid"][i] = _split(rs, room)


def _families(rs, per, P, D, wide):
    out = []
    for fam in FAMILIES:
        rec = _scatter(rs, per, P, D, wide)
        if fam == "dense":
            _densify(rs, rec, P)
        elif fam == "round_end":
            _densify(rs, rec[: per // 2], P)
            _round_ending_table(rs, rec, P)
        elif fam == "pool_edge":
            _pool_edges(rs, rec, P)
        out.append(_fit(rec, P))
    return np.concatenate(out)


def two_player(n, seed):
    """n records (a multiple of four: n / 4 of every family) of the 128-byte record."""
    assert n % 4 == 0
    return _families(np.random.RandomState(seed), n // 4, 2, 5, False)


def wide(n, P, D, seed):
    """n records (a multiple of four: n / 4 of every family) of the 256-byte record of a P-player batch on D displays."""
    assert n % 4 == 0
    return _families(np.random.RandomState(seed), n // 4, P, D, True)


def family_of(i, n):
    return FAMILIES[i // (n // 4)]


def overflow(n, P, D, seed, wide_record=True):
    """The named records OUTSIDE the closure bound: box = 0, lid = [51] * 5 (255 tiles: the documented domain's limit), a round-ending table
    and, for every player, a full line in row 4 -- count_score returns 4 tiles per player to the lid, the refill finds 255 + 4 P."""
    rs = np.random.RandomState(seed)
    rec = _scatter(rs, n, P, D, wide_record)
    _round_ending_table(rs, rec, P)
    rec["walls"][:, :P] &= rs.randint(0, 1 << 25, size=(n, P)).astype(np.uint32)         # sparse walls: the game goes on
    rec["pattern_lines"][:, :P, 4, :] = 0
    rec["pattern_lines"][np.arange(n)[:, None], np.arange(P)[None, :], 4, rs.randint(0, 5, size=(n, P))] = 5
    rec["box"] = 0
    rec["lid"] = 51
    return rec


def ended(n, P, D, seed, wide_record=True):
    """The named records at the ends of an episode (NOT a family: batch() and the existing tests' records stay what they are), scattered
    records in thirds: the record's ended flag (bit 6 of `flags`) set -- Azul.step answers GameEnded whatever is on the table; an empty
    table without the token -- nothing is legal, the round is over and nobody can end it; a complete wall row with the flag still clear --
    is_end_of_game() reads the walls (azul.py:184-191), step's GameEnded the flag (:298-299): any legal move ends the episode."""
    rs = np.random.RandomState(seed)
    rec = _scatter(rs, n, P, D, wide_record)
    for i in range(n):
        kind = i * 3 // n
        if kind == 0:
            rec["flags"][i] |= 1 << 6
        elif kind == 1:
            rec["displays"][i] = 0
            rec["center"][i] = 0
            if wide_record:
                rec["xdisplays"][i] = 0
        else:
            rec["walls"][i, rs.randint(P)] |= np.uint32(0x1f << (5 * rs.randint(5)))
    return _fit(rec, P)


# ---- the oracle's side ---------------------------------------------------------------------------------------------------------------------------
class LeftOut(Exception):
    """An oracle post-state that the record cannot hold: the GENERATOR is to change, not the test."""


class Game:
    """One record in the oracle: the 128-byte record's runner or the wide record's game, behind one interface."""

    def __init__(self, rec, cfg):
        P, ext, pool = cfg
        self.cfg, self.wide = cfg, np.asarray(rec).dtype == oz.RECORD_NP_DTYPE
        if self.wide:
            self.q, self.g = None, oz.unpack_np(rec, pool, ext)
        else:
            self.q = oz.unpack(rec, pool, oz.FIRST_RANDOM)
            self.g = self.q.game
            self.g.ext = ext

    def pack(self):
        try:
            return oz.pack_np(self.g) if self.wide else oz.pack(self.q)
        except ValueError as e:
            raise LeftOut(str(e))

    def mask(self):
        return oz.check_all_valid_x(self.g) if self.wide else oz.check_all_valid(self.g)

    def obs(self, p):
        return oz.get_state_x(self.g, p) if self.wide else oz.get_state(self.g, p)

    def mover(self):
        p = self.g.current_player - 1
        return p if p >= 0 else self.g.players - 1

    def flags(self):
        L = oz.lib()
        return (1 if L.oz_is_end_of_round(C.byref(self.g)) else 0) | (2 if L.oz_is_end_of_game(C.byref(self.g)) else 0)

    def split(self, a):
        d, c, p = C.c_int(), C.c_int(), C.c_int()
        oz.lib().oz_deserialize_x(C.byref(self.g), int(a), C.byref(d), C.byref(c), C.byref(p))
        return d.value, c.value, p.value

    def move(self, a):
        oz.lib().oz_move(C.byref(self.g), *self.split(a))

    def step(self, a, rng):
        return oz.lib().oz_step(C.byref(self.g), *self.split(a), C.byref(rng))

    def new_round(self, rng):
        return oz.lib().oz_new_round(C.byref(self.g), C.byref(rng))

    def count_score(self):
        oz.lib().oz_count_score(C.byref(self.g))

    def next_player(self):
        oz.lib().oz_next_player(C.byref(self.g))

    def stats(self):
        return np.array([oz.get_statistics(self.g)[k] for k in oz.STAT_KEYS])


def picks(mask):
    """The legal actions the tests play on a record: the first, the middle and the last one (fewer when fewer are legal)."""
    legal = np.flatnonzero(mask)
    return sorted({int(legal[0]), int(legal[len(legal) // 2]), int(legal[-1])}) if len(legal) else []


def stream_of(seed, i):
    """Record i's MT19937 state: random.seed(seed + i), the index anywhere in 0..624 -- every sixth record within the last 30 words, so that
    a deal's words straddle the regeneration."""
    r = oz.seeded_rng(seed + i)
    oz.lib().oz_rng_u32(C.byref(r))                      # (the first word generates the state)
    rs = np.random.RandomState(seed + i)
    r.idx = int(rs.randint(595, 625)) if i % 6 == 0 else int(rs.randint(0, 625))
    return r


def _clone_rng(r):
    c = oz.Rng()
    C.memmove(C.byref(c), C.byref(r), C.sizeof(oz.Rng))
    return c


def rng_words(r):
    return np.ctypeslib.as_array(r.mt).copy(), int(r.idx)


class Answer:
    """The oracle's answers for one record: mask, flags, obs[seat], obs_mover, mover, scored (record after count_score), moved {a: record},
    phi (the potential: seat 0 against the best other seat after count_score on a copy), stepped {a: (status, record, words, index)}, dealt
    (status, record, words, index), passed (record after next_player), action (oz_random_agent_x on the record's own mask, words, index),
    sample_mask / sampled (a foreign mask; the pick on it, words, index), stats, mt / pos (the stream every drawing call starts from)."""


def answer(rec, cfg, rng):
    P = cfg[0]
    a = Answer()
    g = Game(rec, cfg)
    if g.pack().tobytes() != np.asarray(rec).tobytes():
        raise LeftOut("the record does not round-trip")
    a.mt, a.pos = rng_words(rng)
    a.mask, a.flags, a.mover = g.mask(), g.flags(), g.mover()
    a.obs = [g.obs(p) for p in range(P)]
    a.obs_mover = g.obs(a.mover)
    a.stats = g.stats()
    a.picks = picks(a.mask)
    h = Game(rec, cfg)
    h.count_score()
    a.scored = h.pack()
    sc = [int(x) for x in a.scored["score"][:P]]
    a.phi = sc[0] - max(sc[1:])                          # game_runner.py:48-50 (P > 2, beyond the reference: seat 0 against the best other seat)
    a.moved, a.stepped = {}, {}
    for act in a.picks:
        h = Game(rec, cfg)
        h.move(act)
        a.moved[act] = h.pack()
        h, r = Game(rec, cfg), _clone_rng(rng)
        st = h.step(act, r)
        a.stepped[act] = (st, h.pack()) + rng_words(r)
    h, r = Game(rec, cfg), _clone_rng(rng)
    st = h.new_round(r)
    a.dealt = (st, h.pack()) + rng_words(r)
    h = Game(rec, cfg)
    h.next_player()
    a.passed = h.pack()
    NA = len(a.mask)
    m8 = a.mask.astype(np.uint8)
    r = _clone_rng(rng)
    a.action = (int(oz.lib().oz_random_agent_x(m8.ctypes.data_as(C.POINTER(C.c_uint8)), NA, C.byref(r))),) + rng_words(r)
    rs = np.random.RandomState(int(a.mt[5]) & 0x7fffffff)
    a.sample_mask = (rs.rand(NA) < rs.choice([0.03, 0.3, 0.9])).astype(np.uint8)
    r = _clone_rng(rng)
    a.sampled = (int(oz.lib().oz_random_agent_x(a.sample_mask.ctypes.data_as(C.POINTER(C.c_uint8)), NA, C.byref(r))),) + rng_words(r)
    return a


def answers(recs, cfg, seed):
    return [answer(r, cfg, stream_of(seed, i)) for i, r in enumerate(recs)]


CPU_N, GPU_N = 160, 256          # records per config: 40 of each family under the emulation, one batch of 256 on the GPU


@functools.lru_cache(maxsize=None)
def batch(cfg, n):
    """(records, answers) of one config, computed once per session and shared by every test that needs them: leave them unchanged."""
    P, ext, pool = cfg
    seed = 4000 + 100 * (WIDE_CONFIGS + TWO_CONFIGS).index(cfg) + n
    recs = two_player(n, seed) if cfg in TWO_CONFIGS else wide(n, P, displays(cfg), seed)
    return recs, answers(recs, cfg, 10 * seed)


def census(recs, cfg, seed=0, ans=None):
    """{class: number of records that show it} on the oracle alone, over the calls the tests make (count_score on the record, move and step on
    `picks`), and "left_out": oracle post-states that do not pack (must be 0)."""
    P, ext, pool = cfg
    D = displays(cfg)
    n = dict.fromkeys(CLASSES, 0)
    n["left_out"] = 0
    for i, rec in enumerate(recs):
        try:
            a = ans[i] if ans is not None else answer(rec, cfg, stream_of(seed, i))
        except LeftOut:
            n["left_out"] += 1
            continue
        lines = rec["pattern_lines"][:P].astype(np.int64)
        n["mixed_row"] += int(((lines != 0).sum(axis=2) >= 2).any())
        n["overfull_line"] += int((lines > np.arange(1, 6)[None, :, None]).any())
        stepped = list(a.stepped.values())
        dealt = [s for s in stepped if s[0] == oz.OK and (s[3] != a.pos or not np.array_equal(s[2], a.mt))]
        n["deals"] += int(bool(dealt))
        n["ends_game"] += int(any(s[0] == oz.OK and (int(s[1]["flags"]) >> 6) & 1 for s in stepped))
        n["box_empty"] += int(any(s[0] == oz.BOX_EMPTY for s in stepped))
        if ext & SHORT_DEAL and tracks(cfg):
            tiles = lambda r: int(r["displays"].sum()) + (int(r["xdisplays"].sum()) if "xdisplays" in r.dtype.names else 0)
            ended = lambda s: (int(s[1]["flags"]) >> 6) & 1
            n["short_deal"] += int(any(s[0] == oz.OK and not ended(s) and int(s[1]["center"][5]) == 1 and tiles(s[1]) < 4 * D
                                       and int(s[1]["turn_counter"]) == int(rec["turn_counter"]) + 1 for s in stepped))
        mover = a.mover
        n["floor_seven"] += int(int(rec["floors"][mover]) < 7 and any(int(m["floors"][mover]) == 7 for m in a.moved.values()))
        # the clamp (azul.py:294-295): the same scoring from 1000 points higher ends elsewhere than 1000 above
        hi = np.array(rec).copy()
        hi["score"][:P] += 1000
        g = Game(hi, cfg)
        g.count_score()
        n["clamped"] += int(any(int(a.scored["score"][p]) == 0 and int(g.g.score[p]) - 1000 < 0 for p in range(P)))
        # a line bonus paid by count_score: with the bonuses switched off (OZ_EXT_END_BONUS) the same scoring gives less
        if not ext & END_BONUS:
            g = Game(rec, (P, ext | END_BONUS, pool))
            g.count_score()
            n["bonus_paid"] += int(any(int(a.scored["score"][p]) > max(int(g.g.score[p]), 0) for p in range(P)))
    return n
