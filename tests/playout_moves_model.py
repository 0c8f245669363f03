"""TEST helper: the host model of azul_batch_playout_moves on the oracle -- the playout of include/azul_hip.h step by step (a byte copy of
the game, oz_move of the candidate, then oz_is_end_of_round / oz_next_player / check_all_valid / one move of the playout policy decided by
a word of the host Philox4x32-10 of tests/policy_draw_ref.py, until the round ends, then oz_count_score), the table of sums and the choice
from it, a classifier of the playout classes the tests require, and the states the tests share: tests/score_moves_model.stream_states(),
state i of which is global game GBASE + i wherever a test puts it in a batch.

The value of a playout is kept as score[0] - score[1]: the table is computed once per state and negated for the other perspective."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as oz
from tests import policy_draw_ref as pr
from tests import score_moves_model as sm

ILLEGAL = sm.ILLEGAL
PERSP_CURRENT = sm.PERSP_CURRENT
MAX_PLIES = 64
GBASE = 5000                   # global id of shared state 0
SEED, CALL = 0x1234567887654321, 7
KMAX = 3                       # playouts per candidate the shared values hold (the tests use K = 1, 2, 3)
PLAYOUT_CLASSES = ("candidate_ends_round", "plies_8_or_more", "forced_floor", "token_in_playout", "ends_game", "stuck")
STATE_CLASSES = ("best_differs_from_greedy", "tie", "none_legal")
_PLY_BLOCK = 24                # plies whose words are drawn at once; longer playouts draw the next block


def _words(seed, call, G, k_count, ply0):
    """uint64 [180][_PLY_BLOCK][k_count]: word 0 of the block at counter (a | ply << 16, k, G, call), key (seed lo, seed hi)."""
    a = np.arange(180, dtype=np.uint64)[:, None, None]
    ply = np.arange(ply0, ply0 + _PLY_BLOCK, dtype=np.uint64)[None, :, None]
    k = np.arange(k_count, dtype=np.uint64)[None, None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return pr.philox4x32_10((a | (ply << np.uint64(16)), k, int(G) & 0xFFFFFFFF, int(call) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))[0]


class _Draws:
    def __init__(self, seed, call, G, k_count):
        self.args, self.blocks = (seed, call, G, k_count), {}

    def word(self, a, ply, k):
        b = ply // _PLY_BLOCK
        if b not in self.blocks:
            self.blocks[b] = _words(*self.args, b * _PLY_BLOCK)
        return int(self.blocks[b][a, ply - b * _PLY_BLOCK, k])


def playout(game, a, k, draws):
    """One playout of candidate `a` (legal in `game`) -> (score[0] - score[1], facts): the definition, statement by statement."""
    L = oz.lib()
    g, _ = sm._moved(game, a)                                            # 1.
    ply = 0
    facts = dict.fromkeys(PLAYOUT_CLASSES, False)
    while True:                                                          # 2.
        if L.oz_is_end_of_round(C.byref(g)):                             # 2.1
            break
        L.oz_next_player(C.byref(g))                                     # 2.2
        legal = np.flatnonzero(oz.check_all_valid(g))                    # 2.3
        if len(legal) == 0:
            facts["stuck"] = True
            break
        if ply == MAX_PLIES:                                             # 2.4
            break
        J = int((legal < 30).sum())                                      # 2.5
        M = len(legal) - J
        n, base = (M, J) if M > 0 else (J, 0)
        facts["forced_floor"] |= M == 0
        w = draws.word(a, ply, k)                                        # 2.6
        move = int(legal[base + ((w * n) >> 32)])                        # 2.7
        d, c, p = C.c_int(), C.c_int(), C.c_int()
        L.oz_deserialize(move, C.byref(d), C.byref(c), C.byref(p))
        facts["token_in_playout"] |= d.value == 0 and g.center[5] == 1
        L.oz_move(C.byref(g), d.value, c.value, p.value)
        ply += 1
    L.oz_count_score(C.byref(g))                                         # 3.
    facts["candidate_ends_round"] = ply == 0 and not facts["stuck"]
    facts["plies_8_or_more"] = ply >= 8
    facts["ends_game"] = bool(L.oz_is_end_of_game(C.byref(g)))
    facts["plies"] = ply
    return int(g.score[0]) - int(g.score[1]), facts


def state_values(rec, G, seed=SEED, call=CALL, k_count=KMAX, pool=oz.POOL_LID):
    """(values int64 [180][k_count] of score[0] - score[1] per playout, legal bool [180], facts: a list of (k, playout's facts))."""
    game = sm._game(rec, pool)
    legal = oz.check_all_valid(game)
    vals = np.zeros((180, k_count), np.int64)
    facts = []
    draws = _Draws(seed, call, G, k_count)
    for a in np.flatnonzero(legal):
        for k in range(k_count):
            vals[a, k], f = playout(game, int(a), k, draws)
            facts.append((k, f))
    return vals, legal, facts


def table_of(vals, legal, K, mover, perspective=PERSP_CURRENT):
    """int64 [180]: the sum of the first K playouts from `perspective` (0, 1, or PERSP_CURRENT: `mover`, 0 / 1), ILLEGAL where not legal."""
    p = mover if perspective == PERSP_CURRENT else int(perspective)
    s = vals[:, :K].sum(axis=1)
    return np.where(legal, s if p == 0 else -s, ILLEGAL)


def best_of(tab):
    """The first legal action with the maximal sum; -1 when nothing is legal."""
    return sm.greedy(tab)


def mover_of(rec):
    return (int(np.asarray(rec).view(np.uint8).reshape(-1)[31]) & 7) - 1


def table(rec, G, K, perspective=PERSP_CURRENT, seed=SEED, call=CALL, pool=oz.POOL_LID):
    """(table int64 [180], best) of one record as global game G."""
    vals, legal, _ = state_values(rec, G, seed, call, K, pool)
    tab = table_of(vals, legal, K, mover_of(rec), perspective)
    return tab, best_of(tab)


def action_of_game(game, G, K, seed, call):
    """The playout player's answer for an oracle game (mover's perspective): what the rollout's replay hands to GameRunner."""
    legal = oz.check_all_valid(game)
    if not legal.any():
        return -1
    draws = _Draws(seed, call, G, K)
    s = np.zeros(180, np.int64)
    for a in np.flatnonzero(legal):
        s[a] = sum(playout(game, int(a), k, draws)[0] for k in range(K))
    tab = np.where(legal, s if game.current_player == 1 else -s, ILLEGAL)
    return best_of(tab)


@functools.lru_cache(maxsize=None)
def stream_values():
    """The shared values, computed once: (values int64 [360][180][KMAX], legal bool [360][180], movers int [360], facts [360]: per state
    the list of (k, playout's facts)) of sm.stream_states() with state i as global game GBASE + i at (SEED, CALL)."""
    recs = sm.stream_states()[0]
    vals, legal, facts = [], [], []
    for i, r in enumerate(recs):
        v, lg, f = state_values(r, GBASE + i)
        vals.append(v)
        legal.append(lg)
        facts.append(f)
    return np.stack(vals), np.stack(legal), np.array([mover_of(r) for r in recs]), facts


@functools.lru_cache(maxsize=None)
def stream_tables(K, perspective=PERSP_CURRENT):
    """(tables int64 [360][180], best int32 [360]) of the shared states for K <= KMAX playouts."""
    vals, legal, movers, _ = stream_values()
    tabs = np.stack([table_of(vals[i], legal[i], K, int(movers[i]), perspective) for i in range(len(vals))])
    return tabs, np.array([best_of(t) for t in tabs], np.int32)


def classify_states(indices, K=2):
    """{class: count} over the shared states `indices` at K playouts per candidate: the playout classes count playouts, the state classes
    states; "playouts" and "longest" ride along."""
    assert K <= KMAX
    greedy = sm.stream_tables(PERSP_CURRENT)[1]
    tabs, best = stream_tables(K)
    _, legal_all, _, facts = stream_values()
    total = dict.fromkeys(PLAYOUT_CLASSES + STATE_CLASSES + ("playouts", "longest"), 0)
    for i in indices:
        for k, f in facts[i]:
            if k < K:
                for name in PLAYOUT_CLASSES:
                    total[name] += int(f[name])
                total["playouts"] += 1
                total["longest"] = max(total["longest"], f["plies"])
        lg = np.flatnonzero(legal_all[i])
        total["none_legal"] += int(len(lg) == 0)
        total["best_differs_from_greedy"] += int(len(lg) > 0 and best[i] != greedy[i])
        total["tie"] += int(len(lg) >= 2 and int((tabs[i][lg] == tabs[i][lg].max()).sum()) >= 2)
    return total


# ---- arbitrary in-domain records (tests/domain_records.py) ------------------------------------------------------------------------------------
DOMAIN_GBASE = 70000           # global id of domain record 0 of a config
DOMAIN_ENDED = 9               # `ended` records behind the emulation's 160; the GPU batch: 254 of the 256 + 3 `ended` = 257
DOMAIN_CLASSES = ("candidate_ends_round", "plies_8_or_more", "forced_floor", "token_in_playout", "ends_game", "none_legal", "tie")


@functools.lru_cache(maxsize=None)
def domain_values(cfg, n):
    """(records uint8 [N][128], values int64 [N][180][KMAX], legal bool [N][180], movers int [N], facts [N]) of a two-player config's domain
    records, computed once: n = dr.CPU_N -> the 160 records of dr.batch(cfg, n) and DOMAIN_ENDED of dr.ended; n = dr.GPU_N -> the first 254
    of dr.batch(cfg, n) and 3 of dr.ended (257: the last wave holds one game).  Record i is global game DOMAIN_GBASE + i at (SEED, CALL)."""
    from tests import domain_records as dr
    pool = cfg[2]
    recs, n_ended = dr.batch(cfg, n)[0], (DOMAIN_ENDED if n == dr.CPU_N else 3)
    recs = np.concatenate([recs if n == dr.CPU_N else recs[:n - 2], dr.ended(n_ended, 2, 5, 8800 + pool, False)])
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).copy()
    vals, legal, facts = zip(*[state_values(r, DOMAIN_GBASE + i, pool=pool) for i, r in enumerate(raw)])
    return raw, np.stack(vals), np.stack(legal), np.array([mover_of(r) for r in raw]), list(facts)


def domain_tables(cfg, n, K, perspective=PERSP_CURRENT):
    """(tables int64 [N][180], best int32 [N]) of domain_values(cfg, n) for K <= KMAX playouts."""
    _, vals, legal, movers, _ = domain_values(cfg, n)
    tabs = np.stack([table_of(vals[i], legal[i], K, int(movers[i]), perspective) for i in range(len(vals))])
    return tabs, np.array([best_of(t) for t in tabs], np.int32)


def domain_census(cfg, n, K):
    """{class of DOMAIN_CLASSES: count} of domain_values(cfg, n) at K playouts: the playout classes count playouts, none_legal and tie records."""
    _, _, legal, _, facts = domain_values(cfg, n)
    tabs, _ = domain_tables(cfg, n, K)
    total = dict.fromkeys(DOMAIN_CLASSES, 0)
    for i, fs in enumerate(facts):
        for k, f in fs:
            if k < K:
                for name in DOMAIN_CLASSES[:5]:
                    total[name] += int(f[name])
        lg = np.flatnonzero(legal[i])
        total["none_legal"] += int(len(lg) == 0)
        total["tie"] += int(len(lg) >= 2 and int((tabs[i][lg] == tabs[i][lg].max()).sum()) >= 2)
    return total


# ---- crafted records ----------------------------------------------------------------------------------------------------------------------
def _blank(current_player=1):
    rec = np.zeros((), oz.RECORD_DTYPE)
    rec["flags"] = current_player                      # current_player | next_first_player << 3 | end_of_game << 6
    rec["box"] = 16                                    # (a playout deals nothing: the pools only make the record a plausible one)
    return rec


def stuck_record():
    """The centre holds only the token and display 0 four tiles of colour 2: whichever row the candidate (display 1, colour 2) fills, the
    display is empty afterwards, nothing is pushed to the centre, the round is not over (the token lies there) and the next player has
    nothing legal -- every playout is stuck at ply 0.  By hand, player 1 to move, all scores 0, from the mover's side per playout:
    row 4 takes the four tiles exactly: a lone wall tile, +1; row 5 stays open: 0; rows 1, 2, 3 fill (+1) and spill 3, 2, 1 tiles to the
    floor (-4, -2, -1): clamped to 0; the floor row takes four: -6, clamped to 0."""
    rec = _blank()
    rec["displays"][0][2] = 4
    rec["center"][5] = 1
    rec["box"][2] = 12
    return np.frombuffer(rec.tobytes(), np.uint8).copy()


STUCK_ACTIONS = {1 + 6 * 2 + 30 * r: (1 if r == 4 else 0) for r in range(6)}      # action -> the mover's value of one playout
STUCK_BEST = 1 + 6 * 2 + 30 * 4


def last_move_record():
    """One move from the end of the round: the centre holds two tiles of colour 0 and no token, every display is empty, player 1 to move
    with 3 points, player 2 with 5.  Every candidate (centre, colour 0, any row) ends the round: 0 plies, no draw.  By hand, score[0] -
    score[1] per playout: row 2 fills: a lone wall tile, 3 + 1 - 5 = -1; row 1 fills and spills one tile: 3 + 1 - 1 - 5 = -2; the floor
    row: 3 - 2 - 5 = -4; rows 3, 4, 5 stay open: 3 - 5 = -2."""
    rec = _blank()
    rec["center"][0] = 2
    rec["score"] = (3, 5)
    rec["box"][0] = 14
    return np.frombuffer(rec.tobytes(), np.uint8).copy()


LAST_MOVE_ACTIONS = {0: -4, 30: -2, 60: -1, 90: -2, 120: -2, 150: -2}
LAST_MOVE_BEST = 60


# ---- which shared states the emulation test runs, and how ---------------------------------------------------------------------------------
EMULATION_SIZES = (1, 2, 3, 7)
EMULATION_COMBOS = tuple((pool, persp) for pool in (oz.POOL_LID, oz.POOL_RANDOM) for persp in (0, 1, PERSP_CURRENT))


def emulation_chunks(combo):
    """The shared states cut into consecutive batches of 1, 2, 3, 7, 1, 2, ... records; every run of four batches (13 states) goes to ONE of
    the six (pool, perspective) combinations, in turn: the six together run every state exactly once, each in batches of all four sizes.
    -> [(first state, count)] of combination number `combo`."""
    out, lo, j = [], 0, 0
    while lo < 360:
        n = min(EMULATION_SIZES[j % 4], 360 - lo)
        if (j // 4) % len(EMULATION_COMBOS) == combo:
            out.append((lo, n))
        lo += n
        j += 1
    return out
