"""TEST helper: the host model of azul_batch_mp_score_moves on the oracle's existing primitives, through tests/domain_records.Game -- the
table (mask(), then per legal action a struct copy of the game, oz_deserialize_x + oz_move, oz_count_score, the scores: s[p] - max_{j != p}
s[j]; game_runner.py:48-50 after azul.py:118-161, BEYOND THE REFERENCE for P > 2 like the wide runner's reward), the greedy choice from it
(np.argmax's rule), a classifier of the edge classes the tests require, and the states the tests share, computed once per session: leave
them unchanged."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as oz
from tests import domain_records as dr

ILLEGAL = -2 ** 31
PERSP_MOVER = 7
FLOOR_PENALTY = (0, -1, -2, -4, -6, -8, -11, -14)        # azul.py:200-209, cumulative
SEEDS, STEPS, DOMAIN_N = (11, 12, 13), 120, 64
# (players, ext, tile_pool, first_player): the five instantiations (P, D) = (2, 5), (3, 5), (3, 7), (4, 5), (4, 9); "Lid" pool and a
# Random first player, one shape on the "Random" pool with first player 1
_X = oz.EXT_DISPLAYS_2P1 | oz.EXT_END_BONUS | oz.EXT_SHORT_DEAL
SHAPES = [(2, oz.EXT_END_BONUS, oz.POOL_LID, oz.FIRST_RANDOM), (3, 0, oz.POOL_LID, oz.FIRST_RANDOM), (3, _X, oz.POOL_LID, oz.FIRST_RANDOM),
          (4, 0, oz.POOL_RANDOM, 1), (4, _X, oz.POOL_LID, oz.FIRST_RANDOM)]
MOVE_CLASSES = ("last_source", "token", "floor_saturates", "clamped", "to_floor", "end_of_game")
STATE_CLASSES = ("tie", "one_legal", "none_legal", "lead_changes", "persp_differs", "best_high")
CLASSES = MOVE_CLASSES + STATE_CLASSES


def cfg_of(shape):
    return shape[:3]


def displays(shape):
    return dr.displays(cfg_of(shape))


def num_actions(shape):
    return 30 * (displays(shape) + 1)


def shape_id(shape):
    return "p%dd%d" % (shape[0], displays(shape))


def perspectives(shape):
    return list(range(shape[0])) + [PERSP_MOVER]


def unreachable(shape):
    """The classes a shape cannot reach: with two seats the best other seat is the only other seat and another seat's view is the mover's
    negated; an action numbered 256 or above needs the 300 actions of nine displays."""
    out = set()
    if shape[0] == 2:
        out |= {"lead_changes", "persp_differs"}
    if num_actions(shape) <= 256:
        out.add("best_high")
    return out


def _copy(game):
    return oz.Game.from_buffer_copy(bytes(game))


def _moved(g, a):
    """A struct copy of dr.Game g's game after oz_deserialize_x + oz_move (the unchecked move)."""
    h = _copy(g.g)
    oz.lib().oz_move(C.byref(h), *g.split(a))
    return h


def _scores(game, P):
    h = _copy(game)
    oz.lib().oz_count_score(C.byref(h))
    return [int(h.score[j]) for j in range(P)]


def margin(s, p):
    return s[p] - max(x for j, x in enumerate(s) if j != p)


def table(rec, cfg, perspective=PERSP_MOVER):
    """int64[num_actions]: s[p] - max_{j != p} s[j] after move + count_score on a copy for every legal action, ILLEGAL elsewhere."""
    g = dr.Game(np.asarray(rec).view(oz.RECORD_NP_DTYPE).reshape(()), cfg)
    P = cfg[0]
    p = g.mover() if perspective == PERSP_MOVER else int(perspective)
    mask = g.mask()
    out = np.full(len(mask), ILLEGAL, np.int64)
    for a in np.flatnonzero(mask):
        out[a] = margin(_scores(_moved(g, a), P), p)
    return out


def greedy(tab):
    """The first legal action with the maximal score; -1 when nothing is legal."""
    legal = tab != ILLEGAL
    return int(np.argmax(np.where(legal, tab, ILLEGAL))) if legal.any() else -1


def greedy_of_game(game, P):
    """The greedy seat's answer for an oracle game (the mover's perspective): what the rollout's replay hands to the runner."""
    g = dr.Game.__new__(dr.Game)
    g.g, g.wide = game, True
    p = g.mover()
    best, best_v = -1, None
    for a in np.flatnonzero(g.mask()):
        v = margin(_scores(_moved(g, a), P), p)
        if best_v is None or v > best_v:
            best, best_v = int(a), v
    return best


def classify(rec, cfg):
    """{class: count} of one state: per legal move the move classes, per state the state classes (0 / 1; best_high: rows over the P + 1
    perspectives)."""
    L = oz.lib()
    P = cfg[0]
    g = dr.Game(np.asarray(rec).view(oz.RECORD_NP_DTYPE).reshape(()), cfg)
    me = g.mover()
    n = dict.fromkeys(CLASSES, 0)
    legal = np.flatnonzero(g.mask())
    after = []
    for a in legal:
        h = _moved(g, a)
        d, c, p = g.split(a)
        n["last_source"] += int(bool(L.oz_is_end_of_round(C.byref(h))))
        n["token"] += int(d == 0 and g.g.center[5] == 1)
        n["floor_saturates"] += int(h.floors[me] == 7 and g.g.floors[me] < 7)
        n["to_floor"] += int(p == 0)
        # the mover's score before the clamp: the wall points alone (floor emptied first: they are never negative), then the floor's penalty
        nofloor = _copy(h)
        nofloor.floors[me] = 0
        L.oz_count_score(C.byref(nofloor))
        n["clamped"] += int(nofloor.score[me] + FLOOR_PENALTY[min(int(h.floors[me]), 7)] < 0)
        L.oz_count_score(C.byref(h))
        n["end_of_game"] += int(bool(L.oz_is_end_of_game(C.byref(h))))
        after.append([int(h.score[j]) for j in range(P)])
    n["one_legal"] = int(len(legal) == 1)
    n["none_legal"] = int(len(legal) == 0)
    if len(legal):
        mine = np.array([margin(s, me) for s in after])
        n["tie"] = int(len(legal) >= 2 and int((mine == mine.max()).sum()) >= 2)
        for p in range(P):
            if p == me:
                continue
            others = [j for j in range(P) if j != p]
            leaders = {others[int(np.argmax([s[j] for j in others]))] for s in after}
            n["lead_changes"] |= int(len(leaders) >= 2)
            theirs = np.array([margin(s, p) for s in after])
            n["persp_differs"] |= int(int(np.argmax(theirs)) != int(np.argmin(mine)))
        for p in list(range(P)) + [me]:
            n["best_high"] += int(int(legal[int(np.argmax([margin(s, p) for s in after]))]) >= 256)
    return n


def fresh_record(shape):
    """One game before its first new_round: current_player 0 (the seat to move is P - 1), every source empty, nothing legal."""
    P, ext, pool, first = shape
    g, r = oz.Game(), oz.seeded_rng(5)
    assert oz.lib().oz_init_ext(C.byref(g), P, first, pool, ext, C.byref(r)) == 0
    return np.frombuffer(oz.pack_np(g).tobytes(), np.uint8).copy()


@functools.lru_cache(maxsize=None)
def states(i):
    """The shared states of SHAPES[i], uint8[3 * 120 + 64 + 1][256]: the records of oz.StreamX(seed, ...).advance(120) for seeds 11, 12, 13,
    domain_records.wide(64, P, D, seed) (arbitrary in-domain records, incl. states no game reaches), one game before its first new_round."""
    shape = SHAPES[i]
    P, ext, pool, first = shape
    recs = []
    for seed in SEEDS:
        ra = oz.StreamX(seed, P, first, pool, ext).advance(STEPS)["rec_after"]
        recs += [np.frombuffer(ra[t].tobytes(), np.uint8) for t in range(STEPS)]
    dom = dr.wide(DOMAIN_N, P, displays(shape), 7300 + i)
    recs += [np.frombuffer(dom[k].tobytes(), np.uint8) for k in range(DOMAIN_N)]
    recs.append(fresh_record(shape))
    out = np.stack(recs).copy()
    out.setflags(write=False)
    return out


N_STREAM, N_STATES = len(SEEDS) * STEPS, len(SEEDS) * STEPS + DOMAIN_N + 1


@functools.lru_cache(maxsize=None)
def tables(i, perspective=PERSP_MOVER):
    """(tables int64[N_STATES][num_actions], best int32[N_STATES]) of the shared states of SHAPES[i], computed once per perspective."""
    cfg = cfg_of(SHAPES[i])
    tabs = np.stack([table(r, cfg, perspective) for r in states(i)])
    best = np.array([greedy(t) for t in tabs], np.int32)
    tabs.setflags(write=False)
    best.setflags(write=False)
    return tabs, best


@functools.lru_cache(maxsize=None)
def census(i):
    """(per-state class counts: list of dicts, totals over the stream states, totals over the domain records + the fresh game)"""
    cfg = cfg_of(SHAPES[i])
    per = [classify(r, cfg) for r in states(i)]
    tot = lambda rows: {k: sum(int(bool(r[k])) if k in STATE_CLASSES and k != "best_high" else r[k] for r in rows) for k in CLASSES}
    return per, tot(per[:N_STREAM]), tot(per[N_STREAM:])
