"""TEST helper: the host model of azul_batch_score_moves on the oracle -- the table (check_all_valid, then per legal action a byte copy of
the game, oz_move, oz_potential: game_runner.py:48-50 after azul.py:118-161), the greedy choice from it (np.argmax's rule), a classifier of
the edge classes the tests require, and the states the tests share: every record of three oracle self-play streams."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as oz

ILLEGAL = -2 ** 31
PERSP_CURRENT = 2
FLOOR_PENALTY = (0, -1, -2, -4, -6, -8, -11, -14)        # azul.py:200-209, cumulative
SEEDS, STEPS = (11, 12, 13), 120
CLASSES = ("last_source", "token", "floor_saturates", "clamped", "to_floor", "end_of_game", "one_legal", "tie", "none_legal")


def _copy(game):
    return oz.Game.from_buffer_copy(bytes(game))


def _game(rec, pool=oz.POOL_LID):
    return oz.unpack(rec, pool).game


def _moved(game, a):
    d, c, p = C.c_int(), C.c_int(), C.c_int()
    oz.lib().oz_deserialize(int(a), C.byref(d), C.byref(c), C.byref(p))
    g = _copy(game)
    oz.lib().oz_move(C.byref(g), d.value, c.value, p.value)
    return g, (d.value, c.value, p.value)


def table(rec, perspective=PERSP_CURRENT, pool=oz.POOL_LID):
    """int64[180]: score[p] - score[1 - p] after move + count_score on a copy for every legal action, ILLEGAL elsewhere."""
    game = _game(rec, pool)
    p = game.current_player - 1 if perspective == PERSP_CURRENT else int(perspective)
    out = np.full(180, ILLEGAL, np.int64)
    for a in np.flatnonzero(oz.check_all_valid(game)):
        g, _ = _moved(game, a)
        phi = int(oz.lib().oz_potential(C.byref(g)))
        out[a] = phi if p == 0 else -phi
    return out


def greedy(tab):
    """The first legal action with the maximal score; -1 when nothing is legal."""
    legal = tab != ILLEGAL
    return int(np.argmax(np.where(legal, tab, ILLEGAL))) if legal.any() else -1


def greedy_of_game(game):
    """The greedy opponent's answer for an oracle game (mover's perspective): what the rollout's replay hands to GameRunner."""
    p = game.current_player - 1
    best, best_v = -1, None
    for a in np.flatnonzero(oz.check_all_valid(game)):
        g, _ = _moved(game, a)
        phi = int(oz.lib().oz_potential(C.byref(g)))
        v = phi if p == 0 else -phi
        if best_v is None or v > best_v:
            best, best_v = int(a), v
    return best


def classify(rec, pool=oz.POOL_LID):
    """{class: count} of one state: per legal move the move classes, per state the state classes (0 / 1)."""
    L = oz.lib()
    game = _game(rec, pool)
    me = game.current_player - 1
    n = dict.fromkeys(CLASSES, 0)
    legal = np.flatnonzero(oz.check_all_valid(game))
    for a in legal:
        g, (d, c, p) = _moved(game, a)
        n["last_source"] += int(bool(L.oz_is_end_of_round(C.byref(g))))
        n["token"] += int(d == 0 and game.center[5] == 1)
        n["floor_saturates"] += int(g.floors[me] == 7 and game.floors[me] < 7)
        n["to_floor"] += int(p == 0)
        # the mover's score before the clamp: the wall points alone (floor emptied first: they are never negative), then the floor's penalty
        nofloor = _copy(g)
        nofloor.floors[me] = 0
        L.oz_count_score(C.byref(nofloor))
        n["clamped"] += int(nofloor.score[me] + FLOOR_PENALTY[min(int(g.floors[me]), 7)] < 0)
        L.oz_count_score(C.byref(g))
        n["end_of_game"] += int(bool(L.oz_is_end_of_game(C.byref(g))))
    tab = table(rec, PERSP_CURRENT, pool)
    n["one_legal"] = int(len(legal) == 1)
    n["none_legal"] = int(len(legal) == 0)
    n["tie"] = int(len(legal) >= 2 and int((tab == tab.max()).sum()) >= 2)
    return n


@functools.lru_cache(maxsize=None)
def stream_states():
    """The shared states: for seeds 11, 12, 13 the 120 records of oz.Stream(seed).advance(120) ("Random" first player, "Lid" pool).
    -> (records uint8[360][128], next_action int32[360], next_potential int64[360]): the action the stream took on the state and
    oz_potential of the record it led to, where both belong to the state's episode; next_action -1 elsewhere (the episode ended on the
    state, the stream's last record, or nobody could move)."""
    recs, nxt, pot = [], [], []
    for seed in SEEDS:
        o = oz.Stream(seed).advance(STEPS)
        ra = o["rec_after"]
        for t in range(STEPS):
            recs.append(np.frombuffer(ra[t].tobytes(), np.uint8))
            ok = o["done"][t] == 0 and t + 1 < STEPS and o["action"][t + 1] >= 0
            nxt.append(int(o["action"][t + 1]) if ok else -1)
            pot.append(int(oz.lib().oz_potential(C.byref(_game(ra[t + 1])))) if ok else 0)
    return np.stack(recs).copy(), np.array(nxt, np.int32), np.array(pot, np.int64)


@functools.lru_cache(maxsize=None)
def stream_tables(perspective=PERSP_CURRENT):
    """(tables int64[360][180], best int32[360]) of the shared states, computed once per perspective."""
    recs = stream_states()[0]
    tabs = np.stack([table(r, perspective) for r in recs])
    return tabs, np.array([greedy(t) for t in tabs], np.int32)
