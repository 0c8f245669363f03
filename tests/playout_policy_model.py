"""TEST helper: the host model of azul_batch_playout_moves_policy on the oracle -- tests/playout_moves_model.py's playout with the ply's
move chosen by the playout POLICY of include/azul_hip.h, statement by statement: the uniform policy's ordinal from the ply's Philox word, or
the greedy move (tests/score_moves_model.greedy_of_game's rule: the first legal action, in ascending action order, that maximises the
mover's score difference after oz_move + oz_potential on a byte copy), the word's low byte against `explore` deciding which.  With
explore == 0 no word is read.  The draws (_Draws), the copy (sm._moved), the shared states, their global ids (GBASE, SEED, CALL) and the
domain records are the existing models'.

The value of a playout is kept as score[0] - score[1]; the tables per (explore, K) configuration are computed once."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as oz
from tests import playout_moves_model as pm
from tests import score_moves_model as sm
from tests.playout_moves_model import _Draws

ILLEGAL, PERSP_CURRENT, MAX_PLIES = pm.ILLEGAL, pm.PERSP_CURRENT, pm.MAX_PLIES
GBASE, SEED, CALL, DOMAIN_GBASE = pm.GBASE, pm.SEED, pm.CALL, pm.DOMAIN_GBASE
UNIFORM, GREEDY = 0, 1
CONFIGS = ((0, 1), (64, 2))                      # (explore, K) of the emulation; the GPU test adds (0, 3) = 3 x (0, 1) and (255, 3)
PLY_CLASSES = ("first_of_equals", "forced_floor")                 # counted per ply
PLAYOUT_CLASSES = ("ends_game", "explored_and_greedy")            # counted per playout
STATE_CLASSES = ("best_differs_from_greedy", "tie", "none_legal")  # counted per state


def greedy_ply(game):
    """(sm.greedy_of_game's move, whether two or more legal actions share its value: the choice fell to the action order).  One evaluation
    per legal action; tests/test_playout_policy_model.py holds it to sm.greedy_of_game."""
    L = oz.lib()
    p = game.current_player - 1
    best, best_v, ties = -1, None, 0
    for a in np.flatnonzero(oz.check_all_valid(game)):
        g, _ = sm._moved(game, a)
        phi = int(L.oz_potential(C.byref(g)))
        v = phi if p == 0 else -phi
        if best_v is None or v > best_v:
            best, best_v, ties = int(a), v, 1
        elif v == best_v:
            ties += 1
    return best, ties >= 2


def playout(game, a, k, draws, policy, explore):
    """One playout of candidate `a` (legal in `game`) under (policy, explore) -> (score[0] - score[1], facts).  The numbered statements are
    tests/playout_moves_model.playout's; 2.6 / 2.7 are the policy's."""
    L = oz.lib()
    g, _ = sm._moved(game, a)                                            # 1.
    ply = 0
    facts = {"first_of_equals": 0, "forced_floor": 0, "explored": 0, "greedy": 0}
    while True:                                                          # 2.
        if L.oz_is_end_of_round(C.byref(g)):                             # 2.1
            break
        L.oz_next_player(C.byref(g))                                     # 2.2
        legal = np.flatnonzero(oz.check_all_valid(g))                    # 2.3
        if len(legal) == 0:
            break
        if ply == MAX_PLIES:                                             # 2.4
            break
        J = int((legal < 30).sum())                                      # 2.5
        M = len(legal) - J
        n, base = (M, J) if M > 0 else (J, 0)
        facts["forced_floor"] += int(M == 0)
        w = draws.word(a, ply, k) if (policy == UNIFORM or explore) else None      # 2.6 (explore == 0 under the greedy policy: no word is read)
        if w is not None and (policy == UNIFORM or (w & 0xFF) < explore):      # 2.7 the low byte decides the branch, the high bits the ordinal
            move = int(legal[base + ((w * n) >> 32)])
            facts["explored"] += 1
        else:
            move, tied = greedy_ply(g)
            facts["greedy"] += 1
            facts["first_of_equals"] += int(tied)
        d, c, p = C.c_int(), C.c_int(), C.c_int()
        L.oz_deserialize(move, C.byref(d), C.byref(c), C.byref(p))
        L.oz_move(C.byref(g), d.value, c.value, p.value)
        ply += 1
    L.oz_count_score(C.byref(g))                                         # 3.
    facts["ends_game"] = bool(L.oz_is_end_of_game(C.byref(g)))
    facts["explored_and_greedy"] = facts["explored"] > 0 and facts["greedy"] > 0
    facts["plies"] = ply
    return int(g.score[0]) - int(g.score[1]), facts


def game_values(game, G, K, policy=GREEDY, explore=0, seed=SEED, call=CALL):
    """(values int64 [180][K] of score[0] - score[1] per playout, legal bool [180], facts: one dict per playout run).  Under the greedy policy
    with explore == 0 the K playouts of a candidate are equal by definition: one is run, its value stands K times."""
    legal = oz.check_all_valid(game)
    vals = np.zeros((180, K), np.int64)
    facts = []
    draws = _Draws(seed, call, G, K)
    runs = 1 if (policy == GREEDY and explore == 0) else K
    for a in np.flatnonzero(legal):
        for k in range(runs):
            vals[a, k], f = playout(game, int(a), k, draws, policy, explore)
            facts.append(f)
        vals[a, runs:] = vals[a, 0]
    return vals, legal, facts


def state_values(rec, G, K, policy=GREEDY, explore=0, seed=SEED, call=CALL, pool=oz.POOL_LID):
    return game_values(sm._game(rec, pool), G, K, policy, explore, seed, call)


table_of, best_of, mover_of = pm.table_of, pm.best_of, pm.mover_of


def table(rec, G, K, policy=GREEDY, explore=0, perspective=PERSP_CURRENT, seed=SEED, call=CALL, pool=oz.POOL_LID):
    """(table int64 [180], best) of one record as global game G."""
    vals, legal, _ = state_values(rec, G, K, policy, explore, seed, call, pool)
    tab = table_of(vals, legal, K, mover_of(rec), perspective)
    return tab, best_of(tab)


def action_of_game(game, G, K, explore, seed, call):
    """The greedy-playout player's answer for an oracle game (mover's perspective): what the rollout's replay hands to GameRunner."""
    vals, legal, _ = game_values(game, G, K, GREEDY, explore, seed, call)
    if not legal.any():
        return -1
    return best_of(table_of(vals, legal, K, game.current_player - 1))


@functools.lru_cache(maxsize=None)
def stream_values(explore, K, policy=GREEDY):
    """The shared values of a configuration, computed once: (values int64 [360][180][K], legal bool [360][180], movers int [360], facts [360])
    of sm.stream_states() with state i as global game GBASE + i at (SEED, CALL)."""
    recs = sm.stream_states()[0]
    vals, legal, facts = zip(*[state_values(r, GBASE + i, K, policy, explore) for i, r in enumerate(recs)])
    return np.stack(vals), np.stack(legal), np.array([mover_of(r) for r in recs]), list(facts)


def _tables(vals, legal, movers, K, perspective):
    tabs = np.stack([table_of(vals[i], legal[i], K, int(movers[i]), perspective) for i in range(len(vals))])
    return tabs, np.array([best_of(t) for t in tabs], np.int32)


@functools.lru_cache(maxsize=None)
def stream_tables(explore, K, perspective=PERSP_CURRENT):
    """(tables int64 [360][180], best int32 [360]) of the shared states under the greedy policy.  explore == 0: K times the one playout's table
    (the values of (0, 1) are the only ones computed)."""
    vals, legal, movers, _ = stream_values(explore, 1 if explore == 0 else K)
    if explore == 0:
        vals = np.repeat(vals[:, :, :1], K, axis=2)
    return _tables(vals, legal, movers, K, perspective)


def _census(facts_per_state, tabs, legal, best, greedy_best):
    total = dict.fromkeys(PLY_CLASSES + PLAYOUT_CLASSES + STATE_CLASSES + ("playouts", "longest"), 0)
    for i, fs in enumerate(facts_per_state):
        for f in fs:
            for name in PLY_CLASSES + PLAYOUT_CLASSES:
                total[name] += int(f[name])
            total["playouts"] += 1
            total["longest"] = max(total["longest"], f["plies"])
        lg = np.flatnonzero(legal[i])
        total["none_legal"] += int(len(lg) == 0)
        total["best_differs_from_greedy"] += int(len(lg) > 0 and best[i] != greedy_best[i])
        total["tie"] += int(len(lg) >= 2 and int((tabs[i][lg] == tabs[i][lg].max()).sum()) >= 2)
    return total


def census(explore, K, indices=None):
    """{class: count} over the 360 shared states (or those of `indices`) at (explore, K): the ply classes count plies, the playout classes the playouts that were run
    (one per candidate at explore == 0), the state classes states; "playouts" and "longest" ride along."""
    _, legal, _, facts = stream_values(explore, 1 if explore == 0 else K)
    tabs, best = stream_tables(explore, K)
    greedy_best = sm.stream_tables(PERSP_CURRENT)[1]
    if indices is not None:
        idx = list(indices)
        facts, tabs, legal, best, greedy_best = [facts[i] for i in idx], tabs[idx], legal[idx], best[idx], greedy_best[idx]
    return _census(facts, tabs, legal, best, greedy_best)


# ---- arbitrary in-domain records (tests/domain_records.py), the batches of tests/playout_moves_model.domain_values ----------------------------
@functools.lru_cache(maxsize=None)
def domain_values(cfg, n, explore, K):
    """(records uint8 [N][128], values int64 [N][180][K], legal bool [N][180], movers int [N], facts [N]) of pm.domain_values(cfg, n)'s
    records under the greedy policy; record i is global game DOMAIN_GBASE + i at (SEED, CALL)."""
    raw = pm.domain_values(cfg, n)[0]
    vals, legal, facts = zip(*[state_values(r, DOMAIN_GBASE + i, K, GREEDY, explore, pool=cfg[2]) for i, r in enumerate(raw)])
    return raw, np.stack(vals), np.stack(legal), np.array([mover_of(r) for r in raw]), list(facts)


def domain_tables(cfg, n, explore, K, perspective=PERSP_CURRENT):
    _, vals, legal, movers, _ = domain_values(cfg, n, explore, K)
    return _tables(vals, legal, movers, K, perspective)


def domain_census(cfg, n, explore, K):
    raw, _, legal, _, facts = domain_values(cfg, n, explore, K)
    tabs, best = domain_tables(cfg, n, explore, K)
    greedy_best = [sm.greedy(sm.table(r, PERSP_CURRENT, cfg[2])) for r in raw]
    return _census(facts, tabs, legal, best, greedy_best)


# ---- a crafted record ---------------------------------------------------------------------------------------------------------------------------
def tie_ply_record():
    """Every playout of this record is ONE greedy ply, and that ply's six values are equal: the action order decides it.
    Player 1 to move; scores 0, walls and lines empty, centre empty and without the token; display 1 holds two tiles of colour 0 and one of
    colour 1; player 2's floor holds 7 tiles (-14).  Player 1's candidates are (display 1, colour c, row r) = 1 + 6 c + 30 r, twelve of
    them.  Whichever he plays, the display's other colour goes to the centre, now the only source, and player 2 replies:
      the greedy ply: (centre, the other colour) into the floor row or a pattern row 1..5.  His floor stays at 7 (the cap), so his score
      after count_score is max(0, 0 - 14 + wall points) with at most one lone wall tile (+1): 0 for all six moves, and player 1's score
      does not depend on the reply.  Six equal values: the greedy move is the FIRST, the floor row -- action 6 after a candidate of
      colour 0, action 0 after one of colour 1.  The round is over; player 2 scores 0.
    Player 1 at the end of the round, hence score[0] - score[1] of the playout:
      colour 0 (two tiles): floor row (1): -2 -> 0; row 1 (31): full, one tile spills: +1 - 1 = 0; row 2 (61): full, a lone wall tile: +1;
                            rows 3, 4, 5 (91, 121, 151): open: 0
      colour 1 (one tile):  floor row (7): -1 -> 0; row 1 (37): full: +1; rows 2..5 (67, 97, 127, 157): open: 0
    The maximum 1 stands at 37 and 61: `best` is 37.  From player 2's side every sign flips and the first maximum (0) is action 1."""
    rec = pm._blank()
    rec["displays"][0][0] = 2
    rec["displays"][0][1] = 1
    rec["floors"][1] = 7
    rec["box"][0] = 14
    rec["box"][1] = 15
    return np.frombuffer(rec.tobytes(), np.uint8).copy()


TIE_PLY_ACTIONS = {1: 0, 31: 0, 61: 1, 91: 0, 121: 0, 151: 0, 7: 0, 37: 1, 67: 0, 97: 0, 127: 0, 157: 0}      # action -> score[0] - score[1] of one playout
TIE_PLY_BEST = 37
TIE_PLY_REPLY = {0: 6, 1: 0}                     # the candidate's colour -> player 2's greedy ply: the floor row, first of six equal values


# ---- which shared states the emulation test runs ------------------------------------------------------------------------------------------
EMULATION_SIZES, EMULATION_COMBOS, emulation_chunks = pm.EMULATION_SIZES, pm.EMULATION_COMBOS, pm.emulation_chunks
