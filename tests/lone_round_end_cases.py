"""Crafted two-player records whose NEXT move ends the round, for the self-play kernel's round-end scoring paths: one game of a wave
ending its round alone (the sibling half scores that game's player 1), both games of a wave on the same move, and a lone round end in the
last wave of an odd batch (one game, the other half absent).  Used by test_hostcheck_lone_round_end.py (CPU emulation) and
test_gpu_lone_round_end.py (device)."""
import ctypes as C

from oracle import oracle as oz

N_GAMES = 13
# game -> kind.  Waves are game pairs (2 b, 2 b + 1): the even game plays in lanes 0..31, the odd one in lanes 32..63.
CASES = {
    0: "plain",       # lone round end in the lower half
    3: "plain",       # lone round end in the upper half
    4: "plain",       # both halves end their round on the same move
    5: "plain",
    6: "over1",       # lone, lower half: player 1's line completes a wall row -> the game ends
    9: "lid",         # lone, upper half: the box is empty -> the next round's deal folds the lid tally in
    11: "over0",      # lone, upper half: player 0's line completes a wall row -> the game ends
    12: "plain",      # the odd batch's last wave: one game, no sibling half
}
LEAD_MOVES = 3        # moves each stream plays before the record is rewritten (first round, well before its end)


def _bit(r, c):
    return 1 << (5 * r + c)


def crafted_record(rec, kind):
    """rec: the record of a game a few moves into a round.  Returns a copy in which one tile of colour 0 is left (centre, no token) --
    whatever the mover does ends the round -- and both players hold full pattern lines next to partly filled walls."""
    rec = rec.copy()
    rec["displays"][:] = 0
    rec["center"][:] = [1, 0, 0, 0, 0, 0]
    pl = rec["pattern_lines"]
    pl[:] = 0
    pl[0, 1, 4] = 2                           # player 0: rows 1 and 3 full, row 2 partial
    pl[0, 3, 2] = 4
    pl[0, 2, 1] = 1
    pl[1, 0, 1] = 1                           # player 1: rows 0, 2 and 4 full
    pl[1, 2, 2] = 3
    pl[1, 4, 3] = 5
    w0 = _bit(1, 0) | _bit(1, 1) | _bit(0, 4) | _bit(2, 4) | _bit(3, 1) | _bit(3, 3)
    w1 = _bit(0, 2) | _bit(0, 3) | _bit(1, 1) | _bit(2, 1) | _bit(3, 2) | _bit(4, 0) | _bit(4, 1)
    if kind == "over0":
        w0 |= _bit(3, 0) | _bit(3, 4)         # row 3 then lacks only colour 2, which player 0's full line brings
    if kind == "over1":
        w1 |= _bit(4, 2) | _bit(4, 4)         # row 4 then lacks only colour 3, which player 1's full line brings
    rec["walls"][:] = [w0, w1]
    rec["floors"][:] = [2, 3]
    if kind == "lid":
        rec["box"][:] = 0
        rec["lid"][:] = [12, 12, 12, 12, 12]
    return rec


def apply(streams, pool, first_player=oz.FIRST_RANDOM):
    """Play LEAD_MOVES moves on every stream, then rewrite the records of the CASES games (the oracle's state and what the kernel loads)."""
    for s in streams:
        s.advance(LEAD_MOVES, want_records=False)
    for g, kind in CASES.items():
        if g >= len(streams):
            continue
        s = streams[g]
        rec = crafted_record(s.record(), kind)
        q = oz.unpack(rec, tile_pool=pool, first_player=first_player)
        C.memmove(C.byref(s.q), C.byref(q), C.sizeof(q))
