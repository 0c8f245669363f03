"""The self-play kernel's round-end scoring under the lockstep 64-lane emulation (csrc/azul_selfplay2.hpp compiled unmodified, see
test_hostcheck_selfplay2.py), against the oracle.  When only one game of a wave ends its round the sibling half scores that game's
player 1 (az2::count_score2_lone); both games on the same move, and the single game of an odd batch's last wave, keep count_score2.
Crafted records (tests/lone_round_end_cases.py) put every case on the first move: a lone round end in the lower and in the upper half,
both halves at once, a lone round end that ends the game through either player's wall row, and one whose next deal folds the lid tally
into an empty box.  Records, every stream, MT19937 words and positions, episode counters and statistics sums are compared, for both
instantiations of the kernel (without and with a move limit) and two output variants; the games then play on through natural round ends."""
import ctypes as C

import pytest

from tests import lone_round_end_cases as lc
from tests.test_hostcheck_selfplay2 import RULES, check_case, load


@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
@pytest.mark.parametrize("variant", [3, 1])
@pytest.mark.parametrize("limit", [0, 60000])
def test_lone_and_shared_round_ends_under_emulation(ruleset, variant, limit):
    L = load()
    L.sh2_set_move_limit.argtypes = [C.c_uint]
    first, pool = RULES[ruleset]
    try:
        L.sh2_set_move_limit(limit)
        check_case(L, first, pool, n=lc.N_GAMES, T=48, variant=variant, seed0=2600,
                   prepare=lambda streams: lc.apply(streams, pool, first))
    finally:
        L.sh2_set_move_limit(0)
