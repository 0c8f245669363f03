"""Writes tests/golden/runner_players.npz: the reference's own GameRunner driven on Azul(players = P) for P = 3, 4.

Run on a machine that has the reference tree (default /root/reference, or $AZUL_REFERENCE):  python tools/gen_golden_mp_runner.py
Data only: arrays of what the reference computed, read by tests/test_mp_runner_model.py.  Nothing on the GPU side reads the reference.

The reference's GameRunner.__init__ / reset build Azul(rules=rules), i.e. two players; the only change here is a subclass whose __init__ and
reset build Azul(players=P, rules=rules) -- everything else (step, opponent_move, get_state, get_valid_moves, RandomAgent,
check_all_valid) is the reference's code, unchanged.  The agent's actions come from a separate random.Random picker over the legal
moves, so the process-global `random` stream is what the game and the opponents consume.  Recorded per agent step: the action, the
reference's reward (score[0] - score[1], game_runner.py:50), the what-if score VECTOR (deepcopy(game).count_score(); .score, :48-49) from
which the tests derive phi = s[0] - max_j>0 s[j], done, the next get_state(0) and mask, the game's fields and the MT19937 state.  When an
episode ends the driver calls reset() (opening replies included), as NNRunner.run_episode does at its start (nn_runner.py:20).
"""
import copy
import os
import random
import sys

import numpy as np

np.int = int      # the reference uses aliases removed in numpy >= 1.24 (azul.py:19-26)
np.bool = bool

REF = os.environ.get("AZUL_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from azulnet.azul import Azul  # noqa: E402
from azulnet.game_runner import GameRunner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "runner_players.npz")
STEPS = 150
SEEDS = (11, 12)


class PRunner(GameRunner):
    """The reference's GameRunner on Azul(players=P): __init__ (game_runner.py:23-36) and reset (:76-85) with the player count."""

    def __init__(self, players, rules):
        self.players = players
        self.game = Azul(players=players, rules=rules)
        self.rules = rules
        self.game_statistics = GameRunner.GameStatistics()
        from azulnet.game_runner import RandomAgent
        self.opponent = RandomAgent()
        self.game.new_round()
        self.player_score = 0
        self.move_counter = 0

    def reset(self):
        self.game = Azul(players=self.players, rules=self.rules)
        self.game.new_round()
        self.player_score = 0
        self.move_counter = 0
        while (self.game.current_player != 1):
            self.opponent_move()


def mt_state():
    st = random.getstate()[1]
    return np.array(st[:624], dtype=np.uint32), int(st[624])


def fields(g, P):
    """The game's fields in a fixed layout: displays 25, centre 6, pattern lines 4 x 25, walls 4 x 25, floors 4, scores 4, box 5, lid 5,
    current_player, next_first_player, turn_counter (int32)."""
    pl = np.zeros((4, 25), np.int32)
    pl[:P] = np.asarray(g.pattern_lines).reshape(P, 25)
    wl = np.zeros((4, 25), np.int32)
    wl[:P] = np.asarray(g.walls).reshape(P, 25)
    fl, sc = np.zeros(4, np.int32), np.zeros(4, np.int32)
    fl[:P], sc[:P] = g.floors, g.score
    box = np.asarray(getattr(g, "box_tiles", np.zeros(5)), np.int32)
    lid = np.asarray(getattr(g, "lid_tiles", np.zeros(5)), np.int32)
    return np.concatenate([np.asarray(g.game_board_displays).reshape(25), g.game_board_center, pl.reshape(-1), wl.reshape(-1), fl, sc, box, lid,
                           [g.current_player, g.next_first_player, g.turn_counter]]).astype(np.int32)


def stream(P, first, pool, seed):
    rules = {"first_player": first, "tile_pool": pool}
    random.seed(seed)
    mt0, pos0 = mt_state()
    picker = random.Random(10_000 + seed)
    runner = PRunner(P, rules)
    rows = {k: [] for k in ("action", "reward", "whatif", "done", "obs", "mask", "fields", "move_counter", "player_score", "mt", "pos")}
    init = {"obs": runner.get_state(0), "mask": runner.get_valid_moves(), "fields": fields(runner.game, P)}
    # the first decision needs player 1 to move: GameRunner() leaves the opening to reset() (NNRunner.run_episode starts with it)
    runner.reset()
    init_reset = {"obs": runner.get_state(0), "mask": runner.get_valid_moves(), "fields": fields(runner.game, P), "mt": mt_state()[0],
                  "pos": mt_state()[1]}
    for _ in range(STEPS):
        legal = np.flatnonzero(runner.get_valid_moves())
        a = int(picker.choice(list(legal)))
        reward, done = runner.step(a)
        wi = copy.deepcopy(runner.game)
        wi.count_score()
        whatif = np.zeros(4, np.int32)
        whatif[:P] = wi.score
        rows["action"].append(a)
        rows["reward"].append(int(reward))
        rows["whatif"].append(whatif)
        rows["done"].append(int(bool(done)))
        rows["player_score"].append(int(runner.player_score))
        rows["move_counter"].append(int(runner.move_counter))
        rows["fields"].append(fields(runner.game, P))           # the state the step left (before the reset below)
        if done:
            runner.reset()
        rows["obs"].append(np.asarray(runner.get_state(0), np.int16))
        rows["mask"].append(np.asarray(runner.get_valid_moves(), np.uint8))
        mt, pos = mt_state()
        rows["mt"].append(mt)
        rows["pos"].append(pos)
    out = {k: np.array(v) for k, v in rows.items()}
    out.update({"mt0": mt0, "pos0": np.int32(pos0), "init_obs": np.asarray(init["obs"], np.int32), "init_mask": np.asarray(init["mask"], np.uint8),
                "init_fields": init["fields"], "reset_obs": np.asarray(init_reset["obs"], np.int32),
                "reset_mask": np.asarray(init_reset["mask"], np.uint8), "reset_fields": init_reset["fields"], "reset_mt": init_reset["mt"],
                "reset_pos": np.int32(init_reset["pos"])})
    return out


def main():
    blob = {}
    keys = []
    for P in (3, 4):
        for first in ("Random", 1, P):
            for pool in ("Lid", "Random"):
                for seed in SEEDS:
                    key = "p%d_f%s_%s_s%d" % (P, first, pool.lower(), seed)
                    for k, v in stream(P, first, pool, seed).items():
                        blob[key + "__" + k] = v
                    keys.append(key)
    blob["keys"] = np.array(keys)
    np.savez_compressed(OUT, **blob)
    print("wrote %s: %d streams x %d agent steps" % (OUT, len(keys), STEPS))


if __name__ == "__main__":
    main()
