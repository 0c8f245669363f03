"""Writes tests/golden/runner_players_net.npz: the reference's own GameRunner on Azul(players = P), P = 3, 4, with a NETWORK opponent.

Run on a machine that has the reference tree (default /root/reference, or $AZUL_REFERENCE):  python tools/gen_golden_mp_net_opponent.py
Data only: arrays of what the reference computed, read by tests/test_mp_net_model.py and tests/test_gpu_mp_net.py.  Nothing on the GPU side
reads the reference.

The runner is tools/gen_golden_mp_runner.py's PRunner (the reference's GameRunner with Azul(players=P) in __init__ / reset) built with
opponent = the reference's Agent() whose ac_net is the reference's ActorCritic(obs_size, 180), seeded with torch.manual_seed: GameRunner(
opponent=Agent(...)) (game_runner.py:27-30).  Its get_a_output is wrapped to record every call -- the state opponent_move() hands over (the
mover's get_state(perspective=current_player-1), game_runner.py:38, order = [p] + the others ascending), the mask, the player moved for,
move_counter and the answer (np.random.choice on the net's distribution, agent.py:73-81).  The agent's actions come from a separate
random.Random picker, so the process-global `random` stream is what the game consumes.  Per agent step: the action, the reference's reward,
the what-if score vector (phi = s[0] - max_j>0 s[j] is derived from it), done, the game's fields (before the reset), move_counter, the next
get_state(0) and mask, and the MT19937 state.  When an episode ends the driver calls reset() (opening moves included), as
NNRunner.run_episode does at its start (nn_runner.py:20); its opponent calls belong to that step.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from azulnet.agent import Agent  # noqa: E402
from azulnet.model import ActorCritic  # noqa: E402

from gen_golden_mp_runner import PRunner, fields, mt_state  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "runner_players_net.npz")
STEPS = 80
SEEDS = (21, 22)


class RecordingAgent:
    """The reference's Agent with ac_net = ActorCritic(obs_size, 180); every get_a_output call is recorded."""

    def __init__(self, runner, obs_size, net_seed):
        self.runner = runner
        self.agent = Agent()
        torch.manual_seed(net_seed)
        self.agent.ac_net = ActorCritic(obs_size, 180)
        self.calls = []
        self.step = -1

    def get_a_output(self, state, valid_moves):
        a = int(self.agent.get_a_output(state, valid_moves))
        self.calls.append({"step": self.step, "state": np.asarray(state, np.int16), "mask": valid_moves.numpy()[0].astype(np.uint8),
                           "player": int(self.runner.game.current_player), "move_counter": int(self.runner.move_counter), "answer": a})
        return a


def stream(P, first, pool, seed):
    rules = {"first_player": first, "tile_pool": pool}
    random.seed(seed)
    np.random.seed(seed)
    mt0, pos0 = mt_state()
    picker = random.Random(20_000 + seed)
    runner = PRunner(P, rules)
    opp = RecordingAgent(runner, 5 * 5 + 6 + 52 * P + 1, 300 + seed)
    runner.opponent = opp
    runner.reset()                                               # step -1: the opening of the first episode
    rows = {k: [] for k in ("action", "reward", "whatif", "done", "obs", "mask", "fields", "move_counter", "player_score", "mt", "pos")}
    for t in range(STEPS):
        opp.step = t
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
    c = opp.calls
    out.update({"mt0": mt0, "pos0": np.int32(pos0), "call_step": np.array([x["step"] for x in c], np.int32),
                "call_state": np.array([x["state"] for x in c], np.int16), "call_mask": np.array([x["mask"] for x in c], np.uint8),
                "call_player": np.array([x["player"] for x in c], np.int32), "call_moves": np.array([x["move_counter"] for x in c], np.int32),
                "call_answer": np.array([x["answer"] for x in c], np.int32)})
    return out


def main():
    blob = {}
    keys = []
    for P in (3, 4):
        for first in ("Random", 1):
            for pool in ("Lid", "Random"):
                for seed in SEEDS:
                    key = "p%d_f%s_%s_s%d" % (P, first, pool.lower(), seed)
                    for k, v in stream(P, first, pool, seed).items():
                        blob[key + "__" + k] = v
                    keys.append(key)
    blob["keys"] = np.array(keys)
    np.savez_compressed(OUT, **blob)
    print("wrote %s: %d streams x %d agent steps, %d opponent calls" % (OUT, len(keys), STEPS,
                                                                     sum(len(blob[k + "__call_step"]) for k in keys)))


if __name__ == "__main__":
    main()
