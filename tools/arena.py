"""Rank networks by playing them against each other: a round-robin tournament inside the window kernels (Arena), its win matrix and
Bradley-Terry ratings, printed and written as JSON.

  --nets a.pt b.pt ...          plain state_dict files (torch.load(..., weights_only=True));
  --checkpoints c1.pt c2.pt ... BatchedTrainer checkpoints, read as load_checkpoint reads them (map_location="cpu", weights_only=False);
                                only their "policy" entry is used.
Both may be given; the members are numbered in the order nets, then checkpoints.  Every network must have the shape of the batch:
ActorCritic(136, 180, hidden 180) for two players, ActorCritic(obs_size, num_actions, hidden 180) for --players 3 / 4.

Usage: python tools/arena.py --nets a.pt b.pt [--checkpoints ...] [--games 4096] [--window 32] [--windows-per-round 8] [--rounds N]
                             [--players 2] [--selection Distribution|Max] [--out arena.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from azul_deep_reinforcement_learning_amd import Arena, BatchedActorCritic  # noqa: E402
from azul_deep_reinforcement_learning_amd.batch import batch_shape  # noqa: E402


def load_members(args, rules):
    sds = [(f, torch.load(f, map_location="cpu", weights_only=True)) for f in args.nets]
    sds += [(f, torch.load(f, map_location="cpu", weights_only=False)["policy"]) for f in args.checkpoints]
    n_obs, n_act = batch_shape(args.players, rules)
    nets = []
    for f, sd in sds:
        net = BatchedActorCritic(n_obs, n_act, 180)
        try:
            net.load_state_dict(sd)
        except RuntimeError as e:
            raise SystemExit("%s is no ActorCritic(%d, %d, hidden 180) of this batch: %s" % (f, n_obs, n_act, e))
        nets.append(net)
    return [f for f, _ in sds], nets


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nets", nargs="*", default=[])
    ap.add_argument("--checkpoints", nargs="*", default=[])
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows-per-round", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=None, help="schedule rounds (default: one full cycle, every ordered pair played)")
    ap.add_argument("--players", type=int, default=2)
    ap.add_argument("--selection", choices=["Distribution", "Max"], default="Distribution")
    ap.add_argument("--out", default="arena.json")
    args = ap.parse_args()
    rules = {"first_player": "Random", "tile_pool": "Lid"}
    names, nets = load_members(args, rules)
    if not nets:
        raise SystemExit("nothing to rank: give --nets and / or --checkpoints")
    ar = Arena(nets, n_games=args.games, window=args.window, players=args.players, rules=rules, selection=args.selection)
    ar.play_schedule(args.windows_per_round, args.rounds)
    res = ar.results()
    rt = ar.ratings()
    K = len(nets)
    with np.errstate(invalid="ignore", divide="ignore"):
        rate = res["wins"] / res["episodes"]
    print("win rate of the agent seat (row) against the opponent seat (column); episodes in brackets")
    for a in range(K):
        print("%3d  " % a + "  ".join("%6.3f (%6d)" % (rate[a, o], res["episodes"][a, o]) if res["episodes"][a, o] else "     - (     0)"
                                     for o in range(K)))
    print("ratings (Bradley-Terry, 400 log10 strength, mean 0; %d iterations)" % rt["iterations"])
    for i in np.argsort(-rt["rating"]):
        print("%8.1f  %3d  %s" % (rt["rating"][i], i, names[i]))
    nan_none = lambda a: [[None if np.isnan(x) else float(x) for x in row] for row in np.asarray(a, dtype=np.float64)]
    with open(args.out, "w") as fh:
        json.dump({"members": names, "games": args.games, "window": args.window, "windows_per_round": args.windows_per_round,
                   "players": args.players, "selection": args.selection, "episodes": res["episodes"].tolist(), "wins": nan_none(res["wins"]),
                   "win_rate": nan_none(rate), "mean": {k: nan_none(v) for k, v in res["mean"].items()},
                   "rating": [float(x) for x in rt["rating"]], "strength": [float(x) for x in rt["strength"]],
                   "iterations": int(rt["iterations"])}, fh, indent=1)
        fh.write("\n")
    print("written: %s" % args.out)


if __name__ == "__main__":
    main()
