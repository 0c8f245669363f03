"""The greedy_margin seats inside the wide window kernel at 4096 games and window 32, beside the per-cut path they replace and the
RandomAgent wide window kernel, for the five compiled shapes (players, displays) = (2, 5), (3, 5), (3, 7), (4, 5), (4, 9) -- per shape three
PolicyRollouts measured in ONE process, written to profiles/mp_greedy_rollout_bench.json:

  * greedy_per_cut   opponent="greedy_margin": one azul_batch_mp_score_moves launch, one azul_batch_mp_net_step_reply launch and one host
                     synchronisation per reply round (the rollout of tools/mp_score_moves_bench.py, re-measured here);
  * greedy_fused     the same with fused_wide=True, fused_seats=True: azul_batch_mp_policy_rollout_greedy, one launch per window;
  * random_fused     opponent="random", fused_wide=True: azul_x_policy_rollout_kernel<P, D, 1>, the RandomAgent seats inside the env step.

Agent steps/s: wall clock over a number of windows that ends in a device synchronisation, after three warm-up windows
(tools/greedy_rollout_bench.py's conventions); `--repeats` such measurements per rollout, the three rollouts alternating, the median
reported beside every repeat; `spread` = (max - min) / median of the repeats.  Reply rounds per agent step from the recorded opp_replies:
per step the maximum over the batch (the reply rounds the per-cut path launches), over the two games of a wave (the passes of the window
kernel's reply loop) and the mean over the games (the opponent moves themselves).

Usage: python tools/mp_greedy_rollout_bench.py [--games 4096] [--window 32] [--windows 100] [--per-cut-windows 8] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from azul_deep_reinforcement_learning_amd import BatchedActorCritic, PolicyRollout  # noqa: E402
from azul_deep_reinforcement_learning_amd.batch import batch_shape  # noqa: E402

EXT = {"displays": "2P+1", "bonuses": "end", "short_deal": True}
SHAPES = [(2, {"first_player": "Random", "tile_pool": "Lid", "bonuses": "end"}), (3, {"first_player": "Random", "tile_pool": "Lid"}),
          (3, dict({"first_player": "Random", "tile_pool": "Lid"}, **EXT)), (4, {"first_player": 1, "tile_pool": "Random"}),
          (4, dict({"first_player": "Random", "tile_pool": "Lid"}, **EXT))]
KINDS = {"greedy_per_cut": dict(opponent="greedy_margin"), "greedy_fused": dict(opponent="greedy_margin", fused_wide=True, fused_seats=True),
         "random_fused": dict(opponent="random", fused_wide=True)}


def make(args, players, rules, kind):
    torch.manual_seed(0)
    n_obs, n_act = batch_shape(players, rules)
    ro = PolicyRollout(BatchedActorCritic(n_obs, n_act, 180), n_games=args.games, window=args.window, players=players, rules=rules, **KINDS[kind])
    assert ro.fused_wide == (kind != "greedy_per_cut") and ro.fused_seats == (kind == "greedy_fused") and not ro.use_graph
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    return ro


def timed(ro, windows):
    """-> (agent steps/s, the first windows' opp_replies [<= 8 T][N] or None)"""
    replies = []
    ro.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        tr = ro.run_window()
        if ro.cut and len(replies) < 8:
            ro.join()                                            # (the caller's stream waits for the window on the device: no host wait)
            replies.append(tr[0]["opp_replies"].clone())
    ro.synchronize()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return ro.n * ro.T * windows / dt, (torch.cat(replies) if replies else None)


def rounds(rep):
    r = rep.float()
    n2 = r.shape[1] // 2 * 2
    pair = torch.maximum(r[:, 0:n2:2], r[:, 1:n2:2])
    return {"reply_rounds_per_step_mean": round(float(r.max(dim=1).values.mean()), 3), "reply_rounds_per_step_max": int(r.max()),
            "wave_passes_per_step_mean": round(float(pair.mean()), 3), "opponent_moves_per_step_mean": round(float(r.mean()), 3)}


def shape_row(args, players, rules):
    ros = {k: make(args, players, rules, k) for k in KINDS}
    rates, reps = {k: [] for k in KINDS}, {}
    for _ in range(args.repeats):
        for k, ro in ros.items():
            rate, rep = timed(ro, args.per_cut_windows if k == "greedy_per_cut" else args.windows)
            rates[k].append(round(rate))
            if rep is not None:
                reps[k] = rep
    n_act = ros["greedy_fused"].num_actions
    row = {"players": players, "displays": n_act // 30 - 1, "num_actions": n_act, "rules": rules}
    for k in KINDS:
        med = sorted(rates[k])[len(rates[k]) // 2]
        row[k] = {"agent_steps_per_s": med, "repeats": rates[k], "spread": round((max(rates[k]) - min(rates[k])) / med, 4),
                  "windows_timed": args.per_cut_windows if k == "greedy_per_cut" else args.windows,
                  "us_per_window": round(args.games * args.window / med * 1e6, 1)}
        if k in reps:
            row[k].update(rounds(reps[k]))
    row["fused_over_per_cut"] = round(row["greedy_fused"]["agent_steps_per_s"] / row["greedy_per_cut"]["agent_steps_per_s"], 2)
    row["fused_over_random_fused"] = round(row["greedy_fused"]["agent_steps_per_s"] / row["random_fused"]["agent_steps_per_s"], 3)
    row["ratio_exceeds_spread"] = bool(row["fused_over_per_cut"] - 1.0 > row["greedy_fused"]["spread"] + row["greedy_per_cut"]["spread"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=100)
    ap.add_argument("--per-cut-windows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp_greedy_rollout_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are the MI355X's: no device, no measurement"
    res = {"tool": "python tools/mp_greedy_rollout_bench.py --games %d --window %d --windows %d --per-cut-windows %d --repeats %d"
                   % (args.games, args.window, args.windows, args.per_cut_windows, args.repeats),
           "note": "one process, one GPU; PolicyRollout agent steps/s, wall clock over the timed windows ending in a device synchronisation, three "
                   "warm-up windows; per shape the three rollouts alternate, `repeats` holds every measurement, agent_steps_per_s their median and "
                   "spread (max - min) / median. greedy_per_cut: one azul_batch_mp_score_moves launch + one net_step_reply launch + one host "
                   "synchronisation per reply round; greedy_fused: azul_batch_mp_policy_rollout_greedy, one launch per window; random_fused: "
                   "azul_batch_mp_policy_rollout with RandomAgent seats. No fixed target: fused_over_per_cut is the ratio of the same run, "
                   "ratio_exceeds_spread says whether it is larger than the two rollouts' run-to-run spread.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for players, rules in SHAPES:
        row = shape_row(args, players, rules)
        res["shapes"]["p%dd%d" % (players, row["displays"])] = row
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
