"""The greedy opponent inside the two-player window kernel at 4096 games and window 32, beside the per-cut path it replaces and the
RandomAgent window kernel it cannot beat -- three PolicyRollouts measured in ONE process, written to profiles/greedy_rollout_bench.json:

  * greedy_per_cut   opponent="greedy": one azul_batch_score_moves launch, one azul_batch_net_step_reply launch and one host
                     synchronisation per reply round (the path of tools/score_moves_bench.py, re-measured here);
  * greedy_fused     the same with fused_opponent=True: azul_batch_policy_rollout_greedy, one launch per window;
  * random_fused     opponent="random", persistent=True: azul_policy_rollout2_kernel<LID, 1>, the floor of the window kernel.

Agent steps/s: wall clock over a number of windows that ends in a device synchronisation, after three warm-up windows
(tools/score_moves_bench.py's conventions); `--repeats` such measurements per rollout, the three rollouts alternating, the median
reported beside every repeat.  Reply rounds per agent step from the recorded opp_replies: per step the maximum over the batch (the
reply rounds the per-cut path launches), over the two games of a wave (the passes of the window kernel's reply loop) and the mean over
the games (the opponent moves themselves).

Usage: python tools/greedy_rollout_bench.py [--games 4096] [--window 32] [--windows 400] [--per-cut-windows 20] [--repeats 3] [--out FILE]
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

KINDS = {"greedy_per_cut": dict(opponent="greedy"), "greedy_fused": dict(opponent="greedy", fused_opponent=True),
         "random_fused": dict(opponent="random", persistent=True)}


def make(args, kind):
    torch.manual_seed(0)
    ro = PolicyRollout(BatchedActorCritic(136, 180, 180), n_games=args.games, window=args.window, **KINDS[kind])
    assert ro.persistent == (kind != "greedy_per_cut") and not ro.use_graph
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    return ro


def timed(ro, windows):
    """-> (agent steps/s, the windows' opp_replies [windows * T][N] or None)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=400)
    ap.add_argument("--per-cut-windows", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_rollout_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the rates are the MI355X's: no device, no measurement"
    res = {"tool": "python tools/greedy_rollout_bench.py --games %d --window %d --windows %d --per-cut-windows %d --repeats %d"
                   % (args.games, args.window, args.windows, args.per_cut_windows, args.repeats),
           "note": "one process; PolicyRollout agent steps/s, wall clock over the timed windows ending in a device synchronisation, three warm-up "
                   "windows; the three rollouts alternate, `repeats` holds every measurement and agent_steps_per_s their median. greedy_per_cut: "
                   "one score_moves launch + one net_step_reply launch + one host synchronisation per reply round; greedy_fused: "
                   "azul_batch_policy_rollout_greedy, one launch per window; random_fused: azul_batch_policy_rollout with the RandomAgent.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0)}
    ros = {k: make(args, k) for k in KINDS}
    rates, reps = {k: [] for k in KINDS}, {}
    for _ in range(args.repeats):
        for k, ro in ros.items():
            rate, rep = timed(ro, args.per_cut_windows if k == "greedy_per_cut" else args.windows)
            rates[k].append(round(rate))
            if rep is not None:
                reps[k] = rep
    for k in KINDS:
        res[k] = {"agent_steps_per_s": sorted(rates[k])[len(rates[k]) // 2], "repeats": rates[k],
                  "windows_timed": args.per_cut_windows if k == "greedy_per_cut" else args.windows}
        res[k]["us_per_window"] = round(args.games * args.window / res[k]["agent_steps_per_s"] * 1e6, 1)
        if k in reps:
            res[k].update(rounds(reps[k]))
    res["fused_over_per_cut"] = round(res["greedy_fused"]["agent_steps_per_s"] / res["greedy_per_cut"]["agent_steps_per_s"], 2)
    res["fused_over_random_fused"] = round(res["greedy_fused"]["agent_steps_per_s"] / res["random_fused"]["agent_steps_per_s"], 3)
    res["acceptance"] = {"floor": "greedy_fused >= 2 x greedy_per_cut of the same run", "met": res["fused_over_per_cut"] >= 2.0}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
