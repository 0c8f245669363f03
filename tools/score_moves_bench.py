"""azul_batch_score_moves and the greedy opponent at 4096 games, all measured in ONE process, written to profiles/score_moves_bench.json:

  * ms per score_moves launch (the [N][180] table + best) and per greedy_action launch (best only) on MID-GAME states -- a seeded batch
    after `--advance` flat self-play moves -- beside ms per azul_batch_legal_mask launch on the same states: HIP events around each
    launch, the three kinds interleaved, medians;
  * agent steps/s of PolicyRollout(opponent="greedy") beside the two-player per-cut network-opponent path (opponent=<a copy of the
    policy>, persistent=False): both one launch per cut of the protocol and one host synchronisation per reply round; wall clock over
    `--windows` windows after three warm-up windows, plus the reply rounds per agent step (max over the batch).

Usage: python tools/score_moves_bench.py [--games 4096] [--advance 40] [--launches 200] [--window 32] [--windows 6] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from azul_deep_reinforcement_learning_amd import BatchedActorCritic, BatchedAzul, PolicyRollout  # noqa: E402
from azul_deep_reinforcement_learning_amd import _lib as L  # noqa: E402


def launch_times(args):
    env = BatchedAzul(args.games, device="cuda", seed=1)
    env.runner_init()
    env.runner_init()
    traj = env.alloc_trajectory(args.advance)
    env.selfplay(args.advance, traj["mask"], traj["action"], traj["reward"], traj["done"])
    torch.cuda.synchronize()
    n = env.n
    scores = torch.empty(n, L.NUM_ACTIONS, dtype=torch.int32, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    mask = torch.empty(n, L.NUM_ACTIONS, dtype=torch.uint8, device="cuda")
    kinds = {"score_moves": lambda: env.score_moves(L.PERSP_CURRENT, scores=scores, best=best),
             "greedy_action": lambda: env.greedy_action(out=best),
             "legal_mask": lambda: env.get_valid_moves(out=mask)}
    times = {k: [] for k in kinds}
    for i in range(args.launches + 20):
        for k, fn in kinds.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            if i >= 20:
                times[k].append(s.elapsed_time(e))
    legal = mask.sum(dim=1).float()
    out = {k + "_launch_ms_median": round(sorted(v)[len(v) // 2], 5) for k, v in times.items()}
    out.update({k + "_launch_ms_min": round(min(v), 5) for k, v in times.items()})
    out.update(legal_moves_per_state_mean=round(float(legal.mean()), 2), states_without_a_legal_move=int((legal == 0).sum()))
    return out


def rollout_rate(args, opponent):
    torch.manual_seed(0)
    pol = BatchedActorCritic(136, 180, 180)
    opp = copy.deepcopy(pol) if opponent == "net" else "greedy"
    ro = PolicyRollout(pol, n_games=args.games, window=args.window, opponent=opp, persistent=False)
    assert not ro.persistent and not ro.use_graph
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    rounds = []
    t0 = time.perf_counter()
    for _ in range(args.windows):
        tr = ro.run_window()
        rounds.append(tr[0]["opp_replies"].max(dim=1).values.float())
    ro.synchronize()
    dt = time.perf_counter() - t0
    r = torch.cat(rounds)
    return {"agent_steps_per_s": round(args.games * args.window * args.windows / dt),
            "reply_rounds_per_step_mean": round(float(r.mean()), 3), "reply_rounds_per_step_max": int(r.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--advance", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_moves_bench.json"))
    args = ap.parse_args()
    res = {"tool": "python tools/score_moves_bench.py --games %d --advance %d --launches %d --window %d --windows %d"
                   % (args.games, args.advance, args.launches, args.window, args.windows),
           "note": "one process. Launch times: HIP events around single launches on the same mid-game states (a seeded batch after --advance flat "
                   "self-play moves), the three kinds interleaved. Rollouts: PolicyRollout agent steps/s, wall clock, both on the per-cut protocol "
                   "(one launch per cut, one host synchronisation per reply round): the greedy opponent answers a round with one "
                   "azul_batch_score_moves launch, the network opponent (a copy of the policy, persistent=False) with one azul_policy_forward launch.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0)}
    res["launches"] = launch_times(args)
    res["rollout_greedy"] = rollout_rate(args, "greedy")
    res["rollout_net_per_cut"] = rollout_rate(args, "net")
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
