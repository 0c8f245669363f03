"""azul_batch_mp_score_moves and the greedy seats of wide batches at 4096 games, for the five compiled shapes (players, displays) = (2, 5),
(3, 5), (3, 7), (4, 5), (4, 9), all measured in ONE process, written to profiles/mp_score_moves_bench.json:

  * ms per score_moves launch (the [N][num_actions] table + best) and per greedy_action launch (best only) on MID-GAME states -- a seeded
    batch after `--advance` flat self-play moves -- beside ms per azul_batch_legal_mask launch on the same states: HIP events around
    each launch, the three kinds interleaved, medians after 20 warm-up rounds;
  * agent steps/s of PolicyRollout(players=P, opponent="greedy_margin") beside the per-cut network opponent (opponent=<a copy of the
    policy>, hidden 180) on the same shape: both one launch per cut of the protocol and one host synchronisation per reply round; wall
    clock over `--windows` windows after three warm-up windows, the two opponents alternating `--repeats` times (median and spread),
    plus the reply rounds per agent step (max over the batch) of both.

Usage: python tools/mp_score_moves_bench.py [--games 4096] [--advance 40] [--launches 200] [--window 32] [--windows 24] [--repeats 3] [--out FILE]
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

from azul_deep_reinforcement_learning_amd import BatchedActorCritic, MultiplayerAzul, PolicyRollout  # noqa: E402
from azul_deep_reinforcement_learning_amd import _lib as L  # noqa: E402

EXT = {"displays": "2P+1", "bonuses": "end", "short_deal": True}
SHAPES = [(2, {"first_player": "Random", "tile_pool": "Lid", "bonuses": "end"}), (3, {"first_player": "Random", "tile_pool": "Lid"}),
          (3, dict({"first_player": "Random", "tile_pool": "Lid"}, **EXT)), (4, {"first_player": 1, "tile_pool": "Random"}),
          (4, dict({"first_player": "Random", "tile_pool": "Lid"}, **EXT))]


def launch_times(args, players, rules):
    env = MultiplayerAzul(args.games, rules=rules, players=players, device="cuda", seed=1)
    env.init()
    env.new_round()
    env.selfplay(args.advance)
    torch.cuda.synchronize()
    n, NA = env.n, env.num_actions
    scores = torch.empty(n, NA, dtype=torch.int32, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    mask = torch.empty(n, NA, dtype=torch.uint8, device="cuda")
    kinds = {"score_moves": lambda: env.score_moves(L.PERSP_MOVER, scores=scores, best=best),
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
    return out, env.obs_size, NA


def rollout_rates(args, players, rules, n_obs, n_act):
    """The two opponents on rollouts of their own, timed in turn `repeats` times."""
    torch.manual_seed(0)
    pol = BatchedActorCritic(n_obs, n_act, 180)
    ros = {"greedy_margin": PolicyRollout(pol, n_games=args.games, window=args.window, opponent="greedy_margin", players=players, rules=rules),
           "net_per_cut": PolicyRollout(pol, n_games=args.games, window=args.window, opponent=copy.deepcopy(pol), players=players, rules=rules)}
    rates, rounds = {k: [] for k in ros}, {k: [] for k in ros}
    for ro in ros.values():
        assert ro.cut and not ro.fused_wide and not ro.use_graph
        for _ in range(3):
            ro.run_window()
        ro.synchronize()
    for _ in range(args.repeats):
        for k, ro in ros.items():
            t0 = time.perf_counter()
            for _ in range(args.windows):
                tr = ro.run_window()
                rounds[k].append(tr[0]["opp_replies"].max(dim=1).values.float())
            ro.synchronize()
            rates[k].append(args.games * args.window * args.windows / (time.perf_counter() - t0))
    out = {}
    for k in ros:
        r = torch.cat(rounds[k])
        out["rollout_" + k] = {"agent_steps_per_s_median": round(sorted(rates[k])[len(rates[k]) // 2]),
                               "agent_steps_per_s_min": round(min(rates[k])), "agent_steps_per_s_max": round(max(rates[k])),
                               "reply_rounds_per_step_mean": round(float(r.mean()), 3), "reply_rounds_per_step_max": int(r.max())}
    g, nt = out["rollout_greedy_margin"], out["rollout_net_per_cut"]
    out["greedy_margin_over_net_per_reply_round"] = round(
        (g["agent_steps_per_s_median"] * (1.0 + g["reply_rounds_per_step_mean"])) / (nt["agent_steps_per_s_median"] * (1.0 + nt["reply_rounds_per_step_mean"])), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--advance", type=int, default=40)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp_score_moves_bench.json"))
    args = ap.parse_args()
    res = {"tool": "python tools/mp_score_moves_bench.py --games %d --advance %d --launches %d --window %d --windows %d --repeats %d"
                   % (args.games, args.advance, args.launches, args.window, args.windows, args.repeats),
           "note": "one process. Launch times: HIP events around single launches on the same mid-game states (a seeded batch after --advance flat "
                   "self-play moves), the three kinds interleaved. Rollouts: PolicyRollout agent steps/s, wall clock, both on the per-cut protocol "
                   "(one launch per cut, one host synchronisation per reply round), timed in turn: a greedy seat answers a round with one "
                   "azul_batch_mp_score_moves launch, the network opponent (a copy of the policy) with two GEMMs and one azul_policy_head_n launch. "
                   "The two opponents play different games, so their reply rounds per agent step differ: greedy_margin_over_net_per_reply_round "
                   "compares launches of the protocol per second, (1 + reply rounds per step) * agent steps/s.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for players, rules in SHAPES:
        launches, n_obs, n_act = launch_times(args, players, rules)
        row = {"players": players, "displays": n_act // 30 - 1, "num_actions": n_act, "rules": rules, "launches": launches}
        row.update(rollout_rates(args, players, rules, n_obs, n_act))
        res["shapes"]["p%dd%d" % (players, n_act // 30 - 1)] = row
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
