"""The arena inside the window kernels at 4096 games and window 32, beside the single network opponent and the league it generalises -- per
batch shape five rollouts measured in ONE process, written to profiles/arena_rollout_bench.json:

  * vs          PolicyRollout(opponent=<module>): azul_batch_policy_rollout_vs / azul_batch_mp_policy_rollout_vs;
  * league_k4   PolicyRollout(opponent=[4 modules]): the league entries, group i -> member i % 4;
  * arena_k1    Arena([module]): every group plays (0, 0) -- the memory traffic of vs with one weight set serving both seats;
  * arena_k4, arena_k16   pools of 4 and 16 distinct nets on round 0 of the round-robin schedule (round_robin_pairs over the 256 groups:
                all 12 ordered pairs of 4, 240 ordered pairs of 16): K x ~330 KB of weights meet a 4 MiB L2 per XCD, read for both seats.

Shapes: the two-player reference batch (ActorCritic(136, 180, 180)) and three players on five displays (ActorCritic(188, 180, 180)).
Agent steps/s: wall clock over a number of windows that ends in a device synchronisation, after three warm-up windows
(tools/league_rollout_bench.py's conventions); `--repeats` such measurements per rollout, the rollouts alternating; the median is reported
beside every repeat, and `spread` is (max - min) / median of the repeats.  No speed is promised: the file says what was measured.

--baseline-only measures `vs` and `league_k4` alone, through nothing but PolicyRollout: the tool then also runs on a checkout of the commit
before the arena.  Hand the files such runs wrote to --parent (their repeats are pooled) and they are recorded as `parent_vs` /
`parent_league_k4` next to this tree's own numbers; --merge FILE takes this tree's numbers from a file an earlier run wrote instead of
measuring (no device needed), so that the parent can be measured before AND after this tree in one job.

Usage: python tools/arena_rollout_bench.py [--games 4096] [--window 32] [--windows 200] [--repeats 5] [--baseline-only] [--parent FILE ...]
                                           [--merge FILE] [--out FILE]
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

SHAPES = {"two_player": dict(players=2, obs=136, act=180, switches=dict(persistent=True)),
          "p3_d5": dict(players=3, obs=188, act=180, switches=dict(fused_wide=True, fused_opponent=True))}
BASELINES = {"vs": None, "league_k4": 4}
ARENAS = {"arena_k1": 1, "arena_k4": 4, "arena_k16": 16}


def make(args, shape, kind):
    sh = SHAPES[shape]
    torch.manual_seed(0)
    net = lambda: BatchedActorCritic(sh["obs"], sh["act"], 180)
    if kind in BASELINES:
        policy, pool = net(), BASELINES[kind]
        opponent = net() if pool is None else [net() for _ in range(pool)]
        ro = PolicyRollout(policy, n_games=args.games, window=args.window, players=sh["players"], opponent=opponent, use_graph=False,
                           **sh["switches"])
        assert ro.window_entry is not None and ro.window_entry.endswith("_vs" if pool is None else "_league"), ro.window_entry
    else:
        from azul_deep_reinforcement_learning_amd import Arena
        ro = Arena([net() for _ in range(ARENAS[kind])], n_games=args.games, window=args.window, players=sh["players"])
        assert ro.arena_entry.endswith("_arena")
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    return ro


def timed(ro, windows):
    ro.synchronize()
    t0 = time.perf_counter()
    for _ in range(windows):
        ro.run_window()
    ro.synchronize()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return ro.n * ro.T * windows / dt


def summary(rates, windows, games, window):
    med = sorted(rates)[len(rates) // 2]
    return {"agent_steps_per_s": med, "repeats": rates, "spread": round((max(rates) - min(rates)) / med, 4), "windows_timed": windows,
            "us_per_window": round(games * window / med * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_rollout_bench.json"))
    args = ap.parse_args()
    assert args.merge or torch.cuda.is_available(), "the rates are the MI355X's: no device, no measurement"
    res = json.load(open(args.merge)) if args.merge else \
          {"tool": "python tools/arena_rollout_bench.py --games %d --window %d --windows %d --repeats %d%s"
                   % (args.games, args.window, args.windows, args.repeats, " --baseline-only" if args.baseline_only else ""),
           "note": "one process; agent steps/s, wall clock over the timed windows ending in a device synchronisation, three warm-up windows; the "
                   "rollouts alternate, `repeats` holds every measurement, agent_steps_per_s their median, spread = (max - min) / median. vs: "
                   "one opponent net; league_k4: a pool of 4 opponents, group i -> member i % 4; arena_kK: K distinct nets in both seats, round "
                   "0 of round_robin_pairs over the groups (K = 1: every group (0, 0)). parent_*: the same rollout measured by --baseline-only on "
                   "a checkout of the commit before the arena, in processes of their own before and after this tree's in the same job.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0)}
    kinds = list(BASELINES) if args.baseline_only else list(BASELINES) + list(ARENAS)
    for shape in SHAPES if not args.merge else []:
        ros = {k: make(args, shape, k) for k in kinds}
        rates = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for k, ro in ros.items():
                rates[k].append(round(timed(ro, args.windows)))
        res[shape] = {k: summary(rates[k], args.windows, args.games, args.window) for k in kinds}
        del ros
        torch.cuda.empty_cache()
    parents = [json.load(open(f)) for f in args.parent]
    for shape in SHAPES if parents else []:
        row = res[shape]
        for k in BASELINES:
            pooled = [r for p in parents for r in p[shape][k]["repeats"]]
            row["parent_" + k] = summary(pooled, parents[0][shape][k]["windows_timed"], args.games, args.window)
            row["%s_over_parent_%s" % (k, k)] = round(row[k]["agent_steps_per_s"] / row["parent_" + k]["agent_steps_per_s"], 4)
            row["%s_within_spread_of_parent_%s" % (k, k)] = bool(abs(row["%s_over_parent_%s" % (k, k)] - 1.0) <=
                                                                 max(row[k]["spread"], row["parent_" + k]["spread"]))
        for k in ARENAS:
            row[k + "_over_vs"] = round(row[k]["agent_steps_per_s"] / row["vs"]["agent_steps_per_s"], 4)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
