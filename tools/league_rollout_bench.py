"""The league inside the window kernels at 4096 games and window 32, beside the single network opponent it generalises -- per batch shape
four PolicyRollouts measured in ONE process, written to profiles/league_rollout_bench.json:

  * vs          opponent=<module>: azul_batch_policy_rollout_vs / azul_batch_mp_policy_rollout_vs, one weight set for every workgroup;
  * league_k1   opponent=[module]: the league entries with a pool of one (the same memory traffic as vs, plus the member read);
  * league_k4, league_k16   pools of 4 and 16 distinct nets, groups dealt round-robin (group i -> member i % K): K x ~330 KB of opponent
                weights meet a 4 MiB L2 per XCD, and the workgroups of one XCD play all K members.

Shapes: the two-player reference batch (ActorCritic(136, 180, 180), persistent=True) and three players on five displays
(ActorCritic(188, 180, 180), fused_wide=True, fused_opponent=True).  Agent steps/s: wall clock over a number of windows that ends in a
device synchronisation, after three warm-up windows (tools/greedy_rollout_bench.py's conventions); `--repeats` such measurements per
rollout, the rollouts alternating; the median is reported beside every repeat, and `spread` is (max - min) / median of the repeats.

--vs-only measures `vs` alone through nothing but PolicyRollout(opponent=<module>): the tool then also runs on a checkout of the commit
before the league.  Hand the file such a run wrote to --parent-vs (several files: their repeats are pooled) and it is recorded as
`parent_vs` next to this tree's own numbers; --merge FILE takes this tree's numbers from a file an earlier run wrote instead of
measuring (no device needed), so that the parent can be measured before AND after this tree in one job.

Usage: python tools/league_rollout_bench.py [--games 4096] [--window 32] [--windows 200] [--repeats 5] [--vs-only] [--parent-vs FILE ...]
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
POOLS = {"league_k1": 1, "league_k4": 4, "league_k16": 16}


def make(args, shape, pool):
    """pool None: the single opponent; K: a league of K distinct nets."""
    sh = SHAPES[shape]
    torch.manual_seed(0)
    net = lambda: BatchedActorCritic(sh["obs"], sh["act"], 180)
    policy = net()
    opponent = net() if pool is None else [net() for _ in range(pool)]
    ro = PolicyRollout(policy, n_games=args.games, window=args.window, players=sh["players"], opponent=opponent, use_graph=False, **sh["switches"])
    assert ro.window_entry is not None and ro.window_entry.endswith("_vs" if pool is None else "_league"), ro.window_entry
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
    ap.add_argument("--vs-only", action="store_true")
    ap.add_argument("--parent-vs", nargs="*", default=[])
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "league_rollout_bench.json"))
    args = ap.parse_args()
    assert args.merge or torch.cuda.is_available(), "the rates are the MI355X's: no device, no measurement"
    res = json.load(open(args.merge)) if args.merge else \
          {"tool": "python tools/league_rollout_bench.py --games %d --window %d --windows %d --repeats %d%s"
                   % (args.games, args.window, args.windows, args.repeats, " --vs-only" if args.vs_only else ""),
           "note": "one process; PolicyRollout agent steps/s, wall clock over the timed windows ending in a device synchronisation, three warm-up "
                   "windows; the rollouts alternate, `repeats` holds every measurement, agent_steps_per_s their median, spread = (max - min) / "
                   "median. vs: one opponent net; league_kK: a pool of K distinct nets, group i -> member i % K. parent_vs: `vs` measured by "
                   "--vs-only on a checkout of the commit before the league, in a process of its own in the same job.",
           "games": args.games, "window": args.window, "hidden": 180, "device": torch.cuda.get_device_name(0)}
    kinds = {"vs": None} if args.vs_only else dict({"vs": None}, **POOLS)
    for shape in SHAPES if not args.merge else []:
        ros = {k: make(args, shape, pool) for k, pool in kinds.items()}
        rates = {k: [] for k in kinds}
        for _ in range(args.repeats):
            for k, ro in ros.items():
                rates[k].append(round(timed(ro, args.windows)))
        res[shape] = {k: summary(rates[k], args.windows, args.games, args.window) for k in kinds}
        del ros
        torch.cuda.empty_cache()
    parents = [json.load(open(f)) for f in args.parent_vs]
    for shape in SHAPES if parents else []:
        pooled = [r for p in parents for r in p[shape]["vs"]["repeats"]]
        row = res[shape]
        row["parent_vs"] = summary(pooled, parents[0][shape]["vs"]["windows_timed"], args.games, args.window)
        vs, pv, k1 = row["vs"], row["parent_vs"], row["league_k1"]
        row["vs_over_parent_vs"] = round(vs["agent_steps_per_s"] / pv["agent_steps_per_s"], 4)
        row["league_k1_over_vs"] = round(k1["agent_steps_per_s"] / vs["agent_steps_per_s"], 4)
        row["league_k4_over_vs"] = round(row["league_k4"]["agent_steps_per_s"] / vs["agent_steps_per_s"], 4)
        row["league_k16_over_vs"] = round(row["league_k16"]["agent_steps_per_s"] / vs["agent_steps_per_s"], 4)
        # the one expectation: vs within the repeats' spread of parent_vs, league_k1 within the spread of vs
        row["vs_within_spread_of_parent_vs"] = bool(abs(row["vs_over_parent_vs"] - 1.0) <= max(vs["spread"], pv["spread"]))
        row["league_k1_within_spread_of_vs"] = bool(abs(row["league_k1_over_vs"] - 1.0) <= max(vs["spread"], k1["spread"]))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
