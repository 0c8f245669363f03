"""Agent steps/s of PolicyRollout(players=3 / 4) (PyTorch-GEMM network + azul_policy_head_n + azul_batch_mp_agent_step, HIP graph per window)
and the launch time of azul_batch_mp_agent_step alone at 4096 games.  One JSON line per configuration and opponent.

--opponent self: the opponent is a network of the policy's shape (a frozen past self): azul_batch_mp_net_* cuts, one opponent forward and
one host synchronisation per reply round, no HIP graph.  The line then also reports the reply rounds a step takes (max over the batch).

--fused-wide: the same run also measures PolicyRollout(fused_wide=True) (azul_batch_mp_policy_rollout: one launch per window) against the
GEMM path with opponent "random": agent steps/s of both, the window kernel's time from HIP events around each window (the returns scan behind
it included), and the share of the f32 matrix peak (157.3 TFLOP/s) that the FLOPs the shapes imply (2 (obs_size 360 + 180 num_actions + 180)
per agent step) reach over that kernel time.  With --opponent self (and --configs p2_d5x ...) it measures the network opponent instead:
PolicyRollout(fused_wide=True, fused_opponent=True) (azul_batch_mp_policy_rollout_vs: the reply rounds inside the window kernel) against the
per-cut path, both with a frozen copy of the policy as the opponent.

Usage: python tools/mp_rollout_bench.py [--games 4096] [--window 32] [--windows 20] [--hidden 180] [--opponent random self] [--configs p3_d5 ...]
                                        [--fused-wide]
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

CONFIGS = [
    ("p3_d5", 3, {"first_player": "Random", "tile_pool": "Lid"}),
    ("p4_d5", 4, {"first_player": "Random", "tile_pool": "Lid"}),
    ("p3_d7", 3, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}),
    ("p4_d9", 4, {"first_player": "Random", "tile_pool": "Lid", "displays": "2P+1"}),
]
# the extended-rule two-player shape: only on request (--configs p2_d5x)
EXTRA_CONFIGS = [("p2_d5x", 2, {"first_player": "Random", "tile_pool": "Lid", "bonuses": "end"})]


F32_MATRIX_PEAK = 157.3e12


def fused_rate(players, rules, args, opponent="random"):
    """(agent steps/s, median window kernel ms, FLOP per agent step, reply-round stats) of PolicyRollout(fused_wide=True); opponent "self":
    fused_opponent=True with a frozen copy of the policy (the FLOP then count the agent's forward only)."""
    probe = MultiplayerAzul(2, rules=rules, players=players)
    torch.manual_seed(0)
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, 180)
    opp = copy.deepcopy(pol) if opponent == "self" else "random"
    ro = PolicyRollout(pol, n_games=args.games, rules=rules, window=args.window, opponent=opp, players=players, fused_wide=True,
                       fused_opponent=opponent == "self")
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    ev, rounds = [], []
    t0 = time.perf_counter()
    for _ in range(args.windows):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(ro.streams[0])
        tr = ro.run_window()
        e.record(ro.streams[0])
        ev.append((s, e))
        if opponent == "self":
            rounds.append(tr[0]["opp_replies"].max(dim=1).values.float())
    ro.synchronize()
    dt = time.perf_counter() - t0
    ms = sorted(s.elapsed_time(e) for s, e in ev)[len(ev) // 2]
    flop = 2 * (probe.obs_size * 360 + 180 * probe.num_actions + 180)
    extra = {}
    if rounds:
        r = torch.cat(rounds)
        extra = {"replies_per_step_max_mean": round(float(r.mean()), 3), "replies_per_step_max": int(r.max())}
    return args.games * args.window * args.windows / dt, ms, flop, extra


def rollout_rate(players, rules, args, opponent):
    probe = MultiplayerAzul(2, rules=rules, players=players)
    torch.manual_seed(0)
    pol = BatchedActorCritic(probe.obs_size, probe.num_actions, args.hidden)
    opp = copy.deepcopy(pol) if opponent == "self" else "random"
    ro = PolicyRollout(pol, n_games=args.games, rules=rules, window=args.window, opponent=opp, players=players)
    for _ in range(3):
        ro.run_window()
    ro.synchronize()
    rounds = []
    t0 = time.perf_counter()
    for _ in range(args.windows):
        tr = ro.run_window()
        if opponent == "self":
            rounds.append(tr[0]["opp_replies"].max(dim=1).values.float())     # (device tensors: read after the timed region)
    ro.synchronize()
    dt = time.perf_counter() - t0
    extra = {}
    if rounds:
        r = torch.cat(rounds)
        extra = {"reply_rounds_per_step_mean": round(float(r.mean()), 3), "reply_rounds_per_step_max": int(r.max())}
    return args.games * args.window * args.windows / dt, ro.use_graph, extra


def launch_ms(players, rules, args):
    env = MultiplayerAzul(args.games, rules=rules, players=players, seed=1)
    env.runner_init()
    env.reset()
    d, n = env.device, env.n
    b = [torch.zeros(n, dtype=torch.int32, device=d), torch.zeros(n, dtype=torch.uint8, device=d), torch.zeros(n, dtype=torch.uint8, device=d),
         torch.zeros(n, env.obs_size, device=d), torch.zeros(n, env.num_actions, dtype=torch.uint8, device=d), torch.zeros(n, dtype=torch.uint8, device=d)]
    _, mask, _ = env.observe_all(0)
    b[4].copy_(mask)
    act = torch.zeros(n, dtype=torch.int32, device=d)
    times = []
    for i in range(60):
        act.copy_(b[4].float().argmax(dim=1).to(torch.int32))
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        env.agent_step(act, *b)
        e.record()
        e.synchronize()
        if i >= 10:
            times.append(s.elapsed_time(e))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--hidden", type=int, default=180)
    ap.add_argument("--opponent", nargs="+", choices=("random", "self"), default=["random"])
    ap.add_argument("--configs", nargs="+", choices=[c[0] for c in EXTRA_CONFIGS + CONFIGS], default=[c[0] for c in CONFIGS])
    ap.add_argument("--fused-wide", action="store_true")
    args = ap.parse_args()
    if args.fused_wide and "self" in args.opponent:
        for name, players, rules in EXTRA_CONFIGS + CONFIGS:
            if name not in args.configs:
                continue
            cut, _, cut_extra = rollout_rate(players, rules, args, "self")
            fused, ms, _, extra = fused_rate(players, rules, args, "self")
            print(json.dumps({"config": name, "opponent": "self", "games": args.games, "window": args.window, "hidden": 180,
                              "per_cut_agent_steps_per_s": round(cut), "fused_agent_steps_per_s": round(fused), "speedup": round(fused / cut, 2),
                              "fused_window_ms_median": round(ms, 4), "fused_kernel_agent_steps_per_s": round(args.games * args.window / (ms * 1e-3)),
                              "per_cut_reply_rounds_per_step_mean": cut_extra.get("reply_rounds_per_step_mean"), **extra}), flush=True)
        return
    if args.fused_wide:
        for name, players, rules in CONFIGS:
            if name not in args.configs:
                continue
            gemm, graph, _ = rollout_rate(players, rules, args, "random")
            fused, ms, flop, _ = fused_rate(players, rules, args)
            steps = args.games * args.window
            print(json.dumps({"config": name, "opponent": "random", "games": args.games, "window": args.window, "hidden": 180,
                              "gemm_agent_steps_per_s": round(gemm), "gemm_graph": graph, "fused_agent_steps_per_s": round(fused),
                              "speedup": round(fused / gemm, 2), "fused_window_ms_median": round(ms, 4),
                              "fused_kernel_agent_steps_per_s": round(steps / (ms * 1e-3)), "flop_per_agent_step": flop,
                              "f32_matrix_peak_share": round(flop * steps / (ms * 1e-3) / F32_MATRIX_PEAK, 4)}), flush=True)
        return
    for name, players, rules in CONFIGS:
        if name not in args.configs:
            continue
        ms = launch_ms(players, rules, args)
        for opponent in args.opponent:
            rate, graph, extra = rollout_rate(players, rules, args, opponent)
            print(json.dumps({"config": name, "opponent": opponent, "games": args.games, "window": args.window, "hidden": args.hidden,
                              "graph": graph, "agent_steps_per_s": round(rate), "mp_agent_step_launch_ms_median": round(ms, 4), **extra}),
                  flush=True)


if __name__ == "__main__":
    main()
