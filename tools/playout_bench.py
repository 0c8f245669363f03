"""azul_batch_playout_moves and the playout opponent at 4096 games, all measured in ONE process, written to profiles/playout_moves_bench.json:

  * ms per playout_moves launch (the [N][180] table + best) for K = 1, 4, 16 playouts per move on MID-GAME states -- a seeded batch after
    `--advance` flat self-play moves, as in tools/score_moves_bench.py -- interleaved with score_moves and legal_mask launches on the same
    states: HIP events around each launch, median and minimum;
  * playout plies per second: the plies the HOST MODEL (tests/playout_moves_model.py, the same draws) plays for the first `--sample` games
    of that batch -- candidate moves and playout moves -- scaled to the batch and divided by the median launch time; beside the flat
    self-play kernel's env steps/s (HIP events around `--selfplay-steps`-move launches of the same process);
  * agent steps/s of PolicyRollout(opponent="playout", opponent_playouts=8) beside opponent="greedy": wall clock over `--windows` windows
    after two warm-up windows;
  * strength: the playout player (K = 8) head to head against greedy_action and against random_action, `--episodes` finished episodes
    each.  Both seats are played from outside through Azul.step for every game (BatchedAzul.azul_step -- BatchedAzul.step is
    GameRunner.step, whose RandomAgent would answer inside), the playout player's seat alternating by game and by episode.  A game whose
    mover has nothing legal, or that exceeds `--move-cap` moves, is restarted and counted apart.  Win rate = wins / episodes with its
    binomial standard error; draws are listed.

Usage: python tools/playout_bench.py [--games 4096] [--advance 40] [--launches 100] [--sample 64] [--window 32] [--windows 3]
                                     [--episodes 2000] [--arena-games 1024] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from azul_deep_reinforcement_learning_amd import BatchedActorCritic, BatchedAzul, PolicyRollout  # noqa: E402
from azul_deep_reinforcement_learning_amd import _lib as L  # noqa: E402

KS = (1, 4, 16)
SEED, CALL = 0xB16B00B5, 3


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def launch_times(args):
    env = BatchedAzul(args.games, device="cuda", seed=1)
    env.runner_init()
    env.runner_init()
    traj = env.alloc_trajectory(args.advance)
    env.selfplay(args.advance, traj["mask"], traj["action"], traj["reward"], traj["done"])
    torch.cuda.synchronize()
    n = env.n
    table = torch.empty(n, L.NUM_ACTIONS, dtype=torch.int32, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    mask = torch.empty(n, L.NUM_ACTIONS, dtype=torch.uint8, device="cuda")
    kinds = {"playout_moves_k%d" % k: (lambda k=k: env.playout_moves(k, SEED, CALL, sums=table, best=best)) for k in KS}
    kinds["score_moves"] = lambda: env.score_moves(L.PERSP_CURRENT, scores=table, best=best)
    kinds["legal_mask"] = lambda: env.get_valid_moves(out=mask)
    times = {k: [] for k in kinds}
    for i in range(args.launches + 10):
        for k, fn in kinds.items():
            t = _timed(fn)
            if i >= 10:
                times[k].append(t)
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = {"launch_ms_median": round(v[len(v) // 2], 5), "launch_ms_min": round(v[0], 5), "launch_ms_p90": round(v[(9 * len(v)) // 10], 5),
                  "launches": len(v)}
    legal = mask.sum(dim=1).float()
    out.update(legal_moves_per_state_mean=round(float(legal.mean()), 2), states_without_a_legal_move=int((legal == 0).sum()))
    # the plies of a launch, from the host model on the first games of the batch (global ids 0 ..: the batch's id_base is 0)
    from tests import playout_moves_model as pm
    recs = env.get_records(0, args.sample)
    for k in KS:
        plies = 0
        for g in range(args.sample):
            rec = np.frombuffer(recs[g].tobytes(), np.uint8)
            _, legal_g, facts = pm.state_values(rec, g, SEED, CALL, k)
            plies += sum(f["plies"] + 1 for _, f in facts)         # the candidate's own move and the playout's
        per_launch = plies * (n / args.sample)
        d = out["playout_moves_k%d" % k]
        d["sample_plies"] = plies
        d["plies_per_launch_scaled"] = round(per_launch)
        d["plies_per_s_at_median"] = round(per_launch / (d["launch_ms_median"] * 1e-3))
    # the flat self-play kernel in the same process
    sp = env.alloc_trajectory(args.selfplay_steps)
    run = lambda: env.selfplay(args.selfplay_steps, sp["mask"], sp["action"], sp["reward"], sp["done"])
    run()
    torch.cuda.synchronize()
    ms = sorted(_timed(run) for _ in range(5))
    out["selfplay"] = {"steps_per_launch": args.selfplay_steps, "launch_ms_median": round(ms[2], 4), "launch_ms_min": round(ms[0], 4),
                       "env_steps_per_s_at_median": round(n * args.selfplay_steps / (ms[2] * 1e-3))}
    return out


def rollout_rate(args, opponent):
    torch.manual_seed(0)
    pol = BatchedActorCritic(136, 180, 180)
    kw = {"opponent_playouts": 8} if opponent == "playout" else {}
    ro = PolicyRollout(pol, n_games=args.games, window=args.window, opponent=opponent, persistent=False, **kw)
    assert not ro.persistent and not ro.use_graph
    for _ in range(2):
        ro.run_window()
    ro.synchronize()
    rounds, rates = [], []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        tr = ro.run_window()
        ro.synchronize()
        rates.append(args.games * args.window / (time.perf_counter() - t0))
        rounds.append(tr[0]["opp_replies"].max(dim=1).values.float())
    r = torch.cat(rounds)
    rates.sort()
    return {"agent_steps_per_s_median": round(rates[len(rates) // 2]), "agent_steps_per_s_min": round(rates[0]), "agent_steps_per_s_max": round(rates[-1]),
            "windows": args.windows, "reply_rounds_per_step_mean": round(float(r.mean()), 3), "reply_rounds_per_step_max": int(r.max())}


def head_to_head(args, other):
    """The playout player (K = 8) against `other` ("greedy" | "random") until args.episodes episodes have finished."""
    n = args.arena_games
    env = BatchedAzul(n, device="cuda", seed=7000 if other == "greedy" else 9000)
    env.runner_init()
    dev = env.device
    idx = torch.arange(n, device=dev)
    played = torch.zeros(n, dtype=torch.int64, device=dev)         # episodes finished or abandoned per game: the playout seat alternates with it
    moves = torch.zeros(n, dtype=torch.int64, device=dev)
    wins = losses = draws = stuck = capped = 0
    margin = 0
    call = 0
    while wins + losses + draws < args.episodes:
        recs = env.get_records()
        mover = torch.from_numpy((recs["flags"] & 7).astype(np.int64) - 1).to(dev)
        seat = (idx + played) & 1                                  # the playout player's seat in this episode
        mine = (mover == seat).to(torch.uint8)
        act = env.greedy_action(active=1 - mine) if other == "greedy" else env.random_action(active=1 - mine)
        env.playout_action(8, SEED + 1, call, active=mine, out=act)
        call += 1
        nothing = act < 0
        env.azul_step(torch.where(nothing, torch.zeros_like(act), act), active=(~nothing).to(torch.uint8))
        moves += 1
        over = env.is_end_of_game()
        cut = (nothing | (moves > args.move_cap)) & ~over
        if bool(over.any()) or bool(cut.any()):
            sc = torch.from_numpy(env.get_records()["score"].astype(np.int64)).to(dev)
            d = torch.where(seat == 0, sc[:, 0] - sc[:, 1], sc[:, 1] - sc[:, 0])[over]
            wins, losses, draws = wins + int((d > 0).sum()), losses + int((d < 0).sum()), draws + int((d == 0).sum())
            margin += int(d.sum())
            stuck += int((nothing & ~over).sum())
            capped += int((cut & ~nothing).sum())
            again = over | cut
            env.runner_init(active=again.to(torch.uint8))
            played += again.to(torch.int64)
            moves[again] = 0
    ep = wins + losses + draws
    p = wins / ep
    return {"opponent": other, "episodes": ep, "wins": wins, "losses": losses, "draws": draws, "win_rate": round(p, 4),
            "win_rate_standard_error": round(math.sqrt(p * (1 - p) / ep), 4), "mean_score_margin": round(margin / ep, 3),
            "restarted_nothing_legal": stuck, "restarted_move_cap": capped, "games": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--advance", type=int, default=40)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--selfplay-steps", type=int, default=512)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--arena-games", type=int, default=1024)
    ap.add_argument("--move-cap", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_moves_bench.json"))
    args = ap.parse_args()
    res = {"tool": "python tools/playout_bench.py --games %d --advance %d --launches %d --sample %d --selfplay-steps %d --window %d --windows %d "
                   "--episodes %d --arena-games %d --move-cap %d" % (args.games, args.advance, args.launches, args.sample, args.selfplay_steps,
                                                                     args.window, args.windows, args.episodes, args.arena_games, args.move_cap),
           "note": "one process. Launch times: HIP events around single launches on the same mid-game states (a seeded batch after --advance flat "
                   "self-play moves), the kinds interleaved. Plies: the host model's count (candidate move + playout moves) for the first --sample "
                   "games at the launch's own seed and call, scaled by games / sample. Rollouts: PolicyRollout agent steps/s per window, wall "
                   "clock, both on the per-cut protocol. Strength: both seats played from outside through Azul.step for every game, the "
                   "playout player's seat alternating; win rate = wins / finished episodes, draws listed.",
           "games": args.games, "window": args.window, "device": torch.cuda.get_device_name(0)}
    res["launches"] = launch_times(args)
    res["rollout_playout_k8"] = rollout_rate(args, "playout")
    res["rollout_greedy"] = rollout_rate(args, "greedy")
    res["strength_k8"] = [head_to_head(args, "greedy"), head_to_head(args, "random")]
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
