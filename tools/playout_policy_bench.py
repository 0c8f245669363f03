"""azul_batch_playout_moves_policy and the greedy-playout opponent at 4096 games, all measured in ONE process, written to
profiles/playout_policy_bench.json (tools/playout_bench.py's method: HIP events around single launches on MID-GAME states -- a seeded batch
after `--advance` flat self-play moves -- 100 launches after 10 warm-ups, the kinds interleaved; median, minimum, p90):

  * launch time of the greedy policy at (explore 0, K 1), (64, 4) and (64, 16) beside the uniform policy at K = 1, 8, 16, score_moves and
    legal_mask;
  * the uniform kernel against the PARENT commit's library (`--parent-lib`: a libazulhip.so built from the parent's sources with the same
    flags, loaded beside the package's own; its batch holds the same records): azul_batch_playout_moves at K = 1, 4, 16 through both
    libraries, interleaved; the difference of the medians beside the spread (p90 - median) of the parent's own repeats;
  * agent steps/s of PolicyRollout against the greedy-playout opponent at (0, 1), beside the uniform K = 8 opponent and opponent="greedy";
  * strength, head to head as tools/playout_bench.py plays it (both seats through Azul.step, seats alternating by game and episode,
    `--episodes` finished episodes per pairing): greedy-playout (0, 1) against greedy_action, against the uniform K = 8 playout player and
    against random_action, and (64, 4) against greedy_action.

Usage: python tools/playout_policy_bench.py [--parent-lib FILE] [--games 4096] [--episodes 2000] [--only launches,parent,rollouts,strength] [--out FILE]
"""
import argparse
import ctypes as C
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
from azul_deep_reinforcement_learning_amd.batch import parse_rules  # noqa: E402

SEED, CALL = 0xB16B00B5, 3
GREEDY_KINDS = ((0, 1), (64, 4), (64, 16))
UNIFORM_KS = (1, 8, 16)
PARENT_KS = (1, 4, 16)


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _interleaved(kinds, launches):
    times = {k: [] for k in kinds}
    for i in range(launches + 10):
        for k, fn in kinds.items():
            t = _timed(fn)
            if i >= 10:
                times[k].append(t)
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = {"launch_ms_median": round(v[len(v) // 2], 5), "launch_ms_min": round(v[0], 5), "launch_ms_p90": round(v[(9 * len(v)) // 10], 5),
                  "launches": len(v)}
    return out


def _midgame(args):
    env = BatchedAzul(args.games, device="cuda", seed=1)
    env.runner_init()
    env.runner_init()
    traj = env.alloc_trajectory(args.advance)
    env.selfplay(args.advance, traj["mask"], traj["action"], traj["reward"], traj["done"])
    torch.cuda.synchronize()
    return env


def launch_times(args, env):
    n = env.n
    table = torch.empty(n, L.NUM_ACTIONS, dtype=torch.int32, device="cuda")
    best = torch.empty(n, dtype=torch.int32, device="cuda")
    mask = torch.empty(n, L.NUM_ACTIONS, dtype=torch.uint8, device="cuda")
    kinds = {"greedy_explore%d_k%d" % (e, k): (lambda e=e, k=k: env.playout_moves(k, SEED, CALL, sums=table, best=best, policy="greedy", explore=e))
             for e, k in GREEDY_KINDS}
    kinds.update({"uniform_k%d" % k: (lambda k=k: env.playout_moves(k, SEED, CALL, sums=table, best=best)) for k in UNIFORM_KS})
    kinds["score_moves"] = lambda: env.score_moves(L.PERSP_CURRENT, scores=table, best=best)
    kinds["legal_mask"] = lambda: env.get_valid_moves(out=mask)
    out = _interleaved(kinds, args.launches)
    legal = mask.sum(dim=1).float()
    out.update(legal_moves_per_state_mean=round(float(legal.mean()), 2), states_without_a_legal_move=int((legal == 0).sum()))
    out["greedy_0_1_in_uniform_k1_launches"] = round(out["greedy_explore0_k1"]["launch_ms_median"] / out["uniform_k1"]["launch_ms_median"], 2)
    return out


def parent_comparison(args, env):
    """azul_batch_playout_moves through the parent's library and through this one, on batches holding the same records."""
    P = C.CDLL(os.path.abspath(args.parent_lib))
    vp = C.c_void_p
    P.azul_batch_create_rules.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    P.azul_batch_set_state.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    P.azul_batch_playout_moves.argtypes = [vp, C.c_int, C.c_int, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
    P.azul_batch_destroy.argtypes = [vp]
    assert not hasattr(P, "azul_batch_playout_moves_policy"), "--parent-lib is not the parent's library: it has the new entry"
    first, pool = parse_rules(env.rules, 2)
    h = vp()
    assert P.azul_batch_create_rules(C.byref(h), env.n, 2, first, pool, 0) == L.SUCCESS
    recs = np.ascontiguousarray(env.get_records())
    stream = env._stream()
    assert P.azul_batch_set_state(h, 0, env.n, recs.ctypes.data_as(vp), stream) == L.SUCCESS
    torch.cuda.synchronize()
    n = env.n
    tabs = [torch.empty(n, L.NUM_ACTIONS, dtype=torch.int32, device="cuda") for _ in range(2)]
    bests = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    ptr = lambda t: vp(t.data_ptr())
    kinds = {}
    for k in PARENT_KS:
        kinds["parent_k%d" % k] = lambda k=k: P.azul_batch_playout_moves(h, L.PERSP_CURRENT, k, SEED, CALL, None, ptr(tabs[0]), ptr(bests[0]), stream)
        kinds["new_k%d" % k] = lambda k=k: L.lib.azul_batch_playout_moves(env._h, L.PERSP_CURRENT, k, SEED, CALL, None, ptr(tabs[1]), ptr(bests[1]), stream)
    out = _interleaved(kinds, args.launches)
    for k in PARENT_KS:
        kinds["parent_k%d" % k]()
        kinds["new_k%d" % k]()
        torch.cuda.synchronize()
        assert torch.equal(tabs[0], tabs[1]) and torch.equal(bests[0], bests[1]), "the two libraries' tables differ at K = %d" % k
        p, q = out["parent_k%d" % k], out["new_k%d" % k]
        spread = p["launch_ms_p90"] - p["launch_ms_median"]
        diff = q["launch_ms_median"] - p["launch_ms_median"]
        out["k%d" % k] = {"median_difference_ms": round(diff, 5), "median_difference_percent": round(100 * diff / p["launch_ms_median"], 3),
                          "parent_spread_ms_p90_minus_median": round(spread, 5),
                          "parent_spread_percent": round(100 * spread / p["launch_ms_median"], 3), "inside_parent_spread": bool(abs(diff) <= spread),
                          "tables_equal": True}
    P.azul_batch_destroy(h)
    return out


def rollout_rate(args, opponent, **kw):
    torch.manual_seed(0)
    pol = BatchedActorCritic(136, 180, 180)
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


def head_to_head(args, explore, K, other, seed):
    """The greedy-playout player at (explore, K) against `other` ("greedy" | "random" | "uniform_k8") until args.episodes episodes have
    finished: tools/playout_bench.py's head_to_head with this player in the alternating seat."""
    n = args.arena_games
    env = BatchedAzul(n, device="cuda", seed=seed)
    env.runner_init()
    dev = env.device
    idx = torch.arange(n, device=dev)
    played = torch.zeros(n, dtype=torch.int64, device=dev)         # episodes finished or abandoned per game: the player's seat alternates with it
    moves = torch.zeros(n, dtype=torch.int64, device=dev)
    wins = losses = draws = stuck = capped = 0
    margin = 0
    call = 0
    while wins + losses + draws < args.episodes:
        recs = env.get_records()
        mover = torch.from_numpy((recs["flags"] & 7).astype(np.int64) - 1).to(dev)
        seat = (idx + played) & 1                                  # the greedy-playout player's seat in this episode
        mine = (mover == seat).to(torch.uint8)
        if other == "greedy":
            act = env.greedy_action(active=1 - mine)
        elif other == "random":
            act = env.random_action(active=1 - mine)
        else:
            act = env.playout_action(8, SEED + 2, call, active=1 - mine)
        env.playout_action(K, SEED + 1, call, active=mine, out=act, policy="greedy", explore=explore)
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
    return {"player": "greedy playout, explore %d, K %d" % (explore, K), "opponent": other, "episodes": ep, "wins": wins, "losses": losses,
            "draws": draws, "win_rate": round(p, 4), "win_rate_standard_error": round(math.sqrt(p * (1 - p) / ep), 4),
            "mean_score_margin": round(margin / ep, 3), "restarted_nothing_legal": stuck, "restarted_move_cap": capped, "games": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--advance", type=int, default=40)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--arena-games", type=int, default=1024)
    ap.add_argument("--move-cap", type=int, default=400)
    ap.add_argument("--only", default="launches,parent,rollouts,strength")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_policy_bench.json"))
    args = ap.parse_args()
    only = set(args.only.split(","))
    res = {"tool": "python tools/playout_policy_bench.py --parent-lib <the parent commit's libazulhip.so> --games %d --advance %d --launches %d "
                   "--window %d --windows %d --episodes %d --arena-games %d --move-cap %d --only %s"
                   % (args.games, args.advance, args.launches, args.window, args.windows, args.episodes, args.arena_games, args.move_cap, args.only),
           "note": "one process. Launch times: HIP events around single launches on the same mid-game states (a seeded batch after --advance flat "
                   "self-play moves), the kinds interleaved, 10 warm-ups. uniform_vs_parent: azul_batch_playout_moves of this library and of the "
                   "parent commit's, built with the same flags, on batches holding the same records; spread = p90 - median of the parent's own "
                   "repeats. Rollouts: PolicyRollout agent steps/s per window, wall clock, all on the per-cut protocol. Strength: both seats "
                   "played from outside through Azul.step for every game, the first-named player's seat alternating by game and episode; win "
                   "rate = wins / finished episodes, draws listed.",
           "games": args.games, "window": args.window, "device": torch.cuda.get_device_name(0)}
    env = _midgame(args)
    if "launches" in only:
        res["launches"] = launch_times(args, env)
    if "parent" in only and args.parent_lib:
        res["uniform_vs_parent"] = parent_comparison(args, env)
    if "rollouts" in only:
        res["rollout_greedy_playout_0_1"] = rollout_rate(args, "playout", opponent_playouts=1, opponent_playout_policy="greedy")
        res["rollout_uniform_playout_k8"] = rollout_rate(args, "playout", opponent_playouts=8)
        res["rollout_greedy"] = rollout_rate(args, "greedy")
    if "strength" in only:
        res["strength"] = [head_to_head(args, 0, 1, "greedy", 7000), head_to_head(args, 0, 1, "uniform_k8", 8000),
                           head_to_head(args, 0, 1, "random", 9000), head_to_head(args, 64, 4, "greedy", 7100)]
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
