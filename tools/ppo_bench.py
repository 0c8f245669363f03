"""What PPO costs, measured in ONE process on one GPU and written to profiles/ppo_bench.json:

  * gradients  one azul_ppo_gradients launch beside one azul_a2c_gradients launch for each of the five compiled shapes, on the SAME
               n = games x window samples, weights and 256 workspace parts: ms per launch from device events around `--launches`
               back-to-back launches (gradient kernel + reduce), the two entries alternating, `--repeats` measurements each, the median
               beside every repeat, spread = (max - min) / median.  The two differ in the per-sample head only (csrc/azul_learner.hpp).
  * trainer    agent steps/s of BatchedTrainer.run_batch(collect_stats=False) with bootstrap_tail=True, gae_lambda=0.95, ring=1:
               algorithm="ppo" at epochs=1, minibatches=1 beside algorithm="a2c" (one optimiser step per window each), for the two-player
               persistent path and for three players with fused_wide=True and the fused learner; wall clock over `--batches` batches
               ending in a device synchronisation, three warm-up batches, the two trainers alternating.
  * ppo_4x4    the PPO trainer at epochs=4, minibatches=4 on the same two paths: agent steps/s and optimiser steps/s.

No claim about learning speed.  The GPU work runs under the script's own time limit (`--time-limit` seconds: the default action of SIGALRM
ends the process, also inside a blocked device call).

Usage: python tools/ppo_bench.py [--games 4096] [--window 32] [--launches 50] [--batches 100] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from azul_deep_reinforcement_learning_amd import BatchedActorCritic, _lib as L  # noqa: E402
from azul_deep_reinforcement_learning_amd.learner import A2CLearner, REFERENCE_SHAPE, WIDE_SHAPES  # noqa: E402
from azul_deep_reinforcement_learning_amd.training import BatchedTrainer  # noqa: E402

p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def median(xs):
    return sorted(xs)[len(xs) // 2]


def summary(xs, digits):
    med = median(xs)
    return {"median": round(med, digits), "repeats": [round(x, digits) for x in xs], "spread": round((max(xs) - min(xs)) / med, 4)}


def gradients(args):
    n = args.games * args.window
    res = {}
    for IN, H, A in (REFERENCE_SHAPE,) + WIDE_SHAPES:
        torch.manual_seed(0)
        pol = BatchedActorCritic(IN, A, H).cuda()
        lrn = A2CLearner(pol, fused=True)
        kw, ws = lrn.kweights("cuda"), lrn._ensure_flat(torch.device("cuda", torch.cuda.current_device()))
        g = torch.Generator(device="cuda").manual_seed(1)
        obs = torch.randint(0, 6, (n, IN), device="cuda", generator=g).float()
        mask = (torch.rand(n, A, device="cuda", generator=g) < 0.2).to(torch.uint8)
        action = torch.randint(0, A, (n,), device="cuda", generator=g).to(torch.int32)
        mask.scatter_(1, action.long().unsqueeze(1), 1)
        ret = torch.randn(n, device="cuda", generator=g) * 3
        old = -torch.rand(n, device="cuda", generator=g) * 4
        adv = torch.randn(n, device="cuda", generator=g)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        wts = (p(kw["w1t"]), p(kw["b1"]), p(kw["w2c"]), p(kw["b2c"]), p(kw["w2a_t"]), p(kw["b2a"]), p(pol.actor_linear2.weight), IN, H, A,
               p(ws["ws"]), 256, p(ws["grad"]), None, None, None)
        f32 = C.c_float
        calls = {"azul_a2c_gradients": lambda: L.check(L.lib.azul_a2c_gradients(p(obs), p(mask), p(action), p(ret), n, f32(1.0 / n), *wts, st)),
                 "azul_ppo_gradients": lambda: L.check(L.lib.azul_ppo_gradients(p(obs), p(mask), p(action), p(ret), p(old), p(adv), n, f32(1.0 / n),
                                                                               f32(0.2), f32(0.5), f32(0.01), *wts, None, st))}
        for call in calls.values():
            for _ in range(5):
                call()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, call in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    call()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / args.launches)
        row = {k: summary(v, 4) for k, v in ms.items()}
        row["ppo_over_a2c"] = round(row["azul_ppo_gradients"]["median"] / row["azul_a2c_gradients"]["median"], 4)
        res["%dx%dx%d" % (IN, H, A)] = row
        print(json.dumps({"gradients": {"%dx%dx%d" % (IN, H, A): row}}), flush=True)
        del lrn, pol, obs, mask
        torch.cuda.empty_cache()
    return {"samples": n, "workspace_parts": 256, "launches_per_measurement": args.launches, "ms_per_launch": res}


PATHS = {"two_player_persistent": dict(players=2, persistent=True),
         "three_player_fused_wide": dict(players=3, fused_wide=True, fused_learner=True)}


def trainer(args, path, **kw):
    torch.manual_seed(0)
    pk = PATHS[path]
    tr = BatchedTrainer(BatchedActorCritic(188 if pk["players"] == 3 else 136, 180, 180), n_games=args.games, window=args.window, opponent="random",
                        ring=1, bootstrap_tail=True, gae_lambda=0.95, **pk, **kw)
    for _ in range(3):
        tr.run_batch(collect_stats=False)
    torch.cuda.synchronize()
    return tr


def timed(tr, batches):
    torch.cuda.synchronize()
    u0, t0 = tr.learner.updates, time.perf_counter()
    for _ in range(batches):
        tr.run_batch(collect_stats=False)
    tr.rollout.synchronize()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return tr.rollout.n * tr.rollout.T * batches / dt, (tr.learner.updates - u0) / dt


def trainers(args):
    res = {"one_step_per_window": {}, "ppo_4x4": {}}
    for path in PATHS:
        trs = {"a2c": trainer(args, path, algorithm="a2c"), "ppo_1x1": trainer(args, path, algorithm="ppo", epochs=1, minibatches=1),
               "ppo_4x4": trainer(args, path, algorithm="ppo", epochs=4, minibatches=4)}
        rates = {k: ([], []) for k in trs}
        for _ in range(args.repeats):
            for k, tr in trs.items():
                steps, opt = timed(tr, args.batches if k != "ppo_4x4" else max(1, args.batches // 4))
                rates[k][0].append(steps)
                rates[k][1].append(opt)
        row = {k: {"agent_steps_per_s": summary(rates[k][0], 0), "samples_last_step": float(trs[k].learner.statistics["samples"][-1])}
               for k in ("a2c", "ppo_1x1")}
        row["ppo_over_a2c"] = round(row["ppo_1x1"]["agent_steps_per_s"]["median"] / row["a2c"]["agent_steps_per_s"]["median"], 4)
        res["one_step_per_window"][path] = row
        res["ppo_4x4"][path] = {"agent_steps_per_s": summary(rates["ppo_4x4"][0], 0), "optimiser_steps_per_s": summary(rates["ppo_4x4"][1], 1),
                                "samples_last_step": float(trs["ppo_4x4"].learner.statistics["samples"][-1])}
        print(json.dumps({path: {"one_step_per_window": row, "ppo_4x4": res["ppo_4x4"][path]}}), flush=True)
        del trs
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the figures are the MI355X's: no device, no measurement"
    signal.alarm(args.time_limit)                              # (no handler: the default action ends the process)
    res = {"tool": "python tools/ppo_bench.py --games %d --window %d --launches %d --batches %d --repeats %d"
                   % (args.games, args.window, args.launches, args.batches, args.repeats),
           "note": "one process, one GPU. gradients: ms per launch (gradient kernel + reduce) from device events around back-to-back launches "
                   "of each entry on the same samples, weights and 256 workspace parts, the entries alternating. trainer: "
                   "BatchedTrainer.run_batch(collect_stats=False) with ring=1, bootstrap_tail=True, gae_lambda=0.95, wall clock over the timed "
                   "batches ending in a device synchronisation, three warm-up batches, the trainers alternating; ppo_4x4 runs a quarter of the "
                   "batches per measurement. median, every repeat and spread = (max - min) / median.",
           "device": torch.cuda.get_device_name(0), "games": args.games, "window": args.window}
    res["gradients"] = gradients(args)
    res["trainer"] = trainers(args)
    signal.alarm(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
