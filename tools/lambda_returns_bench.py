"""What the TD(lambda) returns cost, measured in ONE process on one GPU and written to profiles/lambda_returns_bench.json:

  * scan      azul_discounted_returns_ring and azul_lambda_returns_ring on the SAME buffers (4096 games, a ring of 4 x 32 slots, the whole
              ring per launch): ms per launch from device events around `--launches` back-to-back launches (so a launch's fixed cost is
              in the figure), the two entries alternating, `--repeats` such measurements each, the median beside every repeat.  Per step
              the new scan reads 9 bytes (reward 4, done 1, value 4) where the old one reads 5, both write 4: the file records the ratio
              beside 9 / 5 and 13 / 9.  No target: an unexpected ratio is a finding.
  * trainer   agent steps/s of BatchedTrainer.run_batch(collect_stats=False) at 4096 games, window 32, for the two-player persistent
              path and for three players with fused_wide=True and the fused learner: gae_lambda=None against 0.95 (ring of three windows),
              and ring=1 without against with bootstrap_tail=True (which trains every recorded step, so it also does more learner work);
              wall clock over `--batches` batches ending in a device synchronisation, after three warm-up batches; the trainers of a
              comparison alternate, `--repeats` measurements each, spread = (max - min) / median.

No claim about learning speed.  The GPU work runs under the script's own time limit (`--time-limit` seconds: the default action of SIGALRM
ends the process, also inside a blocked device call).

Usage: python tools/lambda_returns_bench.py [--games 4096] [--window 32] [--launches 2000] [--batches 300] [--repeats 5] [--out FILE]
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
from azul_deep_reinforcement_learning_amd.training import BatchedTrainer  # noqa: E402

p = lambda t: C.c_void_p(t.data_ptr())


def median(xs):
    return sorted(xs)[len(xs) // 2]


def summary(xs, digits):
    med = median(xs)
    return {"median": round(med, digits), "repeats": [round(x, digits) for x in xs], "spread": round((max(xs) - min(xs)) / med, 4)}


def scan(args):
    N, R = args.games, 4 * args.window
    g = torch.Generator(device="cuda").manual_seed(0)
    reward = torch.randint(-30, 31, (R, N), dtype=torch.int32, device="cuda", generator=g)
    done = (torch.rand(R, N, device="cuda", generator=g) < 0.03).to(torch.uint8)
    value = torch.randn(R, N, device="cuda", generator=g) * 5
    out = torch.zeros(R, N, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    played = 7 * args.window                                   # the newest step in the middle of the ring
    calls = {"azul_discounted_returns_ring": lambda: L.check(L.lib.azul_discounted_returns_ring(p(reward), p(done), p(out), C.c_float(0.99), R,
                                                                                               played, R, N, st)),
             "azul_lambda_returns_ring": lambda: L.check(L.lib.azul_lambda_returns_ring(p(reward), p(done), p(value), None, p(out), C.c_float(0.99),
                                                                                       C.c_float(0.95), R, played, R, N, st))}
    for call in calls.values():
        for _ in range(20):
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
    res = {"games": N, "ring_steps": R, "span_steps": R, "launches_per_measurement": args.launches,
           "ms_per_launch": {k: summary(v, 5) for k, v in ms.items()}}
    old, new = (res["ms_per_launch"][k]["median"] for k in calls)
    res["lambda_over_discounted"] = round(new / old, 3)
    res["expected_by_bytes_read"] = round(9 / 5, 3)
    res["expected_by_bytes_moved"] = round(13 / 9, 3)
    res["bytes_moved_per_launch"] = {"azul_discounted_returns_ring": 9 * R * N, "azul_lambda_returns_ring": 13 * R * N}
    res["gb_per_s"] = {k: round(res["bytes_moved_per_launch"][k] / (res["ms_per_launch"][k]["median"] * 1e-3) / 1e9, 1) for k in calls}
    return res


PATHS = {"two_player_persistent": dict(players=2, persistent=True),
         "three_player_fused_wide": dict(players=3, fused_wide=True, fused_learner=True)}
COMPARISONS = {"gae_lambda_ring3": [("none", dict(ring=3)), ("lambda_0p95", dict(ring=3, gae_lambda=0.95))],
               "bootstrap_tail_ring1": [("none", dict(ring=1)), ("bootstrap_tail", dict(ring=1, bootstrap_tail=True)),
                                        ("bootstrap_tail_lambda_0p95", dict(ring=1, bootstrap_tail=True, gae_lambda=0.95))]}


def trainer(args, path, kw):
    torch.manual_seed(0)
    pk = PATHS[path]
    tr = BatchedTrainer(BatchedActorCritic(188 if pk["players"] == 3 else 136, 180, 180), n_games=args.games, window=args.window, opponent="random",
                        **pk, **kw)
    for _ in range(3):
        tr.run_batch(collect_stats=False)
    torch.cuda.synchronize()
    return tr


def timed(tr, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        tr.run_batch(collect_stats=False)
    tr.rollout.synchronize()
    torch.cuda.synchronize()
    return tr.rollout.n * tr.rollout.T * batches / (time.perf_counter() - t0)


def trainers(args):
    res = {}
    for path in PATHS:
        res[path] = {}
        for name, variants in COMPARISONS.items():
            trs = {k: trainer(args, path, kw) for k, kw in variants}
            rates = {k: [] for k in trs}
            for _ in range(args.repeats):
                for k, tr in trs.items():
                    rates[k].append(timed(tr, args.batches))
            row = {k: dict(summary(v, 0), ring=trs[k].rollout.ring, samples_last_update=float(trs[k].learner.statistics["samples"][-1]))
                   for k, v in rates.items()}
            for k in list(rates)[1:]:
                row[k + "_over_none"] = round(row[k]["median"] / row["none"]["median"], 4)
            res[path][name] = row
            print(json.dumps({path: {name: row}}), flush=True)
            del trs
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--batches", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lambda_returns_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the figures are the MI355X's: no device, no measurement"
    signal.alarm(args.time_limit)                              # (no handler: the default action ends the process)
    res = {"tool": "python tools/lambda_returns_bench.py --games %d --window %d --launches %d --batches %d --repeats %d"
                   % (args.games, args.window, args.launches, args.batches, args.repeats),
           "note": "one process, one GPU. scan: ms per launch from device events around back-to-back launches of each entry on the same "
                   "buffers (whole ring of 4 windows per launch), the entries alternating; the ratio stands beside what the bytes read "
                   "(9 / 5) and the bytes moved (13 / 9) per step would give, no target. trainer: agent steps/s of "
                   "BatchedTrainer.run_batch(collect_stats=False), wall clock over the timed batches ending in a device synchronisation, "
                   "three warm-up batches, the trainers of a comparison alternating; median, every repeat and spread = (max - min) / "
                   "median. bootstrap_tail trains every recorded step (samples_last_update), so its learner does more work per batch.",
           "device": torch.cuda.get_device_name(0), "games": args.games, "window": args.window}
    res["scan"] = scan(args)
    print(json.dumps(res["scan"]), flush=True)
    res["trainer"] = trainers(args)
    signal.alarm(0)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
