#!/usr/bin/env python3
"""Diagnostic: what ends a self-play launch -- one record per wave of azul_selfplay2_kernel (-DAZ_PROFILE_SEGMENTS build).

Every wave of the diagnostic build writes its s_memtime stamps (kernel entry, loop start, loop end, after rng2_close), its blockIdx.x,
where the hardware put it (HW_REG_HW_ID / HW_REG_XCC_ID) and how many of its game-moves took each rare block (csrc/azul_common.hpp).
This tool runs the bench's batch (seeds 0.., padded rows, compact record, 512 moves per launch) for a few launches after warm-up and
prints, per batch size: the histogram of wave end times, loop time per SIMD slot split older / younger, the same per XCD and per CU,
the regression of loop time on the rare-block counts, and prologue / epilogue durations.

    python tools/wave_timeline.py [--lib PATH] [--games 4096,2048,8192] [--launches 4] [--warmup 8] [--chunk 512] [--out FILE]

Without --lib the diagnostic library is built first (hipcc, as tools/segment_profile.py does).  The stamps cost time (the loop carries
the segment stamps too): read the SHAPE of the distribution here, never this build's absolute run time.  Ticks of s_memtime are
turned into microseconds with the launch's own event time over its first-start .. last-end span.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REC = 8
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def fields(rec):
    hw = (rec[:, 4] >> np.uint64(32)).astype(np.int64)
    return {
        "entry": rec[:, 0].astype(np.int64), "loop0": rec[:, 1].astype(np.int64), "loop1": rec[:, 2].astype(np.int64), "close": rec[:, 3].astype(np.int64),
        "block": (rec[:, 4] & np.uint64(0xffffffff)).astype(np.int64),
        "slot": hw & 15, "simd": (hw >> 4) & 3, "cu": (hw >> 8) & 15, "sh": (hw >> 12) & 1, "se": (hw >> 13) & 7,
        "xcd": (rec[:, 5] & np.uint64(15)).astype(np.int64),
        "round_end": (rec[:, 6] & np.uint64(0xffffffff)).astype(np.int64), "deal": (rec[:, 6] >> np.uint64(32)).astype(np.int64),
        "reset": (rec[:, 7] & np.uint64(0xffffffff)).astype(np.int64), "regen": (rec[:, 7] >> np.uint64(32)).astype(np.int64),
    }


def one_launch(f, wall_ms, tag):
    # s_memtime is read from a counter of the wave's own CU, and the counters do not share a zero (the raw stamps of one launch lie tens of
    # milliseconds apart between CUs): every stamp is taken relative to the earliest entry stamp of ITS CU -- the dispatcher hands every CU
    # its first wave of a launch within about a microsecond.  Durations inside a wave need no such assumption.
    cuk = ((f["xcd"] * 8 + f["se"]) * 2 + f["sh"]) * 16 + f["cu"]
    base = np.zeros(len(cuk), dtype=np.int64)
    for v in np.unique(cuk):
        base[cuk == v] = f["entry"][cuk == v].min()
    span = float((f["close"] - base).max())
    us = wall_ms * 1e3 / span if span > 0 else 0.0      # microseconds per tick, from the launch's own event time (upper bound: the event bracket holds the launch gap too)
    end = (f["close"] - base) * us
    start = (f["entry"] - base) * us
    loop = (f["loop1"] - f["loop0"]) * us
    pro = (f["loop0"] - f["entry"]) * us
    epi = (f["close"] - f["loop1"]) * us
    say("-- %s: %d waves, event time %.1f us, first start .. last end %d ticks" % (tag, len(end), wall_ms * 1e3, int(span)))
    say("   wave start after the first: mean %.1f us  p99 %.1f  max %.1f" % (start.mean(), np.percentile(start, 99), start.max()))
    say("   prologue %.2f us mean (max %.2f)   loop %.1f us mean (min %.1f  max %.1f)   epilogue %.2f us mean (max %.2f)" %
        (pro.mean(), pro.max(), loop.mean(), loop.min(), loop.max(), epi.mean(), epi.max()))
    say("   wave end, relative to the launch's first start, as a share of the last end (%.1f us):" % end.max())
    edges = np.linspace(0.6, 1.0, 21)
    h, _ = np.histogram(end / end.max(), bins=edges)
    below = int((end / end.max() < 0.6).sum())
    say("     < 0.600: %5d" % below)
    for i in range(20):
        say("     %.3f .. %.3f: %5d %s" % (edges[i], edges[i + 1], h[i], "#" * int(round(60.0 * h[i] / max(1, h.max())))))
    # the waves that share a SIMD: key (xcd, se, sh, cu, simd); older / younger by the entry stamp
    key = (((f["xcd"] * 8 + f["se"]) * 2 + f["sh"]) * 16 + f["cu"]) * 4 + f["simd"]
    order = np.lexsort((f["entry"], key))
    ks = key[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    rank = np.arange(len(ks)) - np.maximum.accumulate(np.where(first, np.arange(len(ks)), 0))
    counts = np.bincount(np.unique(ks, return_inverse=True)[1])
    say("   SIMDs holding waves: %d; waves per SIMD: %s" % (len(counts), dict(zip(*[a.tolist() for a in np.unique(counts, return_counts=True)]))))
    for rk in range(int(rank.max()) + 1 if rank.max() < 4 else 4):
        sel = order[rank == rk]
        if len(sel) == 0:
            continue
        say("   rank %d on its SIMD (0 = older): %5d waves  loop mean %.1f us  max %.1f   end mean %.1f us  max %.1f   slot ids %s" %
            (rk, len(sel), loop[sel].mean(), loop[sel].max(), end[sel].mean(), end[sel].max(),
             dict(zip(*[a.tolist() for a in np.unique(f["slot"][sel], return_counts=True)]))))
    pairs = order[(rank == 1)]
    older = order[np.flatnonzero(rank == 1) - 1] if len(pairs) else pairs
    if len(pairs):
        d = loop[pairs] - loop[older]
        say("   younger minus older loop time on the same SIMD: mean %+.1f us  std %.1f  |d| mean %.1f   (start gap mean %.2f us)" %
            (d.mean(), d.std(), np.abs(d).mean(), (start[pairs] - start[older]).mean()))
        say("   slower-of-the-pair minus faster: mean %.1f us; correlation of the pair's loop times %.3f" %
            (np.abs(d).mean(), float(np.corrcoef(loop[pairs], loop[older])[0, 1])))
    for name in ("xcd", "se", "simd", "slot"):
        vals = np.unique(f[name])
        say("   per %-4s " % name + "  ".join("%d: %.1f/%.1f" % (v, loop[f[name] == v].mean(), end[f[name] == v].max()) for v in vals) + "   (loop mean / last end, us)")
    cu_mean = np.array([loop[cuk == v].mean() for v in np.unique(cuk)])
    cu_end = np.array([end[cuk == v].max() for v in np.unique(cuk)])
    say("   per CU (%d CUs): loop mean min %.1f  median %.1f  max %.1f us;  last end min %.1f  median %.1f  max %.1f us" %
        (len(cu_mean), cu_mean.min(), np.median(cu_mean), cu_mean.max(), cu_end.min(), np.median(cu_end), cu_end.max()))
    # luck: loop time on the rare-block counts
    X = np.stack([np.ones(len(loop)), f["round_end"], f["deal"], f["reset"], f["regen"]], axis=1).astype(np.float64)
    coef, *_ = np.linalg.lstsq(X, loop, rcond=None)
    fit = X @ coef
    r2 = 1.0 - ((loop - fit) ** 2).sum() / max(1e-30, ((loop - loop.mean()) ** 2).sum())
    say("   counts per wave: round ends %.1f +- %.1f  deals %.1f +- %.1f  resets %.1f +- %.1f  regenerations %.1f +- %.1f" %
        (f["round_end"].mean(), f["round_end"].std(), f["deal"].mean(), f["deal"].std(), f["reset"].mean(), f["reset"].std(), f["regen"].mean(), f["regen"].std()))
    say("   loop us = %.1f %+.3f round_end %+.3f deal %+.3f reset %+.3f regen   R^2 %.3f   (std of loop %.2f us, of the fit %.2f us, of the residual %.2f us)" %
        (coef[0], coef[1], coef[2], coef[3], coef[4], r2, loop.std(), fit.std(), (loop - fit).std()))
    say("   last end / mean end %.4f   last end / median end %.4f   mean idle share of a slot before the launch's end %.2f %%" %
        (end.max() / end.mean(), end.max() / np.median(end), 100.0 * (1.0 - end.mean() / end.max())))
    return end.max() / end.mean()


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="a diagnostic library built before (default: build build/libazulhip_prof.so)")
    ap.add_argument("--games", default="4096,2048,8192")
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--dump", default=None, help="also write every launch's raw records to this .npz")
    args = ap.parse_args()
    lib = args.lib
    if lib is None:
        lib = os.path.join(ROOT, "build", "libazulhip_prof.so")
        os.makedirs(os.path.dirname(lib), exist_ok=True)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + ge.HIPCC_FLAGS + ["-DAZ_PROFILE_SEGMENTS", "-I", os.path.join(ROOT, "include"),
                              "-o", lib, os.path.join(ge.CSRC, "azul_kernels.hip")], cwd=ge.CSRC)
    import azul_deep_reinforcement_learning_amd._lib as L
    L.LIB_PATH = os.path.abspath(lib)
    L.lib = L._load()
    import torch
    from azul_deep_reinforcement_learning_amd import BatchedAzul
    L.lib.azul_batch_wave_timeline.restype = C.c_int
    L.lib.azul_batch_wave_timeline.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

    raw = {}

    def run_batch(n):
        env = BatchedAzul(n)
        env.seed(0)
        env.runner_init()
        env.runner_init()
        b = env.alloc_trajectory(args.chunk, packed_mask=True, mask_pitch=192, mask_bits=False)
        run = lambda: env.selfplay(args.chunk, b["mask"], b["action"], b["reward"], b["done"], packed=b["packed"])
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        nw = (n + 1) // 2
        rec = np.zeros((nw, REC), dtype=np.uint64)
        say("")
        say("==== %d games (%d waves), %d moves per launch, %d warm-up launches ====" % (n, nw, args.chunk, args.warmup))
        for i in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            L.check(L.lib.azul_batch_wave_timeline(env._h, rec.ctypes.data_as(C.c_void_p), nw))
            one_launch(fields(rec), e0.elapsed_time(e1), "launch %d" % i)
            raw["games%d_launch%d" % (n, i)] = rec.copy()
            raw["games%d_launch%d_event_ms" % (n, i)] = np.float64(e0.elapsed_time(e1))
        del env

    say("# per-wave timeline of azul_selfplay2_kernel (diagnostic build %s)" % os.path.basename(lib))
    for n in [int(x) for x in args.games.split(",")]:
        run_batch(n)
    if args.dump:
        np.savez_compressed(args.dump, **raw)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
