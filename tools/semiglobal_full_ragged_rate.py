#!/usr/bin/env python3
"""Times of the exact semi-global aligners on batches of mixed (len1, len2) (swmi_semiglobal_full_ragged*)
against the fixed-length entries timed in the same run; writes ONE JSON line to profiles/semiglobal_full_ragged_rate.txt (or
--out) and prints it.  Linear (1, -1, 1) and affine (1, -1, 3, 1), ends-only and traceback.  Every seq2 starts with a mutated
copy of its seq1 (90 % identity from position 0), so the best cell lies deep in the table and the walk has real work.

P1  the cost of raggedness, padding excluded: n = 16384, len2 = 1024 W with W uniform on {1, 2, 3, 4}, len1 drawn as pairs L
    and 4096 - L with L uniform on [1, 4095] inside each wave count, so each wave count's sum of len1 is that of len1 = 2048.
    Baseline: four fixed device calls at (2048, 1024 W) with that W's count, their times summed.
P2  equal shapes: every alignment (1024, 1024), n = 16384, ragged against fixed.
P0  the per-call term: the same n, every alignment (1, 1), ragged against fixed -- the plan on the CPU and the copy of the slots
    from pageable memory, with next to no kernel time under them.
P3  host arrays in and out, traceback, n = 2048, both lengths uniform on [64, 2048]: one ragged host call against one fixed
    host call per alignment.

THE ONE BAR is on P2, where the two kernels differ only by the slot load: ragged median <= fixed median * (1 + 2 * spread of the
fixed repeats) + (ragged median - fixed median) of P0 (never below 0).  A miss is reported as a miss ("within_bar": false and
the list "P2_misses").  No ratio is fixed in advance; the baseline is the unchanged fixed entry of the same run.

Device entries are timed with HIP events (torch) around `iters` back-to-back calls on one stream, after one warm-up call (it
grows the workspaces).  The baseline alternates with the ragged calls, `repeats` (5) of each; every entry reports all its
times, the medians, the ratio of the medians (baseline / ragged: above 1 the ragged call is the faster one) and the baseline's
spread (max - min) / median.

    python tools/semiglobal_full_ragged_rate.py [--iters 2] [--repeats 5] [--skip-p3] [--n 16384] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

SM = swmi.match_matrix(1, -1)
LINEAR, AFFINE = (1,), (3, 1)


def _events(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def _mutated(x, rng):
    """a copy of x with one base in ten redrawn"""
    return np.where(rng.random(x.shape) < 0.9, x, rng.integers(0, 4, x.shape)).astype(np.uint8)


def ragged_pairs(len1s, len2s, rng):
    """(seq1s, seq2s) concatenated: seq2 k starts with a mutated copy of seq1 k's start"""
    off1, off2 = _offsets(len1s), _offsets(len2s)
    cat1 = rng.integers(0, 4, int(off1[-1]), dtype=np.uint8)
    cat2 = rng.integers(0, 4, int(off2[-1]), dtype=np.uint8)
    for k in range(len(len1s)):
        w = int(min(len1s[k], len2s[k]))
        a, b = int(off1[k]), int(off2[k])
        cat2[b:b + w] = _mutated(cat1[a:a + w], rng)
    return cat1, off1, cat2, off2


def fixed_pairs(len1, len2, n, rng):
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[:, :w] = _mutated(a[:, :w], rng)
    return a, b


def _results(n, words, tb, dev):
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    mv = torch.zeros(max(int(words), 2), dtype=torch.int64, device=dev) if tb else None
    ln = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
    return (sc, ends, mv, ln), (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, ln.data_ptr() if tb else None)


def ragged_device_call(len1s, len2s, affine, tb, rng):
    """(call, what keeps its buffers alive)"""
    dev = torch.device("cuda:0")
    cat1, off1, cat2, off2 = ragged_pairs(len1s, len2s, rng)
    mo = swmi.local_full_ragged_move_offsets(off1, off2)
    pad = np.zeros(16, np.uint8)
    d1 = torch.from_numpy(np.concatenate([cat1, pad])).to(dev)
    d2 = torch.from_numpy(np.concatenate([cat2, pad])).to(dev)
    keep, bufs = _results(len(len1s), mo[-1], tb, dev)
    stream = torch.cuda.current_stream().cuda_stream
    sr = swmi.semiglobal_ragged
    entry = sr.semiglobal_full_affine_ragged_device if affine else sr.semiglobal_full_ragged_device
    gaps = AFFINE if affine else LINEAR
    return (lambda: entry(d1.data_ptr(), off1, d2.data_ptr(), off2, SM, *gaps, *bufs, stream=stream)), (d1, d2, keep)


def fixed_device_call(len1, len2, n, affine, tb, rng):
    dev = torch.device("cuda:0")
    a, b = fixed_pairs(len1, len2, n, rng)
    d1, d2 = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    keep, bufs = _results(n, n * swmi.semiglobal_full_move_words(len1, len2), tb, dev)
    stream = torch.cuda.current_stream().cuda_stream
    entry = swmi.semiglobal_full_affine_device if affine else swmi.semiglobal_full_device
    gaps = AFFINE if affine else LINEAR
    return (lambda: entry(d1.data_ptr(), len1, d2.data_ptr(), len2, n, SM, *gaps, *bufs, stream=stream)), (d1, d2, keep)


def summary(ragged, fixed, digits=3):
    """All times, the medians, baseline / ragged, and the baseline's spread."""
    rm, fm = statistics.median(ragged), statistics.median(fixed)
    return {"ragged": [round(x, digits) for x in ragged], "fixed": [round(x, digits) for x in fixed],
            "ragged_median": round(rm, digits), "fixed_median": round(fm, digits), "fixed_over_ragged": round(fm / rm, 3),
            "fixed_spread": round((max(fixed) - min(fixed)) / fm, 4)}


def alternate(ragged_call, fixed_calls, repeats, iters):
    """One warm-up of every call, then `repeats` times: the ragged call, then the fixed calls (their times summed)."""
    ragged_call()
    for call in fixed_calls:
        call()
    torch.cuda.synchronize()
    ragged, fixed = [], []
    for _ in range(repeats):
        ragged.append(_events(ragged_call, iters))
        fixed.append(sum(_events(call, iters) for call in fixed_calls))
    return summary(ragged, fixed)


def p1_shapes(n, rng):
    """(len1s, len2s, {W: count}): W uniform on 1..4; inside each W, len1 in pairs L, 4096 - L (an odd one out gets 2048)."""
    waves = rng.integers(1, 5, n)
    len1s = np.zeros(n, np.int64)
    for w in range(1, 5):
        idx = np.flatnonzero(waves == w)
        half = len(idx) // 2
        L = rng.integers(1, 4096, half)
        len1s[idx[:half]] = L
        len1s[idx[half:2 * half]] = 4096 - L
        len1s[idx[2 * half:]] = 2048
        assert int(len1s[idx].sum()) == 2048 * len(idx)
    order = rng.permutation(n)
    return len1s[order], 1024 * waves[order], {w: int((waves == w).sum()) for w in range(1, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--skip-p3", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semiglobal_full_ragged_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    rng = np.random.default_rng(2026)
    n = args.n
    out = {"metric": "semiglobal_full_ragged_ms", "params": [1, -1, 1], "affine": [1, -1, 3, 1], "n": n, "iters": args.iters,
           "repeats": args.repeats, "device": swmi.device_info()["arch"], "P2_misses": []}
    len1s, len2s, counts = p1_shapes(n, rng)
    for affine in (False, True):
        for tb in (False, True):
            key = "%s_%s" % ("affine" if affine else "linear", "traceback" if tb else "ends_only")
            call, keep = ragged_device_call(len1s, len2s, affine, tb, rng)
            fixed = [fixed_device_call(2048, 1024 * w, counts[w], affine, tb, rng) for w in range(1, 5)]
            out["P1_" + key] = alternate(call, [c for c, _ in fixed], args.repeats, args.iters)
            del call, keep, fixed
            torch.cuda.empty_cache()
            call, keep = ragged_device_call(np.full(n, 1), np.full(n, 1), affine, tb, rng)
            fcall, fkeep = fixed_device_call(1, 1, n, affine, tb, rng)
            p0 = alternate(call, [fcall], args.repeats, args.iters)
            p0["per_call_ms"] = round(p0["ragged_median"] - p0["fixed_median"], 3)
            out["P0_" + key] = p0
            del call, keep, fcall, fkeep
            call, keep = ragged_device_call(np.full(n, 1024), np.full(n, 1024), affine, tb, rng)
            fcall, fkeep = fixed_device_call(1024, 1024, n, affine, tb, rng)
            p2 = alternate(call, [fcall], args.repeats, args.iters)
            bar = p2["fixed_median"] * (1 + 2 * p2["fixed_spread"]) + max(p0["per_call_ms"], 0.0)
            p2["bar_ms"] = round(bar, 3)
            p2["within_bar"] = bool(p2["ragged_median"] <= bar)
            if not p2["within_bar"]:
                out["P2_misses"].append(key)
            out["P2_" + key] = p2
            print("P1, P0, P2", key, "done", file=sys.stderr, flush=True)      # (progress; the result is the one line)
            del call, keep, fcall, fkeep
            torch.cuda.empty_cache()
    if not args.skip_p3:
        m = 2048
        l1, l2 = rng.integers(64, 2049, m), rng.integers(64, 2049, m)
        cat1, off1, cat2, off2 = ragged_pairs(l1, l2, rng)
        a = [cat1[int(off1[k]):int(off1[k + 1])] for k in range(m)]
        b = [cat2[int(off2[k]):int(off2[k + 1])] for k in range(m)]
        pair1, pair2 = (cat1, off1), (cat2, off2)
        for affine in (False, True):
            if affine:
                run = lambda: swmi.semiglobal_ragged.semiglobal_full_affine_ragged(pair1, pair2, SM, *AFFINE)  # noqa: E731
                one = lambda x, y: swmi.semiglobal_full_affine(x[None], y[None], SM, *AFFINE)  # noqa: E731
            else:
                run = lambda: swmi.semiglobal_ragged.semiglobal_full_ragged(pair1, pair2, SM, *LINEAR)  # noqa: E731
                one = lambda x, y: swmi.semiglobal_full(x[None], y[None], SM, *LINEAR)  # noqa: E731
            run()                                                       # warm-up (device buffers of the host entries)
            one(a[0], b[0])
            ragged, fixed = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                run()
                ragged.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                for x, y in zip(a, b):
                    one(x, y)
                fixed.append(time.perf_counter() - t0)
            p3 = summary(ragged, fixed, 4)
            p3["n"] = m
            print("P3", "affine" if affine else "linear", "done", file=sys.stderr, flush=True)
            out["P3_%s_traceback_host_s" % ("affine" if affine else "linear")] = p3
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
