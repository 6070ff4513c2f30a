#!/usr/bin/env python3
"""Times of the any-length local aligners on batches of mixed (len1, len2) (swmi_local_full_ragged*)
against the fixed-length entries; prints ONE JSON line.  Parameters (1, -1, 1) and, for the affine aligner, (1, -1, 2, 1).

P1  the cost of raggedness, padding excluded: n = 16384, len2 = 1024 W with W uniform on {1, 2, 3, 4}, len1 drawn as pairs L
    and 4096 - L with L uniform on [1, 4095] inside each wave count, so each wave count's sum of len1 is that of len1 = 2048.
    Baseline: four fixed device calls at (2048, 1024 W) with that W's count, their times summed.  ratio = baseline / ragged
    (floor 0.85), linear and affine, ends-only and traceback.
P2  equal shapes: every alignment (1024, 1024), n = 16384; ragged time / fixed time (ceiling 1.10).
P3  host arrays in and out, traceback, n = 2048, both lengths uniform on [64, 2048]: one ragged host call against one fixed
    host call per alignment (floor 5x); and the time the asynchronous device entry takes to return for that batch, which
    bounds the CPU-side plan from above (the plan, the slots' staging copy and the launches' enqueueing).

Device entries are timed with HIP events (torch) around `iters` back-to-back calls on one stream, after one warm-up call (it
grows the workspaces).  The fixed-entry times are the baseline only while the fixed kernels are the parent's (DESIGN.md
section 19 records the assembly diff).

    python tools/local_full_ragged_rate.py [--iters 3] [--skip-p3] [--n 16384]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

SM = swmi.match_matrix(1, -1)
AFFINE = (2, 1)


def _events(call, iters):
    call()                                              # warm-up: workspaces grow here
    torch.cuda.synchronize()
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


def _results(n, words, tb, dev):
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros(max(int(words), 2), dtype=torch.int64, device=dev) if tb else None
    st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
    return (sc, ends, mv, st), (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None)


def ragged_device_call(len1s, len2s, affine, tb, rng):
    dev = torch.device("cuda:0")
    off1, off2 = _offsets(len1s), _offsets(len2s)
    mo = swmi.local_full_ragged_move_offsets(off1, off2)
    d1 = torch.from_numpy(rng.integers(0, 4, int(off1[-1]) + 16, dtype=np.uint8)).to(dev)
    d2 = torch.from_numpy(rng.integers(0, 4, int(off2[-1]) + 16, dtype=np.uint8)).to(dev)
    keep, bufs = _results(len(len1s), mo[-1], tb, dev)
    stream = torch.cuda.current_stream().cuda_stream
    if affine:
        call = lambda: swmi.local_full_affine_ragged_device(d1.data_ptr(), off1, d2.data_ptr(), off2, SM, *AFFINE, *bufs, stream=stream)  # noqa: E731
    else:
        call = lambda: swmi.local_full_ragged_device(d1.data_ptr(), off1, d2.data_ptr(), off2, SM, 1, *bufs, stream=stream)  # noqa: E731
    return call, (d1, d2, keep)


def fixed_device_ms(len1, len2, n, affine, tb, iters, rng):
    dev = torch.device("cuda:0")
    d1 = torch.from_numpy(rng.integers(0, 4, (n, len1), dtype=np.uint8)).to(dev)
    d2 = torch.from_numpy(rng.integers(0, 4, (n, len2), dtype=np.uint8)).to(dev)
    keep, bufs = _results(n, n * swmi.local_full_move_words(len1, len2), tb, dev)
    stream = torch.cuda.current_stream().cuda_stream
    if affine:
        call = lambda: swmi.local_full_affine_device(d1.data_ptr(), len1, d2.data_ptr(), len2, n, SM, *AFFINE, *bufs, stream=stream)  # noqa: E731
    else:
        call = lambda: swmi.local_full_device(d1.data_ptr(), len1, d2.data_ptr(), len2, n, SM, 1, *bufs, stream=stream)  # noqa: E731
    return _events(call, iters)


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
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--skip-p3", action="store_true")
    args = ap.parse_args()
    swmi.init(0)
    rng = np.random.default_rng(2025)
    n = args.n
    out = {"metric": "local_full_ragged_ms", "params": [1, -1, 1], "affine": [1, -1, 2, 1], "n": n, "device": swmi.device_info()["arch"]}
    len1s, len2s, counts = p1_shapes(n, rng)
    for affine in (False, True):
        for tb in (False, True):
            key = "%s_%s" % ("affine" if affine else "linear", "traceback" if tb else "ends_only")
            call, keep = ragged_device_call(len1s, len2s, affine, tb, rng)
            r_ms = _events(call, args.iters)
            del call, keep
            f_ms = [fixed_device_ms(2048, 1024 * w, counts[w], affine, tb, args.iters, rng) for w in range(1, 5)]
            out["P1_" + key] = {"ragged_ms": round(r_ms, 3), "fixed_ms": [round(x, 3) for x in f_ms], "fixed_sum_ms": round(sum(f_ms), 3),
                                "ratio": round(sum(f_ms) / r_ms, 3), "floor": 0.85}
            call, keep = ragged_device_call(np.full(n, 1024), np.full(n, 1024), affine, tb, rng)
            r_ms = _events(call, args.iters)
            del call, keep
            f_ms = fixed_device_ms(1024, 1024, n, affine, tb, args.iters, rng)
            out["P2_" + key] = {"ragged_ms": round(r_ms, 3), "fixed_ms": round(f_ms, 3), "time_ratio": round(r_ms / f_ms, 3), "ceiling": 1.10}
            torch.cuda.empty_cache()
    if not args.skip_p3:
        m = 2048
        l1, l2 = rng.integers(64, 2049, m), rng.integers(64, 2049, m)
        a = [rng.integers(0, 4, int(x), dtype=np.uint8) for x in l1]
        b = [rng.integers(0, 4, int(x), dtype=np.uint8) for x in l2]
        pair1, pair2 = swmi._ragged_seq1s(a), swmi._ragged_seq1s(b)
        for affine in (False, True):
            if affine:
                run = lambda: swmi.local_full_affine_ragged(pair1, pair2, SM, *AFFINE)  # noqa: E731
                one = lambda x, y: swmi.local_full_affine(x[None], y[None], SM, *AFFINE)  # noqa: E731
            else:
                run = lambda: swmi.local_full_ragged(pair1, pair2, SM, 1)  # noqa: E731
                one = lambda x, y: swmi.local_full(x[None], y[None], SM, 1)  # noqa: E731
            run()                                                           # warm-up (device buffers of the host entry)
            t0 = time.perf_counter()
            run()
            t_ragged = time.perf_counter() - t0
            one(a[0], b[0])
            t0 = time.perf_counter()
            for x, y in zip(a, b):
                one(x, y)
            t_fixed = time.perf_counter() - t0
            call, keep = ragged_device_call(l1, l2, affine, True, rng)
            call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t_issue = time.perf_counter() - t0
            torch.cuda.synchronize()
            del call, keep
            out["P3_%s_traceback" % ("affine" if affine else "linear")] = {
                "n": m, "ragged_host_s": round(t_ragged, 4), "per_alignment_host_s": round(t_fixed, 4),
                "speedup": round(t_fixed / t_ragged, 2), "floor": 5.0, "device_entry_returns_after_ms": round(t_issue * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
