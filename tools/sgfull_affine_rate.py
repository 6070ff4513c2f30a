#!/usr/bin/env python3
"""Alignments per second of the affine exact semi-global aligner (swmi_semiglobal_full_affine*) against
the linear one (swmi_semiglobal_full*, section 13) on the same resident buffers, in one process; prints ONE JSON line.

Resident buffers: HIP events around `iters` back-to-back device calls after one untimed call (the *_time_device entries), at
16384 x 16384 (ends-only and traceback, walk included), 4096 x 4096 and 1024 x 1024; and one host-entry line (host arrays in
and out, traceback) at 16384 x 16384, timed on a second call after one that grows the buffers.  Inputs: pairs of the reference's 70 %-identity shape (10 % mismatches, 5 % insertions,
5 % deletions, seeded), so that the walks are full length.  Parameters (1, -1) with open 5, extend 2 against linear gap 2.

    python tools/sgfull_affine_rate.py [--n 256] [--iters 5] [--sizes 16384,4096,1024] [--no-host]

(--sizes 16384 --no-host: the 16384 x 16384 device lines alone, for a kernel-trace run.)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

OPEN, EXTEND, GAP = 5, 2, 2


def pairs(n, length, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, length), dtype=np.uint8)
    b = a.copy()
    sub = rng.random((n, length)) < 0.10
    b[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
    for k in range(n):                                  # indels: drop 5 % of the positions, insert as many random bases
        keep = rng.random(length) >= 0.05
        row = b[k][keep]
        ins = np.sort(rng.integers(0, len(row), length - len(row)))
        b[k] = np.insert(row, ins, rng.integers(0, 4, len(ins), dtype=np.uint8))[:length]
    return a, b


def both_rates(a, b, traceback, iters, sm):
    """(affine ms, linear ms) per call on the same device buffers"""
    dev = torch.device("cuda:0")
    n, length = a.shape
    d1 = torch.from_numpy(a).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.semiglobal_full_move_words(length, length)), dtype=torch.int64, device=dev) if traceback else None
    ln = torch.zeros(n, dtype=torch.int32, device=dev) if traceback else None
    torch.cuda.synchronize()
    args = (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if traceback else None, ln.data_ptr() if traceback else None, 0, iters)
    ms_a = swmi.semiglobal_full_affine_time_device(d1.data_ptr(), length, d2.data_ptr(), length, n, sm, OPEN, EXTEND, *args)
    swmi.semiglobal_full_affine_release_workspaces()
    ms_l = swmi.semiglobal_full_time_device(d1.data_ptr(), length, d2.data_ptr(), length, n, sm, GAP, *args)
    swmi.semiglobal_full_release_workspaces()
    return ms_a, ms_l


def row(n, length, ms_a, ms_l):
    return {"n": n, "affine_ms": round(ms_a, 3), "linear_ms": round(ms_l, 3),
            "affine_alignments_per_s": round(n / (ms_a * 1e-3), 1), "linear_alignments_per_s": round(n / (ms_l * 1e-3), 1),
            "affine_gcups": round(n * length * length / (ms_a * 1e-3) / 1e9, 1), "ratio": round(ms_l / ms_a, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", default="16384,4096,1024")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    swmi.init(0)
    sm = swmi.match_matrix(1, -1)
    out = {"metric": "semiglobal_full_affine_vs_linear", "params": [1, -1], "open_extend": [OPEN, EXTEND], "linear_gap": GAP,
           "device": swmi.device_info()["arch"]}
    a, b = pairs(args.n, 16384, 1776)
    for length, n in ((16384, args.n), (4096, 2048), (1024, 8192)):
        if length not in sizes:
            continue
        a2, b2 = (a, b) if length == 16384 else pairs(n, length, length)
        for tb in (False, True):
            out["%d_%s" % (length, "traceback" if tb else "ends_only")] = row(n, length, *both_rates(a2, b2, tb, args.iters, sm))
    if args.no_host:
        print(json.dumps(out))
        return
    swmi.semiglobal_full_affine(a, b, sm, OPEN, EXTEND)             # buffers grown and streams set up outside the timing
    t0 = time.perf_counter()
    swmi.semiglobal_full_affine(a, b, sm, OPEN, EXTEND)
    dt = time.perf_counter() - t0
    swmi.semiglobal_full_affine_release_workspaces()
    swmi.semiglobal_full(a, b, sm, GAP)
    t0 = time.perf_counter()
    swmi.semiglobal_full(a, b, sm, GAP)
    dl = time.perf_counter() - t0
    swmi.semiglobal_full_release_workspaces()
    out["host_16384_traceback"] = row(args.n, 16384, dt * 1e3, dl * 1e3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
