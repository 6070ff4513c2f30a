#!/usr/bin/env python3
"""Alignments per second and TCUPS of the exact semi-global aligner (swmi_semiglobal_full*); prints
ONE JSON line.

Resident buffers (swmi_semiglobal_full_time_device: HIP events around back-to-back device calls) at 16384 x 16384,
ends-only and traceback (walk included), and the traceback on pairs with no walk (the walk's share of the time); the host entry (swmi_semiglobal_full, host arrays in and out) with traceback.
Inputs: pairs of the reference's 70 %-identity shape (10 % mismatches, 5 % insertions, 5 % deletions, seeded), so that the
walks are full length.  Parameters (1, -1, 1), those of the reference's SemiGlobal_111.

    python tools/sgfull_rate.py [--n 256] [--iters 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

L = 16384


def pairs(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, L), dtype=np.uint8)
    b = a.copy()
    sub = rng.random((n, L)) < 0.10
    b[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
    for k in range(n):                                  # indels: drop 5 % of the positions, insert as many random bases
        keep = rng.random(L) >= 0.05
        row = b[k][keep]
        ins = np.sort(rng.integers(0, len(row), L - len(row)))
        b[k] = np.insert(row, ins, rng.integers(0, 4, len(ins), dtype=np.uint8))[:L]
    return a, b


def device_rate(a, b, traceback, iters, sm):
    dev = torch.device("cuda:0")
    n = len(a)
    d1 = torch.from_numpy(a).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.semiglobal_full_move_words(L, L)), dtype=torch.int64, device=dev) if traceback else None
    ln = torch.zeros(n, dtype=torch.int32, device=dev) if traceback else None
    torch.cuda.synchronize()
    ms = swmi.semiglobal_full_time_device(d1.data_ptr(), L, d2.data_ptr(), L, n, sm, 1, sc.data_ptr(), ends.data_ptr(),
                                          mv.data_ptr() if traceback else None, ln.data_ptr() if traceback else None, 0, iters)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(1, -1)
    a, b = pairs(args.n, 1776)
    out = {"metric": "semiglobal_full_alignments_per_s", "shape": [L, L], "params": [1, -1, 1], "device": swmi.device_info()["arch"]}
    for tb in (False, True):
        ms = device_rate(a, b, tb, args.iters, sm)
        out["device_%s" % ("traceback" if tb else "ends_only")] = {
            "n": args.n, "ms_per_call": round(ms, 3), "alignments_per_s": round(args.n / (ms * 1e-3), 1),
            "tcups": round(args.n * L * L / (ms * 1e-3) / 1e12, 3)}
    # the walk's share: the same traceback call on pairs whose best cell is (0,0) (every cell a mismatch), which write
    # the same codes and walk no step
    ms = device_rate(np.zeros_like(a), np.ones_like(b), True, args.iters, sm)
    out["device_traceback_no_walk"] = {"n": args.n, "ms_per_call": round(ms, 3)}
    out["walk_share"] = round(1 - ms / out["device_traceback"]["ms_per_call"], 4)
    swmi.semiglobal_full(a[:1], b[:1], sm, 1)                      # buffers and streams set up outside the timing
    t0 = time.perf_counter()
    swmi.semiglobal_full(a, b, sm, 1)
    dt = time.perf_counter() - t0
    out["host_traceback"] = {"n": args.n, "ms_per_call": round(dt * 1e3, 2), "alignments_per_s": round(args.n / dt, 1),
                             "tcups": round(args.n * L * L / dt / 1e12, 3)}
    swmi.semiglobal_full_release_workspaces()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
