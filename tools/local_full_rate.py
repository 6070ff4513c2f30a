#!/usr/bin/env python3
"""Alignments per second and TCUPS of the any-length local aligner (swmi_local_full*) beside the exact
semi-global aligner (swmi_semiglobal_full*, section 13) on the same buffers in the same run; prints ONE JSON line.

Resident buffers (the *_time_device entries: HIP events around `iters` back-to-back device calls after a warm-up call),
ends-only and traceback (walk included), at 16384 x 16384 (256 alignments per call), 4096 x 4096 (2048) and 1024 x 1024
(8192); and at 2048 x 128 (65536) beside swmi_local_align at len1 = 2048, the kernel built for 128 columns.  Inputs: pairs
with 10 % mismatches, 5 % insertions and 5 % deletions (seeded), parameters (1, -1, 1).  The floor of section 17 is
local / semi-global >= 0.75 in alignments per second at 16384 x 16384 and 4096 x 4096, both modes; "floors" says which hold.

    python tools/local_full_rate.py [--iters 5] [--scale 1.0] [--only-128]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

SHAPES = [(16384, 16384, 256), (4096, 4096, 2048), (1024, 1024, 8192)]
FLOOR = 0.75
FLOOR_SHAPES = ((16384, 16384), (4096, 4096))


def pairs(n, len1, len2, seed):
    """seq2 = seq1 with 10 % substitutions, 5 % of the positions dropped and as many random bases inserted (cut or padded
    with random bases to len2)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    for k in range(n):
        row = a[k].copy()
        sub = rng.random(len1) < 0.10
        row[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
        row = row[rng.random(len1) >= 0.05]
        ins = np.sort(rng.integers(0, len(row) + 1, len1 - len(row)))
        row = np.insert(row, ins, rng.integers(0, 4, len(ins), dtype=np.uint8))
        m = min(len(row), len2)
        b[k, :m] = row[:m]
    return a, b


def entry(n, len1, len2, ms):
    return {"ms_per_call": round(ms, 3), "alignments_per_s": round(n / (ms * 1e-3), 1),
            "tcups": round(n * len1 * len2 / (ms * 1e-3) / 1e12, 3)}


def measure(len1, len2, n, iters, sm, seed):
    dev = torch.device("cuda:0")
    a, b = pairs(n, len1, len2, seed)
    d1 = torch.from_numpy(a).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.local_full_move_words(len1, len2)), dtype=torch.int64, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    row = {"shape": [len1, len2], "n": n}
    for tb in (False, True):
        mode = "traceback" if tb else "ends_only"
        moves, counts = (mv.data_ptr(), cnt.data_ptr()) if tb else (None, None)
        local = swmi.local_full_time_device(d1.data_ptr(), len1, d2.data_ptr(), len2, n, sm, 1, sc.data_ptr(), ends.data_ptr(),
                                            moves, counts, 0, iters)
        if len2 == 128:
            other, name = swmi.local_time_device(d1.data_ptr(), len1, d2.data_ptr(), n, sm, 1, sc.data_ptr(), ends.data_ptr(),
                                                 moves, counts, 0, iters), "local_align"
        else:
            other, name = swmi.semiglobal_full_time_device(d1.data_ptr(), len1, d2.data_ptr(), len2, n, sm, 1, sc.data_ptr(),
                                                           ends.data_ptr(), moves, counts, 0, iters), "semiglobal_full"
        row[mode] = {"local_full": entry(n, len1, len2, local), name: entry(n, len1, len2, other),
                     "ratio": round(other / local, 4)}          # alignments per second: local_full over the comparator
    swmi.local_full_release_workspaces()
    swmi.semiglobal_full_release_workspaces()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--only-128", action="store_true", help="the 2048 x 128 line alone (for a kernel trace)")
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(1, -1)
    out = {"metric": "local_full_alignments_per_s", "params": [1, -1, 1], "iters": args.iters, "device": swmi.device_info()["arch"],
           "shapes": [], "floor": FLOOR, "floors": {}}
    if not args.only_128:
        for len1, len2, n in SHAPES:
            row = measure(len1, len2, max(1, int(n * args.scale)), args.iters, sm, 1526 + len1)
            out["shapes"].append(row)
            if (len1, len2) in FLOOR_SHAPES:
                for mode in ("ends_only", "traceback"):
                    out["floors"]["%dx%d %s" % (len1, len2, mode)] = "met" if row[mode]["ratio"] >= FLOOR else "missed"
    out["len2_128"] = measure(2048, 128, max(1, int(65536 * args.scale)), args.iters, sm, 128)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
