#!/usr/bin/env python3
"""Alignments per second and TCUPS of the any-length affine local aligner (swmi_local_full_affine*)
beside the affine exact semi-global aligner (swmi_semiglobal_full_affine*, section 16: the same mapping and cell without the
zero floor) on the same resident buffers in the same process; prints ONE JSON line.

Resident buffers (the *_time_device entries: HIP events around `iters` back-to-back device calls), ends-only and traceback
(walk included), at 16384 x 16384 (256 alignments per call), 4096 x 4096 (2048) and 1024 x 1024 (8192).  Per shape and mode: a
warm-up call of each aligner, then the two aligners ALTERNATED for `rounds` rounds of `iters` calls each; every round is
reported, the ratio is taken on the median round of each.  Inputs: pairs with 10 % mismatches, 5 % insertions and 5 %
deletions (seeded), parameters (1, -1), open 5, extend 2.  Workspaces are released between shapes.  The floor of section 18
is local / semi-global >= 0.75 in alignments per second at 16384 x 16384 and 4096 x 4096, both modes; "floors" says which
hold.  Reported without a floor: 1024 x 1024; swmi_local_full at gap = open on the same buffers (what affine gaps cost);
2048 x 128 beside swmi_local_align_affine, the kernel built for 128 columns; the host entry at 16384 x 16384 with traceback.

    python tools/local_full_affine_rate.py [--iters 10] [--rounds 3] [--scale 1.0] [--no-host]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402
from local_full_rate import pairs  # noqa: E402  (section 17's input recipe)

SHAPES = [(16384, 16384, 256), (4096, 4096, 2048), (1024, 1024, 8192)]
OPEN, EXTEND = 5, 2
FLOOR = 0.75
FLOOR_SHAPES = ((16384, 16384), (4096, 4096))


def entry(n, len1, len2, rounds):
    ms = float(np.median(rounds))
    return {"ms_per_call": round(ms, 3), "rounds_ms": [round(x, 3) for x in rounds], "alignments_per_s": round(n / (ms * 1e-3), 1),
            "tcups": round(n * len1 * len2 / (ms * 1e-3) / 1e12, 3)}


def measure(len1, len2, n, iters, rounds, sm, seed):
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
        moves, counts = (mv.data_ptr(), cnt.data_ptr()) if tb else (None, None)
        head = (d1.data_ptr(), len1, d2.data_ptr())
        tail = (sc.data_ptr(), ends.data_ptr(), moves, counts, 0)
        if len2 == 128:
            name = "local_align_affine"
            other = lambda it: swmi.local_affine_time_device(*head, n, sm, OPEN, EXTEND, *tail, it)  # noqa: E731
        else:
            name = "semiglobal_full_affine"
            other = lambda it: swmi.semiglobal_full_affine_time_device(*head, len2, n, sm, OPEN, EXTEND, *tail, it)  # noqa: E731
        local = lambda it: swmi.local_full_affine_time_device(*head, len2, n, sm, OPEN, EXTEND, *tail, it)  # noqa: E731
        local(1)                                            # warm-up: workspaces, code objects
        other(1)
        got = {"local": [], "other": []}
        for _ in range(rounds):
            got["local"].append(local(iters))
            got["other"].append(other(iters))
        cell = {"local_full_affine": entry(n, len1, len2, got["local"]), name: entry(n, len1, len2, got["other"])}
        # alignments per second: local_full_affine over the comparator, on the median round of each
        cell["ratio"] = round(float(np.median(got["other"])) / float(np.median(got["local"])), 4)
        if len2 != 128:
            swmi.local_full_time_device(*head, len2, n, sm, OPEN, *tail, 1)
            linear = [swmi.local_full_time_device(*head, len2, n, sm, OPEN, *tail, iters) for _ in range(rounds)]
            cell["local_full"] = entry(n, len1, len2, linear)
            cell["ratio_to_local_full"] = round(float(np.median(linear)) / float(np.median(got["local"])), 4)
            swmi.local_full_release_workspaces()
        row["traceback" if tb else "ends_only"] = cell
    swmi.local_full_affine_release_workspaces()
    swmi.semiglobal_full_affine_release_workspaces()
    return row


def host_entry(len1, len2, n, sm, seed):
    a, b = pairs(n, len1, len2, seed)
    swmi.local_full_affine(a[:2], b[:2], sm, OPEN, EXTEND)                # warm-up
    t0 = time.perf_counter()
    swmi.local_full_affine(a, b, sm, OPEN, EXTEND)
    ms = (time.perf_counter() - t0) * 1e3
    swmi.local_full_affine_release_workspaces()
    return {"shape": [len1, len2], "n": n, "ms_per_call": round(ms, 1), "alignments_per_s": round(n / (ms * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--no-host", action="store_true", help="skip the host entry's line (for a kernel trace)")
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(1, -1)
    out = {"metric": "local_full_affine_alignments_per_s", "params": [1, -1, OPEN, EXTEND], "iters": args.iters, "rounds": args.rounds,
           "device": swmi.device_info()["arch"], "shapes": [], "floor": FLOOR, "floors": {}}
    for len1, len2, n in SHAPES:
        row = measure(len1, len2, max(1, int(n * args.scale)), args.iters, args.rounds, sm, 1526 + len1)
        out["shapes"].append(row)
        if (len1, len2) in FLOOR_SHAPES:
            for mode in ("ends_only", "traceback"):
                out["floors"]["%dx%d %s" % (len1, len2, mode)] = "met" if row[mode]["ratio"] >= FLOOR else "missed"
    out["len2_128"] = measure(2048, 128, max(1, int(65536 * args.scale)), args.iters, args.rounds, sm, 128)
    if not args.no_host:
        out["host_entry"] = host_entry(16384, 16384, max(1, int(256 * args.scale)), sm, 1526 + 16384)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
