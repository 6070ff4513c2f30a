#!/usr/bin/env python3
"""Alignments per second and TCUPS of the global / free-end-gap aligner (swmi_global_full*) beside
the exact semi-global aligner's (swmi_semiglobal_full*, section 13) IN THE SAME RUN; prints ONE JSON line.

Resident buffers, 256 alignments of 16384 x 16384, parameters (1, -1, 1), the inputs of tools/sgfull_rate.py (pairs of the
reference's 70 %-identity shape, seeded).  Ends-only and traceback (walk included), for the masks GLOBAL, FIT and OVERLAP.
The yardstick is the semi-global aligner on the same device buffers: in each of `reps` repetitions the four aligners are
timed one after the other (swmi_*_time_device: one untimed call, then HIP events around `iters` back-to-back device calls),
so that whatever else the machine does meets all four alike; the line holds each one's fastest and slowest repetition, and
`semiglobal_spread` = max / min - 1 of the semi-global aligner's own repetitions, the noise against which
`slower_than_semiglobal` = min / semi-global min - 1 is to be read.

    python tools/global_full_rate.py [--n 256] [--reps 5] [--iters 4]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402,F401
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402
from sgfull_rate import L, pairs  # noqa: E402

MASKS = (("global", swmi.ENDS_GLOBAL), ("fit", swmi.ENDS_FIT), ("overlap", swmi.ENDS_OVERLAP))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(1, -1)
    n = args.n
    a, b = pairs(n, 1776)
    dev = torch.device("cuda:0")
    d1 = torch.from_numpy(a).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.global_full_move_words(L, L)), dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    assert swmi.semiglobal_full_move_words(L, L) == swmi.global_full_move_words(L, L)

    def run(name, mask, tb):
        tail = (mv.data_ptr() if tb else None, st.data_ptr() if tb else None, 0, args.iters)
        if name == "semiglobal":
            return swmi.semiglobal_full_time_device(d1.data_ptr(), L, d2.data_ptr(), L, n, sm, 1, sc.data_ptr(), ends.data_ptr(), *tail)
        return swmi.global_full_time_device(d1.data_ptr(), L, d2.data_ptr(), L, n, sm, 1, mask, sc.data_ptr(), ends.data_ptr(), *tail)

    out = {"metric": "global_full_alignments_per_s", "shape": [L, L], "params": [1, -1, 1], "n": n, "reps": args.reps,
           "iters": args.iters, "device": swmi.device_info()["arch"]}
    for tb in (False, True):
        ms = {name: [] for name in ("semiglobal",) + tuple(m[0] for m in MASKS)}
        for _ in range(args.reps):
            for name, mask in (("semiglobal", 0),) + MASKS:
                ms[name].append(run(name, mask, tb))
        sg_min = min(ms["semiglobal"])
        block = {}
        for name, v in ms.items():
            lo, hi = min(v), max(v)
            block[name] = {"ms_min": round(lo, 3), "ms_max": round(hi, 3), "alignments_per_s": round(n / (lo * 1e-3), 1),
                           "tcups": round(n * L * L / (lo * 1e-3) / 1e12, 3), "slower_than_semiglobal": round(lo / sg_min - 1, 4)}
        block["semiglobal_spread"] = round(max(ms["semiglobal"]) / sg_min - 1, 4)
        out["device_%s" % ("traceback" if tb else "ends_only")] = block
    swmi.semiglobal_full_release_workspaces()
    swmi.global_full_release_workspaces()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
