#!/usr/bin/env python3
"""Alignments per second and TCUPS of the affine global / free-end-gap aligner (swmi_global_full_affine*, DESIGN.md section
21) beside the affine exact semi-global aligner's (swmi_semiglobal_full_affine*, section 16) IN THE SAME RUN; prints ONE
JSON line.

Resident buffers, 256 alignments of 16384 x 16384, score matrix (1, -1), open 3, extend 1, the inputs of tools/sgfull_rate.py
(pairs of the reference's 70 %-identity shape, seeded).  Ends-only and traceback (walk included), for the masks GLOBAL, FIT
and OVERLAP.  The yardstick is the affine semi-global aligner on the same device buffers: in each of `reps` repetitions the
four aligners are timed one after the other (swmi_*_time_device: one untimed call, then HIP events around `iters`
back-to-back device calls), so that whatever else the machine does meets all four alike; the line holds each one's fastest
and slowest repetition, and `semiglobal_spread` = max / min - 1 of the semi-global aligner's own repetitions, the noise
against which `slower_than_semiglobal` = min / semi-global min - 1 is to be read.

Each of the two blocks (ends-only, traceback) runs in a child process of its own under a time limit of its own; the parent
opens no GPU, and after a child that fails or runs out of time it starts nothing more.

    python tools/global_full_affine_rate.py [--n 256] [--reps 5] [--iters 4] [--limit 240]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

OPEN, EXTEND = 3, 1
BLOCKS = ("ends_only", "traceback")


def block(args, tb):
    """One block's measurements, on the GPU: {aligner: {...}, "semiglobal_spread": ...} and the device's name."""
    import numpy as np  # noqa: F401
    import torch  # (before libswmi.so: INTEGRATION.md 3)

    import swmi
    from sgfull_rate import L, pairs
    masks = (("global", swmi.ENDS_GLOBAL), ("fit", swmi.ENDS_FIT), ("overlap", swmi.ENDS_OVERLAP))
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

    def run(name, mask):
        shape = (d1.data_ptr(), L, d2.data_ptr(), L, n, sm, OPEN, EXTEND)
        tail = (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None, 0, args.iters)
        if name == "semiglobal":
            return swmi.semiglobal_full_affine_time_device(*shape, *tail)
        return swmi.global_affine.global_full_affine_time_device(*shape, mask, *tail)

    ms = {name: [] for name in ("semiglobal",) + tuple(m[0] for m in masks)}
    for _ in range(args.reps):
        for name, mask in (("semiglobal", 0),) + masks:
            ms[name].append(run(name, mask))
    sg_min = min(ms["semiglobal"])
    out = {}
    for name, v in ms.items():
        lo, hi = min(v), max(v)
        out[name] = {"ms_min": round(lo, 3), "ms_max": round(hi, 3), "alignments_per_s": round(n / (lo * 1e-3), 1),
                     "tcups": round(n * L * L / (lo * 1e-3) / 1e12, 3), "slower_than_semiglobal": round(lo / sg_min - 1, 4)}
    out["semiglobal_spread"] = round(max(ms["semiglobal"]) / sg_min - 1, 4)
    swmi.semiglobal_full_affine_release_workspaces()
    swmi.global_affine.global_full_affine_release_workspaces()
    return {"shape": [L, L], "device": swmi.device_info()["arch"], "block": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--limit", type=int, default=240, help="seconds each block's child process may take")
    ap.add_argument("--block", choices=BLOCKS, help="(the child's mode) measure this block and print it")
    args = ap.parse_args()
    if args.block:
        print(json.dumps(block(args, args.block == "traceback")))
        return 0
    out = {"metric": "global_full_affine_alignments_per_s", "params": [1, -1, OPEN, EXTEND], "n": args.n, "reps": args.reps,
           "iters": args.iters}
    for name in BLOCKS:
        cmd = [sys.executable, os.path.abspath(__file__), "--block", name, "--n", str(args.n), "--reps", str(args.reps), "--iters",
               str(args.iters)]
        try:
            child = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.stderr.write("block %s ran out of its %d s: nothing more is started\n" % (name, args.limit))
            return 1
        if child.returncode != 0:
            sys.stderr.write("block %s ended with status %d: nothing more is started\n" % (name, child.returncode))
            return 1
        got = json.loads(child.stdout.strip().splitlines()[-1])
        out["shape"], out["device"] = got["shape"], got["device"]
        out["device_" + name] = got["block"]
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
