#!/usr/bin/env python3
"""Cells per second of the long semi-global aligners (swmi_semiglobal_long*) at 32768 x 32768 and 65536 x
65536 beside the unchanged fixed-length entries (swmi_semiglobal_full, swmi_semiglobal_full_affine) at 16384 x 16384 IN THE SAME
RUN AND THE SAME PROCESS; prints ONE JSON line.

Resident buffers, score matrix (1, -1) with gap 1, and with open 3 / extend 1 for the affine pair (both inside the domain rule at
65536 x 65536), pairs of the reference's 70 %-identity shape (tools/sgfull_rate.py's recipe at the longer lengths, seeded).
Ends-only every call holds 256 alignments, one workgroup per CU; with a traceback the long entries hold ONE slice
(swmi_semiglobal_long*_slices_for: 64 alignments at 32768 x 32768, 16 at 65536 x 65536), and the fixed entry is timed at 256 and
at those same counts, so that each long row has a comparator with as many workgroups on the card.  In each of `reps` repetitions
every row of a block is timed one after the other (swmi_*_time_device: one untimed call, then HIP events around `iters`
back-to-back device calls); the line holds each row's fastest and slowest repetition and `ratio` = its cells per second / the fixed
entry's at 256 alignments (`ratio_same_n`: / the fixed entry's at the row's own count).

The four blocks (linear / affine x ends-only / traceback) run one after the other in this one process; a block frees its buffers
and both families' workspaces before the next begins.  The caller puts the run under a time limit.

    python tools/semiglobal_long_rate.py [--reps 3] [--iters 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

GAP, OPEN, EXTEND = 1, 3, 1
BLOCKS = ("linear_ends_only", "linear_traceback", "affine_ends_only", "affine_traceback")
FULL = 256                                  # alignments that give every CU a workgroup


def pairs(n, length, seed):
    """tools/sgfull_rate.py's pairs at any length: 10 % substitutions, 5 % of the positions dropped and as many inserted."""
    import numpy as np
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, length), dtype=np.uint8)
    b = a.copy()
    sub = rng.random((n, length)) < 0.10
    b[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
    for k in range(n):
        keep = rng.random(length) >= 0.05
        row = b[k][keep]
        ins = np.sort(rng.integers(0, len(row), length - len(row)))
        b[k] = np.insert(row, ins, rng.integers(0, 4, len(ins), dtype=np.uint8))[:length]
    return a, b


def block(args, affine, tb):
    """One block's rows, on the GPU."""
    import torch  # (before libswmi.so: INTEGRATION.md 3)

    import swmi
    sm = swmi.match_matrix(1, -1)
    gaps = (OPEN, EXTEND) if affine else (GAP,)
    gl = swmi.semiglobal_long
    slices_for = gl.semiglobal_long_affine_slices_for if affine else gl.semiglobal_long_slices_for
    long_timer = gl.semiglobal_long_affine_time_device if affine else gl.semiglobal_long_time_device
    fixed_timer = swmi.semiglobal_full_affine_time_device if affine else swmi.semiglobal_full_time_device
    dev = torch.device("cuda:0")
    rows = []                               # (name, timer, length, n)
    for length in (32768, 65536):
        n = slices_for(1 << 20, length, length, True)[0] if tb else FULL
        rows.append(("long_%d" % length, long_timer, length, n))
    counts = sorted({FULL} | ({r[3] for r in rows} if tb else set()), reverse=True)
    rows = [("fixed_16384_n%d" % c, fixed_timer, 16384, c) for c in counts] + rows
    bufs = {}
    for length in (16384, 32768, 65536):
        n = max(r[3] for r in rows if r[2] == length)
        a, b = pairs(n, length, 1776 + length)
        bufs[length] = (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.zeros(n, dtype=torch.int32, device=dev),
                        torch.zeros((n, 2), dtype=torch.int32, device=dev),
                        torch.zeros((n, gl.move_words(length, length)), dtype=torch.int64, device=dev) if tb else None,
                        torch.zeros(n, dtype=torch.int32, device=dev) if tb else None)
    torch.cuda.synchronize()
    ms = {r[0]: [] for r in rows}
    for _ in range(args.reps):
        for name, timer, length, n in rows:
            d1, d2, sc, ends, mv, st = bufs[length]
            ms[name].append(timer(d1.data_ptr(), length, d2.data_ptr(), length, n, sm, *gaps, sc.data_ptr(),
                                  ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None, 0, args.iters))
    out = {}
    for name, _, length, n in rows:
        lo, hi = min(ms[name]), max(ms[name])
        out[name] = {"n": n, "ms_min": round(lo, 3), "ms_max": round(hi, 3), "tcups": round(n * length * length / (lo * 1e-3) / 1e12, 4)}
    base = out["fixed_16384_n%d" % FULL]["tcups"]
    for name, _, _, n in rows:
        out[name]["ratio"] = round(out[name]["tcups"] / base, 4)
        out[name]["ratio_same_n"] = round(out[name]["tcups"] / out["fixed_16384_n%d" % n]["tcups"], 4)
    del bufs
    torch.cuda.synchronize()
    for release in (gl.semiglobal_long_release_workspaces, gl.semiglobal_long_affine_release_workspaces,
                    swmi.semiglobal_full_release_workspaces, swmi.semiglobal_full_affine_release_workspaces):
        release()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=2)
    args = ap.parse_args()
    import torch  # noqa: F401  (before libswmi.so: INTEGRATION.md 3)

    import swmi
    swmi.init(0)
    out = {"metric": "semiglobal_long_tcups", "params": {"linear": [1, -1, GAP], "affine": [1, -1, OPEN, EXTEND]}, "reps": args.reps,
           "iters": args.iters, "device": swmi.device_info()["arch"]}
    for name in BLOCKS:
        out[name] = block(args, name.startswith("affine"), name.endswith("traceback"))
        sys.stderr.write("%s done\n" % name)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
