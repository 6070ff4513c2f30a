#!/usr/bin/env python3
"""Alignments per second of the affine local aligner with traceback (swmi_local_align_affine*); prints
ONE JSON line.

Resident buffers (swmi_local_affine_time_device: HIP events around back-to-back device calls): len1 = 128, 1024 and 16384,
ends-only and traceback; the host entry (swmi_local_align_affine, host arrays in and out) at len1 = 128 with traceback.  Beside
each resident figure, the linear aligner (swmi_local_time_device) on the same buffers and its ratio, so that the comparison
does not depend on another process's clocks.  Inputs: the library's pair generator; for len1 > 128 each seq1 is its generated
128-mer repeated.  Parameters (2, -3), open 5, extend 2 (the linear aligner: gap 5).

    python tools/local_affine_rate.py [--n128 1048576] [--iters 10]
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

OPEN, EXTEND = 5, 2


def device_rates(len1, n, traceback, iters, sm):
    dev = torch.device("cuda:0")
    a, b = swmi.generate_pairs_host(n, 123, 0)
    s1 = np.ascontiguousarray(np.tile(a, (1, (len1 + 127) // 128))[:, :len1])     # seq1 k = seq1 k of the generator, repeated
    d1 = torch.from_numpy(s1).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.local_move_words(len1)), dtype=torch.int64, device=dev) if traceback else None
    st = torch.zeros(n, dtype=torch.int32, device=dev) if traceback else None
    torch.cuda.synchronize()
    bufs = (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if traceback else None, st.data_ptr() if traceback else None, 0, iters)
    ms = swmi.local_affine_time_device(d1.data_ptr(), len1, d2.data_ptr(), n, sm, OPEN, EXTEND, *bufs)
    ms_linear = swmi.local_time_device(d1.data_ptr(), len1, d2.data_ptr(), n, sm, OPEN, *bufs)
    return ms, ms_linear


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n128", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(2, -3)
    out = {"metric": "local_align_affine_alignments_per_s", "params": [2, -3, OPEN, EXTEND], "device": swmi.device_info()["arch"]}
    for len1, n in ((128, args.n128), (1024, max(args.n128 // 8, 1)), (16384, max(args.n128 // 128, 1))):
        for tb in (False, True):
            ms, ms_linear = device_rates(len1, n, tb, args.iters, sm)
            key = "len%d_%s" % (len1, "traceback" if tb else "ends_only")
            out[key] = {"n": n, "ms_per_call": round(ms, 4), "alignments_per_s": round(n / (ms * 1e-3)),
                        "linear_alignments_per_s": round(n / (ms_linear * 1e-3)), "ratio_to_linear": round(ms_linear / ms, 3)}
    a, b = swmi.generate_pairs_host(args.n128, 321, 0)
    swmi.local_align_affine(a[:1024], b[:1024], sm, OPEN, EXTEND)          # buffers and streams set up outside the timing
    t0 = time.perf_counter()
    swmi.local_align_affine(a, b, sm, OPEN, EXTEND)
    dt = time.perf_counter() - t0
    out["len128_host_traceback"] = {"n": args.n128, "ms_per_call": round(dt * 1e3, 3), "alignments_per_s": round(args.n128 / dt)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
