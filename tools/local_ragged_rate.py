#!/usr/bin/env python3
"""Cell rates of the local aligners on batches of mixed seq1 lengths (swmi_local_align_ragged*); prints
ONE JSON line.  Parameters (1, -1, 1) and, for the affine aligner, open = extend = 1.

P1  lengths uniform on [64, 4096], n = 65536, through the ragged device entry, against the fixed-length device entry at
    len1 = 2048 with the same n (ends-only and traceback, linear and affine): cells = 128 * sum of lengths.
P2  equal lengths through the ragged device entry against the fixed one: len1 = 1024 at n = 131072, len1 = 128 at n = 2^20.
P3  P1's inputs through the ragged host entry against one fixed-length host call per distinct length (traceback).

Device entries are timed with torch CUDA events around `iters` back-to-back calls on one stream, after one warm-up call (it
grows the workspaces).  Kernel times alone: run this under rocprofv3 --kernel-trace --stats.

    python tools/local_ragged_rate.py [--iters 5] [--skip-p3]
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


def ragged_device_ms(cat, off, b, affine, tb, iters):
    dev = torch.device("cuda:0")
    n = len(off) - 1
    mo = swmi.local_ragged_move_offsets(off)
    d1 = torch.from_numpy(np.concatenate([cat, np.zeros(16, np.uint8)])).to(dev)
    d2 = torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros(int(mo[-1]), dtype=torch.int64, device=dev) if tb else None
    st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
    stream = torch.cuda.current_stream().cuda_stream
    bufs = (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None)
    if affine:
        call = lambda: swmi.local_align_affine_ragged_device(d1.data_ptr(), off, d2.data_ptr(), SM, 1, 1, *bufs, stream=stream)  # noqa: E731
    else:
        call = lambda: swmi.local_align_ragged_device(d1.data_ptr(), off, d2.data_ptr(), SM, 1, *bufs, stream=stream)  # noqa: E731
    return _events(call, iters)


def fixed_device_ms(len1, n, affine, tb, iters, rng):
    dev = torch.device("cuda:0")
    d1 = torch.from_numpy(rng.integers(0, 4, (n, len1), dtype=np.uint8)).to(dev)
    d2 = torch.from_numpy(rng.integers(0, 4, (n, 128), dtype=np.uint8)).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, swmi.local_move_words(len1)), dtype=torch.int64, device=dev) if tb else None
    st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
    stream = torch.cuda.current_stream().cuda_stream
    bufs = (sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None)
    if affine:
        call = lambda: swmi.local_align_affine_device(d1.data_ptr(), len1, d2.data_ptr(), n, SM, 1, 1, *bufs, stream=stream)  # noqa: E731
    else:
        call = lambda: swmi.local_align_device(d1.data_ptr(), len1, d2.data_ptr(), n, SM, 1, *bufs, stream=stream)  # noqa: E731
    return _events(call, iters)


def ragged_inputs(lens, rng):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 4, int(off[-1]), dtype=np.uint8), off, rng.integers(0, 4, (len(lens), 128), dtype=np.uint8)


def gcells(cells, ms):
    return round(cells / (ms * 1e-3) / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-p3", action="store_true")
    args = ap.parse_args()
    swmi.init(0)
    rng = np.random.default_rng(2024)
    out = {"metric": "local_ragged_gcells_per_s", "params": [1, -1, 1], "device": swmi.device_info()["arch"]}
    n = 65536
    lens = rng.integers(64, 4097, n)
    cat, off, b = ragged_inputs(lens, rng)
    cells = 128 * int(lens.sum())
    for affine in (False, True):
        for tb in (False, True):
            key = "%s_%s" % ("affine" if affine else "linear", "traceback" if tb else "ends_only")
            r_ms = ragged_device_ms(cat, off, b, affine, tb, args.iters)
            f_ms = fixed_device_ms(2048, n, affine, tb, args.iters, rng)
            r, f = gcells(cells, r_ms), gcells(128 * 2048 * n, f_ms)
            out["P1_" + key] = {"ragged_ms": round(r_ms, 3), "ragged_gcells": r, "fixed2048_ms": round(f_ms, 3), "fixed2048_gcells": f,
                                "ratio": round(r / f, 3)}
    for len1, m in ((1024, 131072), (128, 1 << 20)):
        e_cat, e_off, e_b = ragged_inputs(np.full(m, len1), rng)
        for affine in (False, True):
            for tb in (False, True):
                key = "P2_len%d_%s_%s" % (len1, "affine" if affine else "linear", "traceback" if tb else "ends_only")
                r_ms = ragged_device_ms(e_cat, e_off, e_b, affine, tb, args.iters)
                f_ms = fixed_device_ms(len1, m, affine, tb, args.iters, rng)
                out[key] = {"n": m, "ragged_ms": round(r_ms, 3), "fixed_ms": round(f_ms, 3), "time_ratio": round(r_ms / f_ms, 3)}
    if not args.skip_p3:
        a = [cat[int(off[k]):int(off[k + 1])] for k in range(n)]
        for affine in (False, True):
            run = (lambda s1, s2: swmi.local_align_affine_ragged(s1, s2, SM, 1, 1)) if affine else \
                (lambda s1, s2: swmi.local_align_ragged(s1, s2, SM, 1))
            run((cat, off), b)                                              # warm-up (device buffers of the host entry)
            t0 = time.perf_counter()
            run((cat, off), b)
            t_ragged = time.perf_counter() - t0
            groups = {}
            for k, L in enumerate(lens):
                groups.setdefault(int(L), []).append(k)
            t0 = time.perf_counter()
            for L, idx in groups.items():
                s1 = np.stack([a[k] for k in idx])
                if affine:
                    swmi.local_align_affine(s1, b[idx], SM, 1, 1)
                else:
                    swmi.local_align(s1, b[idx], SM, 1)
            t_fixed = time.perf_counter() - t0
            out["P3_%s_traceback" % ("affine" if affine else "linear")] = {
                "ragged_host_s": round(t_ragged, 3), "per_length_calls": len(groups), "per_length_host_s": round(t_fixed, 3),
                "speedup": round(t_fixed / t_ragged, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
