#!/usr/bin/env python3
"""Times of the wide-alphabet aligners (swmi.wide, libswmi_wide.so) against the 4-letter mixed-shape
affine aligners (swmi_local_full_affine_ragged_device, swmi_global_full_affine_ragged_device), in one run and on IDENTICAL
inputs: DNA letters, the 4 x 4 matrix (2, -3) for the 4-letter side and swmi.wide.embed_dna of it for the wide side, gaps
(5, 1), the global kind under mask 0.

Shapes: len1 = 1024 against len2 = 300, 1024, 2048 and 4096 (W = 1, 1, 2, 4 wavefronts), n alignments each at W = 1 -- 16384, so
that every CU holds all the wavefronts either kernel's resources allow -- and n / 8 above (the codes of a traceback), ends-only
and with a traceback; every third seq2 is a noisy copy of its seq1, so that the walks are long.  Then a protein-like batch: both lengths
log-uniform on [50, 2000], 24 letters, the wide side under a random 32 x 32 matrix with a positive diagonal; the 4-letter side
runs on the same bytes (it reads them & 3) as a reference for the time of the same shapes, not for the results.

Device entries are timed with HIP events (torch) around `iters` back-to-back calls on one stream, after one warm-up call of
each (it grows the workspaces).  The two sides alternate, `repeats` of each; a row reports the medians in ms, the wide side's
cell rate, the ratio of the medians (4-letter / wide: below 1 the wide call is the slower one) and the spread (max - min) /
median of each side.  No ratio is fixed in advance.

    python tools/wide_rate.py [--n 16384] [--iters 2] [--repeats 5] [--out profiles/wide_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

SM16 = swmi.match_matrix(2, -3)
GAPS = (5, 1)


def _events(call, iters):
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


def batch(len1s, len2s, letters, rng):
    """(concatenated seq1s, seq2s) of the given lengths; every third seq2 starts with a 90 % copy of its seq1's start."""
    cat1 = rng.integers(0, letters, int(np.sum(len1s)) + 16, dtype=np.uint8)
    cat2 = rng.integers(0, letters, int(np.sum(len2s)) + 16, dtype=np.uint8)
    o1, o2 = _offsets(len1s), _offsets(len2s)
    for k in range(0, len(len1s), 3):
        w = int(min(len1s[k], len2s[k]))
        src = cat1[int(o1[k]):int(o1[k]) + w]
        cat2[int(o2[k]):int(o2[k]) + w] = np.where(rng.random(w) < 0.9, src, rng.integers(0, letters, w)).astype(np.uint8)
    return cat1, o1, cat2, o2


def calls(kind, cat1, off1, cat2, off2, sm32, tb):
    """(wide call, 4-letter call, what keeps their buffers alive): the same device inputs, result buffers of their own."""
    dev = torch.device("cuda:0")
    n = len(off1) - 1
    mo = swmi.local_full_ragged_move_offsets(off1, off2)
    d1, d2 = torch.from_numpy(cat1).to(dev), torch.from_numpy(cat2).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    keep, out = [d1, d2], []
    for _ in range(2):
        sc = torch.zeros(n, dtype=torch.int32, device=dev)
        ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        mv = torch.zeros(max(int(mo[-1]), 2), dtype=torch.int64, device=dev) if tb else None
        st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
        keep += [sc, ends, mv, st]
        out.append((sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None))
    a = (d1.data_ptr(), off1, d2.data_ptr(), off2)
    if kind == "local":
        wide = lambda: swmi.wide.local_device(*a, sm32, *GAPS, *out[0], stream=stream)  # noqa: E731
        dna = lambda: swmi.local_full_affine_ragged_device(*a, SM16, *GAPS, *out[1], stream=stream)  # noqa: E731
    else:
        wide = lambda: swmi.wide.global_device(*a, sm32, *GAPS, 0, *out[0], stream=stream)  # noqa: E731
        dna = lambda: swmi.global_ragged.global_full_affine_ragged_device(*a, SM16, *GAPS, 0, *out[1], stream=stream)  # noqa: E731
    return wide, dna, keep


def measure(wide, dna, cells, repeats, iters, same_results=None):
    wide()
    dna()
    torch.cuda.synchronize()
    if same_results is not None:
        assert same_results(), "the two sides disagree on identical inputs"
    tw, td = [], []
    for _ in range(repeats):
        tw.append(_events(wide, iters))
        td.append(_events(dna, iters))
    mw, md = statistics.median(tw), statistics.median(td)
    return {"wide_ms": round(mw, 3), "dna_ms": round(md, 3), "dna_over_wide": round(md / mw, 3), "wide_gcups": round(cells / mw / 1e6, 1),
            "dna_gcups": round(cells / md / 1e6, 1), "wide_spread": round((max(tw) - min(tw)) / mw, 3),
            "dna_spread": round((max(td) - min(td)) / md, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    rng = np.random.default_rng(2026)
    sm32 = swmi.wide.embed_dna(SM16)
    rows = []
    for len2 in (300, 1024, 2048, 4096):
        n = args.n if len2 <= 1024 else max(args.n // 8, 1)
        len1s, len2s = np.full(n, 1024), np.full(n, len2)
        data = batch(len1s, len2s, 4, rng)
        for kind in ("local", "global"):
            for tb in (False, True):
                wide, dna, keep = calls(kind, *data, sm32, tb)
                same = lambda: all(torch.equal(keep[2 + x], keep[6 + x]) for x in ((0, 1, 3) if tb else (0, 1)))  # noqa: E731
                r = measure(wide, dna, float(n) * 1024 * len2, args.repeats, args.iters, same)
                r.update(batch="1024 x %d" % len2, waves=(len2 + 1023) // 1024, kind=kind, traceback=tb, n=n)
                rows.append(r)
                print(r, file=sys.stderr, flush=True)
                del wide, dna, keep
                torch.cuda.empty_cache()
    # protein-like: lengths log-uniform on [50, 2000], 24 letters
    n = args.n
    len1s = np.exp(rng.uniform(np.log(50), np.log(2000), n)).astype(np.int64)
    len2s = np.exp(rng.uniform(np.log(50), np.log(2000), n)).astype(np.int64)
    data = batch(len1s, len2s, 24, rng)
    pm = rng.integers(-4, 2, (32, 32)).astype(np.int8)
    pm[np.arange(32), np.arange(32)] = rng.integers(4, 12, 32).astype(np.int8)
    for kind in ("local", "global"):
        for tb in (False, True):
            wide, dna, keep = calls(kind, *data, pm.reshape(-1), tb)
            r = measure(wide, dna, float(np.sum(len1s * len2s)), args.repeats, args.iters)
            r.update(batch="protein-like 50..2000, 24 letters", waves="1-2", kind=kind, traceback=tb, n=n)
            rows.append(r)
            print(r, file=sys.stderr, flush=True)
            del wide, dna, keep
            torch.cuda.empty_cache()
    head = "%-34s %-5s %-6s %-9s %6s %10s %10s %9s %11s %10s %8s %8s" % ("batch", "waves", "kind", "traceback", "n", "wide ms", "4-letter ms",
                                                                          "4l/wide", "wide GCUPS", "4l GCUPS", "wide sp", "4l sp")
    lines = ["wide-alphabet aligners against the 4-letter mixed-shape affine aligners: tools/wide_rate.py --n %d --iters %d --repeats %d on %s"
             % (args.n, args.iters, args.repeats, swmi.device_info()["arch"]),
             "medians of %d alternating repeats; 4l/wide = 4-letter ms / wide ms (below 1: the wide call is the slower one); sp = (max - min) / median"
             % args.repeats, "", head]
    for r in rows:
        lines.append("%-34s %-5s %-6s %-9s %6d %10.3f %10.3f %9.3f %11.1f %10.1f %8.3f %8.3f" % (
            r["batch"], r["waves"], r["kind"], "yes" if r["traceback"] else "no", r["n"], r["wide_ms"], r["dna_ms"], r["dna_over_wide"],
            r["wide_gcups"], r["dna_gcups"], r["wide_spread"], r["dna_spread"]))
    lines += ["", json.dumps({"metric": "wide_rate", "rows": rows})]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-2]))


if __name__ == "__main__":
    main()
