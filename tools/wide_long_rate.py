#!/usr/bin/env python3
"""Times of the long wide-alphabet aligners (swmi.wide_long, libswmi_wide_long.so) at each shipped stripe
width (swmi.wide_long.STRIPE_WAVES: 1 and 4 wavefronts; 2 was measured once, profiles/wide_long_rate_w124.txt, won no row
and is no longer built) and under the library's own rule (0), beside the 4-letter long affine aligners
(swmi_local_long_affine_device, swmi_global_long_affine_device), in ONE run and on IDENTICAL inputs: DNA letters, the 4 x 4
matrix (2, -3) for the 4-letter side and the same matrix in the corner of a 32 x 32 one for the wide side (filler -64, never
read, so that the global kind's domain rule admits 65536 x 65536), gaps (5, 1), the global kind under mask 0.  The tool asserts
that every side gives the same scores, ends and (with a traceback) steps.

Rows, each ends-only and with a traceback, both kinds: 16384 x 16384 at n = 256 and at n = 8 (few workgroups: latency);
65536 x 65536 at n = 256 ends-only and n = 16 with a traceback; (1024, 8192) at n = 4096 (many short stripes); and a mixed
IUPAC-like batch, 24 letters, both lengths uniform on [2000, 40000], n = 256, wide side only, in GCUPS.

Device entries on resident buffers, HIP events (torch) around `iters` back-to-back calls on one stream, after one untimed call
of each side (it grows the workspaces).  The sides alternate, `repeats` of each; a row reports each side's median in ms, its
cell rate and its spread (max - min) / median.  No rate is fixed in advance.

    python tools/wide_long_rate.py [--iters 1] [--repeats 5] [--out profiles/wide_long_rate.txt] [--scale 1]
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
wl = swmi.wide_long
WIDTHS = tuple(wl.STRIPE_WAVES) + (0,)


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
    """(concatenated seq1s, offsets, seq2s, offsets); every third seq2 starts with a 90 % copy of its seq1's start."""
    cat1 = rng.integers(0, letters, int(np.sum(len1s)) + 16, dtype=np.uint8)
    cat2 = rng.integers(0, letters, int(np.sum(len2s)) + 16, dtype=np.uint8)
    o1, o2 = _offsets(len1s), _offsets(len2s)
    for k in range(0, len(len1s), 3):
        w = int(min(len1s[k], len2s[k]))
        src = cat1[int(o1[k]):int(o1[k]) + w]
        cat2[int(o2[k]):int(o2[k]) + w] = np.where(rng.random(w) < 0.9, src, rng.integers(0, letters, w)).astype(np.uint8)
    return cat1, o1, cat2, o2


class Side:
    """One timed side: its call and result buffers of its own."""

    def __init__(self, name, n, words, tb, dev):
        self.name, self.times = name, []
        self.sc = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self.mv = torch.zeros(max(words, 2), dtype=torch.int64, device=dev) if tb else None
        self.st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
        self.out = (self.sc.data_ptr(), self.ends.data_ptr(), self.mv.data_ptr() if tb else None, self.st.data_ptr() if tb else None)


def row(kind, cat1, off1, cat2, off2, sm32, tb, cells, fixed, repeats, iters):
    """{side: (median ms, spread)} of the wide widths and, where `fixed` = (len1, len2) names the one shape, the 4-letter side."""
    dev = torch.device("cuda:0")
    n = len(off1) - 1
    words = int(wl.move_offsets(off1, off2)[-1])
    d1, d2 = torch.from_numpy(cat1).to(dev), torch.from_numpy(cat2).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    a = (d1.data_ptr(), off1, d2.data_ptr(), off2)
    sides = []
    for w in WIDTHS:
        s = Side("w%d" % w if w else "rule", n, words, tb, dev)

        def call(s=s, w=w):
            wl.set_stripe_waves(w)
            if kind == "local":
                wl.local_device(*a, sm32, *GAPS, *s.out, stream=stream)
            else:
                wl.global_device(*a, sm32, *GAPS, 0, *s.out, stream=stream)
        s.call = call
        sides.append(s)
    if fixed:
        s = Side("4-letter", n, words, tb, dev)
        f = (d1.data_ptr(), fixed[0], d2.data_ptr(), fixed[1], n)
        if kind == "local":
            s.call = lambda s=s: swmi.local_long.local_long_affine_device(*f, SM16, *GAPS, *s.out, stream=stream)
        else:
            s.call = lambda s=s: swmi.global_long.global_long_affine_device(*f, SM16, *GAPS, 0, *s.out, stream=stream)
        sides.append(s)
    for s in sides:
        s.call()
    torch.cuda.synchronize()
    for s in sides[1:]:
        assert torch.equal(s.sc, sides[0].sc) and torch.equal(s.ends, sides[0].ends), (s.name, "differs from", sides[0].name)
        assert not tb or torch.equal(s.st, sides[0].st), (s.name, "steps")
    for _ in range(repeats):
        for s in sides:
            s.times.append(_events(s.call, iters))
    wl.set_stripe_waves(0)
    out = {}
    for s in sides:
        m = statistics.median(s.times)
        out[s.name] = {"ms": round(m, 3), "gcups": round(cells / m / 1e6, 1), "spread": round((max(s.times) - min(s.times)) / m, 3)}
    del sides, d1, d2
    wl.release_workspaces()
    swmi.local_long.local_long_affine_release_workspaces()
    swmi.global_long.global_long_affine_release_workspaces()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every n by this (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_long_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    rng = np.random.default_rng(2026)
    sm32 = np.full((32, 32), -64, np.int8)
    sm32[:4, :4] = np.asarray(SM16, np.int8).reshape(4, 4)
    sm32 = sm32.reshape(-1)
    rows = []

    def run(name, len1s, len2s, letters, sm, fixed, tbs):
        data = batch(len1s, len2s, letters, rng)
        cells = float(np.sum(len1s.astype(np.float64) * len2s))
        for kind in ("local", "global"):
            for tb in tbs:
                r = {"batch": name, "kind": kind, "traceback": tb, "n": len(len1s), "sides": row(kind, *data, sm, tb, cells, fixed, args.repeats, args.iters)}
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)

    def fixed_rows(len1, len2, n, tbs):
        n = max(n // args.scale, 1)
        run("%d x %d" % (len1, len2), np.full(n, len1), np.full(n, len2), 4, sm32, (len1, len2), tbs)

    fixed_rows(16384, 16384, 256, (False, True))
    fixed_rows(16384, 16384, 8, (False, True))
    fixed_rows(65536, 65536, 256, (False,))
    fixed_rows(65536, 65536, 16, (True,))
    fixed_rows(1024, 8192, 4096, (False, True))
    n = max(256 // args.scale, 1)
    pm = rng.integers(-4, 2, (32, 32)).astype(np.int8)
    pm[np.arange(32), np.arange(32)] = rng.integers(4, 12, 32).astype(np.int8)
    run("IUPAC-like 2000..40000, 24 letters", rng.integers(2000, 40001, n), rng.integers(2000, 40001, n), 24, pm.reshape(-1), None, (False, True))

    names = ["w%d" % w for w in wl.STRIPE_WAVES] + ["rule", "4-letter"]
    head = "%-36s %-6s %-3s %5s" % ("batch", "kind", "tb", "n") + "".join(" | %8s ms %7s %5s" % (x, "GCUPS", "sp") for x in names) + " |  best/4l"
    lines = ["long wide-alphabet aligners per stripe width (wN = N wavefronts; rule = the library's own) beside the 4-letter long affine aligners: "
             "tools/wide_long_rate.py --iters %d --repeats %d --scale %d on %s" % (args.iters, args.repeats, args.scale, swmi.device_info()["arch"]),
             "medians of %d alternating repeats after one untimed call; sp = (max - min) / median; best/4l = 4-letter ms / the fastest width's ms "
             "(below 1: the wide call is the slower one)" % args.repeats, "", head]
    for r in rows:
        line = "%-36s %-6s %-3s %5d" % (r["batch"], r["kind"], "yes" if r["traceback"] else "no", r["n"])
        for x in names:
            s = r["sides"].get(x)
            line += " | %11.3f %7.1f %5.3f" % (s["ms"], s["gcups"], s["spread"]) if s else " | %11s %7s %5s" % ("-", "-", "-")
        if "4-letter" in r["sides"]:
            line += " | %8.3f" % (r["sides"]["4-letter"]["ms"] / min(r["sides"][x]["ms"] for x in names[:-2]))
        lines.append(line)
    lines += ["", json.dumps({"metric": "wide_long_rate", "rows": rows})]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-2]))


if __name__ == "__main__":
    main()
