#!/usr/bin/env python3
"""Times of the profile aligners (swmi.wide_profile, libswmi_wide_profile.so) against the wide-alphabet
aligners (swmi.wide, libswmi_wide.so) on the query replicated n times, in one run and on IDENTICAL inputs: a database of n
sequences, one query, a random 32 x 32 matrix with a positive diagonal, the profile swmi.wide_profile.from_sequence(query,
matrix), gaps (7, 1), the global kind under mask 0.  The two sides must then give equal results, which is asserted (scores,
ends, steps) before anything is timed.

Rows: the protein-like database of section 29 (24 letters, lengths log-uniform on [50, 2000], n = 16384) against queries of
300, 1024, 2048 and 4096 columns, and 1024 x 1024 at n = 16384; both kinds, ends-only and with a traceback.  Every third
database sequence holds a noisy copy of a stretch of the query, so that the walks are long.

Device rows: both sides through their own *_time_device entry (HIP events around `iters` calls after one untimed call that
grows the workspace); one untimed call of each first, then `repeats` alternating repeats; a row reports each side's median,
its spread (slowest - fastest of its repeats, in ms), the ratio of the medians, and whether the bar holds: the profile side's
median may exceed the wide side's by no more than the wide side's spread.  A row that misses is reported as measured.

Host rows (the protein-like database only): the host entries by wall clock, the same protocol.  There the wide side also ships
n x len2 bytes of replicated query.  No bar applies to them.

    python tools/wide_profile_rate.py [--n 16384] [--iters 2] [--repeats 5] [--out profiles/wide_profile_rate.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

GAPS = (7, 1)


def _offsets(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def database(len1s, query, letters, rng):
    """(concatenated sequences, offsets) of the given lengths; every third one starts with a 90 % copy of a stretch of the query."""
    cat = rng.integers(0, letters, int(np.sum(len1s)) + 16, dtype=np.uint8)
    off = _offsets(len1s)
    for k in range(0, len(len1s), 3):
        w = int(min(len1s[k], len(query)))
        lo = int(rng.integers(0, len(query) - w + 1))
        cat[int(off[k]):int(off[k]) + w] = np.where(rng.random(w) < 0.9, query[lo:lo + w], rng.integers(0, letters, w)).astype(np.uint8)
    return cat, off


def device_sides(kind, cat, off, query, sm, profile, tb, iters):
    """(time of the profile side, time of the wide side, same_results, what keeps the buffers alive)."""
    dev = torch.device("cuda:0")
    n, len2 = len(off) - 1, len(query)
    off2 = np.arange(n + 1, dtype=np.uint64) * np.uint64(len2)
    mo = swmi.wide_profile.move_offsets(off, len2)
    assert np.array_equal(mo, swmi.local_full_ragged_move_offsets(off, off2))
    d1 = torch.from_numpy(cat).to(dev)
    d2 = torch.from_numpy(np.concatenate([np.tile(query, n), np.zeros(16, np.uint8)])).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    keep, out = [d1, d2], []
    for _ in range(2):
        sc = torch.zeros(n, dtype=torch.int32, device=dev)
        ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        mv = torch.zeros(max(int(mo[-1]), 2), dtype=torch.int64, device=dev) if tb else None
        st = torch.zeros(n, dtype=torch.int32, device=dev) if tb else None
        keep += [sc, ends, mv, st]
        out.append((sc.data_ptr(), ends.data_ptr(), mv.data_ptr() if tb else None, st.data_ptr() if tb else None))
    k = swmi.wide.LOCAL if kind == "local" else swmi.wide.GLOBAL
    prof = lambda: swmi.wide_profile.time_device(k, d1.data_ptr(), off, profile, *GAPS, 0, *out[0], stream=stream, iters=iters)  # noqa: E731
    wide = lambda: swmi.wide.time_device(k, d1.data_ptr(), off, d2.data_ptr(), off2, sm, *GAPS, 0, *out[1], stream=stream, iters=iters)  # noqa: E731
    same = lambda: all(torch.equal(keep[2 + x], keep[6 + x]) for x in ((0, 1, 3) if tb else (0, 1)))  # noqa: E731
    return prof, wide, same, keep


def host_sides(kind, cat, off, query, sm, profile, tb):
    n = len(off) - 1
    replicated = (np.concatenate([np.tile(query, n), np.zeros(16, np.uint8)]), np.arange(n + 1, dtype=np.uint64) * np.uint64(len(query)))
    results = [None, None]

    def timed(which, call):
        t0 = time.perf_counter()
        results[which] = call()
        return (time.perf_counter() - t0) * 1e3

    if kind == "local":
        prof = lambda: timed(0, lambda: swmi.wide_profile.local((cat, off), profile, *GAPS, traceback=tb))  # noqa: E731
        wide = lambda: timed(1, lambda: swmi.wide.local((cat, off), replicated, sm, *GAPS, traceback=tb))  # noqa: E731
    else:
        prof = lambda: timed(0, lambda: swmi.wide_profile.global_((cat, off), profile, *GAPS, 0, traceback=tb))  # noqa: E731
        wide = lambda: timed(1, lambda: swmi.wide.global_((cat, off), replicated, sm, *GAPS, 0, traceback=tb))  # noqa: E731
    same = lambda: all(np.array_equal(results[0][x], results[1][x]) for x in ((0, 1, 3, 4) if tb else (0, 1)))  # noqa: E731
    return prof, wide, same


def measure(prof, wide, same, cells, repeats):
    prof()
    wide()
    torch.cuda.synchronize()
    assert same(), "the two sides disagree on identical inputs"
    tp, tw = [], []
    for _ in range(repeats):
        tp.append(prof())
        tw.append(wide())
    mp, mw = statistics.median(tp), statistics.median(tw)
    return {"profile_ms": round(mp, 3), "wide_ms": round(mw, 3), "wide_over_profile": round(mw / mp, 3),
            "profile_gcups": round(cells / mp / 1e6, 1), "wide_gcups": round(cells / mw / 1e6, 1),
            "profile_spread_ms": round(max(tp) - min(tp), 3), "wide_spread_ms": round(max(tw) - min(tw), 3),
            "bar_met": bool(mp - mw <= max(tw) - min(tw))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_profile_rate.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rng = np.random.default_rng(2032)
    sm = rng.integers(-4, 2, (32, 32)).astype(np.int8)
    sm[np.arange(32), np.arange(32)] = rng.integers(4, 12, 32).astype(np.int8)
    sm = sm.reshape(-1)
    n = args.n
    protein = np.exp(rng.uniform(np.log(50), np.log(2000), n)).astype(np.int64)
    batches = [("protein-like 50..2000 x %d" % len2, protein, len2, True) for len2 in (300, 1024, 2048, 4096)]
    batches.append(("1024 x 1024", np.full(n, 1024), 1024, False))
    rows = []
    for name, len1s, len2, with_host in batches:
        query = rng.integers(0, 24, len2, dtype=np.uint8)
        cat, off = database(len1s, query, 24, rng)
        profile = swmi.wide_profile.from_sequence(query, sm)
        cells = float(np.sum(len1s)) * len2
        for where in (("device", "host") if with_host else ("device",)):
            for kind in ("local", "global"):
                for tb in (False, True):
                    if where == "device":
                        prof, wide, same, keep = device_sides(kind, cat, off, query, sm, profile, tb, args.iters)
                    else:
                        prof, wide, same = host_sides(kind, cat, off, query, sm, profile, tb)
                        keep = None
                    r = measure(prof, wide, same, cells, args.repeats)
                    if where == "host":
                        r["bar_met"] = None
                    r.update(batch=name, where=where, waves=(len2 + 1023) // 1024, kind=kind, traceback=tb, n=n)
                    rows.append(r)
                    print(r, file=sys.stderr, flush=True)
                    del prof, wide, same, keep
                    torch.cuda.empty_cache()
        swmi.wide_profile.release_workspaces()
        swmi.wide.release_workspaces()
    head = "%-30s %-6s %-5s %-6s %-9s %6s %11s %9s %11s %9s %11s %9s %13s %11s %4s" % (
        "batch", "where", "waves", "kind", "traceback", "n", "profile ms", "spread", "wide ms", "spread", "wide/prof", "", "profile GCUPS",
        "wide GCUPS", "bar")
    lines = ["profile aligners against the wide-alphabet aligners on the replicated query: tools/wide_profile_rate.py --n %d --iters %d --repeats %d on %s"
             % (args.n, args.iters, args.repeats, torch.cuda.get_device_properties(0).gcnArchName),
             "medians of %d alternating repeats after one untimed call of each; spread = slowest - fastest of the side's repeats (ms); "
             "wide/prof = wide ms / profile ms (above 1: the profile call is the faster one)" % args.repeats,
             "bar (device rows): profile median - wide median <= wide spread", "", head]
    for r in rows:
        lines.append("%-30s %-6s %-5s %-6s %-9s %6d %11.3f %9.3f %11.3f %9.3f %11.3f %9s %13.1f %11.1f %4s" % (
            r["batch"], r["where"], r["waves"], r["kind"], "yes" if r["traceback"] else "no", r["n"], r["profile_ms"], r["profile_spread_ms"],
            r["wide_ms"], r["wide_spread_ms"], r["wide_over_profile"], "", r["profile_gcups"], r["wide_gcups"],
            "-" if r["bar_met"] is None else "yes" if r["bar_met"] else "NO"))
    lines += ["", json.dumps({"metric": "wide_profile_rate", "rows": rows})]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-2]))


if __name__ == "__main__":
    main()
