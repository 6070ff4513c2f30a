#!/usr/bin/env python3
"""What the banded local aligner (swmi_banded_local_device) costs beside the full-table affine local
aligner (swmi_local_full_affine_device) on the same resident buffers in one process; writes profiles/banded_rate.txt.

Rows: 1024 x 1024 (65 536 alignments), 4096 x 4096 (4096) and 16 384 x 16 384 (1024), ends-only and with a traceback; and
1024 x 1024 with diagonals NULL beside swmi_score_banded_affine_device under parameters that run its int32 kernel (what the end
cell costs over the bare score).  Inputs: seq2 = seq1 with 8 % substitutions and 3 indel runs of 1 - 8 bases (1024 distinct
pairs, repeated to fill the batch), parameters (2, -3), open 5, extend 1: every path stays inside the band, and every field and
every move of the two aligners is asserted equal before any timing.  Timing: HIP events through the *_time_device entries, one
untimed call of each, then `repeats` alternating single calls of each; the median and the spread (min .. max) of each side.
The only bar: the banded median lies below the full aligner's on every row (it fills at most 1/8 of the cells).

    python tools/banded_rate.py [--repeats 5] [--scale 1.0] [--out profiles/banded_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402

SHAPES = [(1024, 65536), (4096, 4096), (16384, 1024)]
MATCH, MISMATCH, OPEN, EXTEND = 2, -3, 5, 1
DISTINCT = 1024


def related(rng, n, length, sub=0.08, runs=3, max_run=8):
    """seq2 = seq1 with substitutions and a few short indel runs, cut or filled to the same length"""
    a = rng.integers(0, 4, (n, length), dtype=np.uint8)
    b = rng.integers(0, 4, (n, length), dtype=np.uint8)
    for k in range(n):
        src = a[k].copy()
        flip = rng.random(length) < sub
        src[flip] = rng.integers(0, 4, int(flip.sum()), dtype=np.uint8)
        parts, at = [], 0
        for c in sorted(int(x) for x in rng.integers(1, length - 1, runs)):
            g = int(rng.integers(1, max_run + 1))
            parts.append(src[at:c])
            if rng.random() < 0.5:
                parts.append(rng.integers(0, 4, g, dtype=np.uint8))
                at = c
            else:
                at = min(length, c + g)
        parts.append(src[at:])
        out = np.concatenate(parts)[:length]
        b[k, :len(out)] = out
    return a, b


def spread(xs):
    return "median %.3f ms (min %.3f, max %.3f)" % (float(np.median(xs)), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    bd = swmi.banded
    dev = torch.device("cuda:0")
    sm = swmi.match_matrix(MATCH, MISMATCH)
    lines = ["# python tools/banded_rate.py on one %s: swmi_banded_local_device beside swmi_local_full_affine_device, resident buffers,"
             % swmi.device_info()["arch"],
             "# (%d, %d) open %d extend %d, related pairs (8 %% substitutions, 3 indel runs of 1 - 8), every field and move equal before timing;"
             % (MATCH, MISMATCH, OPEN, EXTEND),
             "# HIP events, one untimed call of each, then %d alternating single calls of each." % args.repeats]
    failed = False
    for length, n in SHAPES:
        n = max(4, int(n * args.scale))
        rng = np.random.default_rng(length)
        a, b = related(rng, min(n, DISTINCT), length)
        reps = -(-n // len(a))
        a, b = np.tile(a, (reps, 1))[:n], np.tile(b, (reps, 1))[:n]
        ta, tb_ = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        mw = swmi.local_full_move_words(length, length)
        out = [(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, 4), dtype=torch.int32, device=dev),
                torch.zeros((n, mw), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(2)]
        for tb in (False, True):
            def banded(iters, o=out[0]):
                return bd.time_device(ta, tb_, sm, OPEN, EXTEND, o[0], o[1], o[2] if tb else None, o[3] if tb else None, iters=iters)

            def full(iters, o=out[1]):
                return swmi.local_full_affine_time_device(ta.data_ptr(), length, tb_.data_ptr(), length, n, sm, OPEN, EXTEND, o[0].data_ptr(),
                                                          o[1].data_ptr(), o[2].data_ptr() if tb else None, o[3].data_ptr() if tb else None,
                                                          torch.cuda.current_stream().cuda_stream, iters)
            banded(1)                                   # the untimed calls; their results are compared
            full(1)
            torch.cuda.synchronize()
            got, want = [[x.cpu().numpy() for x in o] for o in out]
            assert np.array_equal(got[0], want[0]), "scores differ"
            assert np.array_equal(got[1][:, :2], want[1][:, :2]), "end cells differ"
            if tb:
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]), "start cells or steps differ"
                words = (got[3].astype(np.int64) + 31) // 32
                for k in range(min(n, DISTINCT)):
                    full_words, part = divmod(int(got[3][k]), 32)
                    assert np.array_equal(got[2][k, :full_words], want[2][k, :full_words]), "moves differ"
                    if part:
                        mask = (1 << (2 * part)) - 1
                        assert (int(got[2][k, full_words]) & mask) == (int(want[2][k, full_words]) & mask), "moves differ"
                assert int(words.max()) > length // 40
            t_b, t_f = [], []
            for _ in range(args.repeats):
                t_b.append(banded(1))
                t_f.append(full(1))
            ratio = float(np.median(t_f)) / float(np.median(t_b))
            ok = float(np.median(t_b)) < float(np.median(t_f))
            failed = failed or not ok
            mode = "traceback" if tb else "ends-only"
            lines.append("%5d x %-5d n %6d %-9s banded %s | full %s | full / banded %.2f | %.3f G band cells/s%s"
                         % (length, length, n, mode, spread(t_b), spread(t_f), ratio,
                            n * 128.0 * length / (float(np.median(t_b)) * 1e-3) / 1e9, "" if ok else "  ** NOT BELOW **"))
            if tb:
                stored = n * 64.0 * (length + 64)
                lines.append("        codes stored: %.2f GB per call = %.3f TB/s over the whole call" % (stored / 1e9, stored / (float(np.median(t_b)) * 1e-3) / 1e12))
        swmi.local_full_affine_release_workspaces()
        bd.release_workspaces()
        if length == 1024:
            # what the end cell costs over the bare score: the scorer's int32 kernel (match 32: 1024 * 32 >= 2^15)
            sm32 = swmi.match_matrix(32, -48)
            name = swmi.banded_affine_kernel_for(length, sm32, OPEN, EXTEND)[0]
            assert name == "sw_banded_affine_kernel<1,0>", name
            sc = torch.zeros(n, dtype=torch.int32, device=dev)

            def scorer():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                swmi.score_banded_affine_device(ta.data_ptr(), tb_.data_ptr(), n, length, sm32, OPEN, EXTEND, sc.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            def ends_only(iters):
                return bd.time_device(ta, tb_, sm32, OPEN, EXTEND, out[0][0], out[0][1], iters=iters)
            scorer()
            ends_only(1)
            torch.cuda.synchronize()
            assert np.array_equal(sc.cpu().numpy(), out[0][0].cpu().numpy()), "scores differ from the scorer's"
            t_b, t_s = [], []
            for _ in range(args.repeats):
                t_b.append(ends_only(1))
                t_s.append(scorer())
            lines.append("%5d x %-5d n %6d diagonals NULL, (32, -48): banded ends-only %s | %s %s | banded / scorer %.2f (report only)"
                         % (length, length, n, spread(t_b), name, spread(t_s), float(np.median(t_b)) / float(np.median(t_s))))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
