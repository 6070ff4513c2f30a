#!/usr/bin/env python3
"""What the banded global / fit / overlap / extension aligner (swmi_banded_global_device) costs beside the
full-table aligners on the same resident buffers in one process; writes profiles/banded_global_rate.txt.

Rows: 1024 x 1024 (65 536 alignments), 4096 x 4096 (4096) and 16 384 x 16 384 (1024), tools/banded_rate.py's shapes, each under
the masks GLOBAL (0) and OVERLAP (15) beside swmi_global_full_affine_device and EXTEND (16) beside
swmi_semiglobal_full_affine_device, ends-only and with a traceback.  Inputs: seq2 = seq1 with 8 % substitutions and 3 indel runs
of 1 - 8 bases (1024 distinct pairs, repeated to fill the batch), parameters (2, -3), open 5, extend 1: every path stays inside
the band, and every field and every move of the two aligners is asserted equal before any timing (EXTEND: score, end cell and
the semi-global aligner's lengths - 1 moves).  Timing: HIP events through the *_time_device entries, one untimed call of each,
then `repeats` alternating single calls of each; the median and the spread (min .. max) of each side.  The only bar: the
banded median lies below the full aligner's on every row (it fills at most 1/8 of the cells).  Report only, no bar: the ratio
to swmi_banded_local_device on the same inputs -- what the borders and the mask cost over the local kernel.

    python tools/banded_global_rate.py [--repeats 5] [--scale 1.0] [--out profiles/banded_global_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402
from banded_rate import DISTINCT, EXTEND, MATCH, MISMATCH, OPEN, SHAPES, related, spread  # noqa: E402

MASKS = [("GLOBAL", 0), ("OVERLAP", 15), ("EXTEND", 16)]


def same_moves(got, want, counts, rows):
    """the first counts[k] moves of rows 0 .. rows - 1 equal"""
    for k in range(rows):
        full_words, part = divmod(int(counts[k]), 32)
        assert np.array_equal(got[k, :full_words], want[k, :full_words]), "moves differ"
        if part:
            mask = (1 << (2 * part)) - 1
            assert (int(got[k, full_words]) & mask) == (int(want[k, full_words]) & mask), "moves differ"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_global_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    bg, bd, ga = swmi.banded_global, swmi.banded, swmi.global_affine
    dev = torch.device("cuda:0")
    sm = swmi.match_matrix(MATCH, MISMATCH)
    lines = ["# python tools/banded_global_rate.py on one %s: swmi_banded_global_device beside swmi_global_full_affine_device (GLOBAL, OVERLAP)"
             % swmi.device_info()["arch"],
             "# and swmi_semiglobal_full_affine_device (EXTEND), resident buffers, (%d, %d) open %d extend %d, related pairs (8 %% substitutions,"
             % (MATCH, MISMATCH, OPEN, EXTEND),
             "# 3 indel runs of 1 - 8), every field and move equal before timing; HIP events, one untimed call of each, then %d alternating"
             % args.repeats,
             "# single calls of each.  global / local: the same call beside swmi_banded_local_device on the same inputs (report only)."]
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
                torch.zeros((n, mw), dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(3)]
        stream = torch.cuda.current_stream().cuda_stream
        for name, mask in MASKS:
            for tb in (False, True):
                def banded(iters, o=out[0]):
                    return bg.time_device(ta, tb_, sm, OPEN, EXTEND, o[0], o[1], o[2] if tb else None, o[3] if tb else None, free_ends=mask,
                                          iters=iters)

                def local(iters, o=out[2]):
                    return bd.time_device(ta, tb_, sm, OPEN, EXTEND, o[0], o[1], o[2] if tb else None, o[3] if tb else None, iters=iters)

                def full(iters, o=out[1]):
                    args_ = (o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr() if tb else None, o[3].data_ptr() if tb else None, stream, iters)
                    if mask == 16:       # (its ends are (n, 2): the first half of the buffer)
                        return swmi.semiglobal_full_affine_time_device(ta.data_ptr(), length, tb_.data_ptr(), length, n, sm, OPEN, EXTEND, *args_)
                    return ga.global_full_affine_time_device(ta.data_ptr(), length, tb_.data_ptr(), length, n, sm, OPEN, EXTEND, mask, *args_)
                banded(1)                                   # the untimed calls; their results are compared
                full(1)
                local(1)
                torch.cuda.synchronize()
                got, want = [[x.cpu().numpy() for x in o] for o in out[:2]]
                rows = min(n, DISTINCT)
                assert np.array_equal(got[0], want[0]), "scores differ"
                if mask == 16:
                    want_ends = want[1].reshape(-1)[:2 * n].reshape(n, 2)
                    assert np.array_equal(got[1][:, :2], want_ends), "end cells differ"
                    if tb:
                        assert not got[1][:, 2:].any() and (got[3] >= want[3] - 1).all(), "start cells or steps differ"
                        same_moves(got[2], want[2], want[3] - 1, rows)
                else:
                    assert np.array_equal(got[1][:, :2], want[1][:, :2]), "end cells differ"
                    if tb:
                        assert np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3]), "start cells or steps differ"
                        same_moves(got[2], want[2], got[3], rows)
                if tb:
                    assert int(got[3].max()) > length // 2
                t_b, t_f, t_l = [], [], []
                for _ in range(args.repeats):
                    t_b.append(banded(1))
                    t_f.append(full(1))
                    t_l.append(local(1))
                med_b, med_f, med_l = (float(np.median(x)) for x in (t_b, t_f, t_l))
                ok = med_b < med_f
                failed = failed or not ok
                lines.append("%5d x %-5d n %6d %-7s %-9s banded %s | full %s | full / banded %.2f | global / local %.2f | %.3f G band cells/s%s"
                             % (length, length, n, name, "traceback" if tb else "ends-only", spread(t_b), spread(t_f), med_f / med_b, med_b / med_l,
                                n * 128.0 * length / (med_b * 1e-3) / 1e9, "" if ok else "  ** NOT BELOW **"))
        ga.global_full_affine_release_workspaces()
        swmi.semiglobal_full_affine_release_workspaces()
        bg.release_workspaces()
        bd.release_workspaces()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
