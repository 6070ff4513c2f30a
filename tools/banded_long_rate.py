#!/usr/bin/env python3
"""What the banded aligners for sequences up to 65536 long cost (swmi_banded_long_*_device) beside the
16384 library's entries (swmi_banded_width_*_device: the parent commit's code, profiles/banded_long_ab.json) and beside the
full-table affine aligners for long sequences, on the same resident buffers in one process; writes profiles/banded_long_rate.txt.

Inputs: related pairs (tools/banded_rate.py's: 8 % substitutions, 3 indel runs of 1 - 8 bases, so every path stays in the
narrowest band), parameters (2, -3), open 5, extend 1, the global kind under mask 0.  Results are asserted equal across the sides
-- every field, and every move up to steps -- before any timing.  Timing: HIP events through the *_time_device entries, one
untimed call of each side, then `repeats` rounds of one single call of each side in turn; the median and the spread (max - min)
of each side.

  BAR parent  1024 x 1024 (65 536 alignments), 4096 x 4096 (4096), 16 384 x 16 384 (1024), each width, both kinds, ends-only and
              traceback: long median <= width median + both spreads.
  BAR full    32 768 x 32 768 and 65 536 x 65 536 (16 alignments): every width's median < swmi_local_long_affine_device's and
              swmi_global_long_affine_device's on the same pairs.
  report      65 536 x 65 536 at n = 1024, each width, beside 4 x the width library's 16 384 x 16 384 row of this run; band cells
              per second; walk time per step (traceback minus ends-only over the mean steps).

    python tools/banded_long_rate.py [--repeats 5] [--scale 1.0] [--out profiles/banded_long_rate.txt]
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
from banded_rate import EXTEND, MATCH, MISMATCH, OPEN, SHAPES  # noqa: E402
from banded_ragged_rate import Outputs, figures, pairs_of, same_moves, show  # noqa: E402

WIDTHS = (128, 256, 512, 1024)
KINDS = [("local", 0), ("global", 1)]
FULL_SHAPES = [(32768, 16), (65536, 16)]
REPORT_SHAPE = (65536, 1024)
DEV = "cuda:0"


class Batch:
    """n alignments of (length, length) on the device, one set of outputs per side"""

    def __init__(self, a, b):
        self.n, self.length = a.shape
        self.off = (self.length * np.arange(self.n + 1)).astype(np.uint64)
        self.t1, self.t2 = torch.from_numpy(a.reshape(-1)).to(DEV), torch.from_numpy(b.reshape(-1)).to(DEV)
        self.mo = swmi.banded_long.move_offsets(self.off, self.off)
        self.out = {side: Outputs(self.n, int(self.mo[-1])) for side in ("long", "other")}

    def tail(self, side, tb):
        o = self.out[side]
        return o.scores, o.ends, o.moves if tb else None, o.steps if tb else None

    def long(self, sm, kind, band, tb):
        return swmi.banded_long.time_device(kind, self.t1, self.off, self.t2, self.off, band, sm, OPEN, EXTEND, 0, *self.tail("long", tb), iters=1)

    def width(self, sm, kind, band, tb):
        return swmi.banded_width.time_device(kind, self.t1, self.off, self.t2, self.off, band, sm, OPEN, EXTEND, 0, *self.tail("other", tb), iters=1)

    def full(self, sm, kind, tb):
        """the full-table affine aligner for long sequences on the same pairs (its moves rows are the same words)"""
        p1, p2 = self.t1.data_ptr(), self.t2.data_ptr()
        tail = [None if t is None else t.data_ptr() for t in self.tail("other", tb)]
        if kind:
            return swmi.global_long.global_long_affine_time_device(p1, self.length, p2, self.length, self.n, sm, OPEN, EXTEND, 0, *tail, iters=1)
        return swmi.local_long.local_long_affine_time_device(p1, self.length, p2, self.length, self.n, sm, OPEN, EXTEND, *tail, iters=1)

    def same(self, tb):
        """the two sides' outputs equal; the mean steps"""
        torch.cuda.synchronize()
        a, b = self.out["long"].host(), self.out["other"].host()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][:, :2], b[1][:, :2]), "scores or end cells differ"
        if tb:
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), "start cells or steps differ"
            for k in range(0, self.n, max(1, self.n // 64)):
                same_moves(a[2][int(self.mo[k]):], b[2][int(self.mo[k]):], a[3][k])
            return float(a[3].mean())
        return 0.0


def rounds(repeats, sides):
    """{name: times} of `repeats` rounds of one call of each side, in turn"""
    times = {name: [] for name, _ in sides}
    for _ in range(repeats):
        for name, call in sides:
            times[name].append(call())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_long_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(MATCH, MISMATCH)
    lines = ["# python tools/banded_long_rate.py --scale %g on one %s: swmi_banded_long_*_device beside swmi_banded_width_*_device" % (args.scale, swmi.device_info()["arch"]),
             "# (the parent's code) and beside swmi_local_long_affine_device / swmi_global_long_affine_device on the same resident pairs,",
             "# (%d, %d) open %d extend %d, related pairs whose paths stay in 128 diagonals, global kind mask 0; every field and move equal" % (MATCH, MISMATCH, OPEN, EXTEND),
             "# before timing; HIP events, one untimed call of each side, then %d alternating single calls; spread = max - min." % args.repeats,
             "# bars: long <= width + both spreads (1024, 4096, 16384); every width < the full table (32768, 65536 at n = 16)."]
    failed = False
    width_16384 = {}
    # ---- against the parent's own code ----
    for length, n in SHAPES:
        n = max(4, int(n * args.scale))
        batch = Batch(*pairs_of(np.random.default_rng(length), n, length, length))
        for name, kind in KINDS:
            for tb in (False, True):
                what = "%-6s %-9s n %6d %5d^2" % (name, "traceback" if tb else "ends-only", n, length)
                for band in WIDTHS:                                               # untimed, and compared
                    batch.width(sm, kind, band, tb)
                    batch.long(sm, kind, band, tb)
                    batch.same(tb)
                sides = []
                for band in WIDTHS:
                    sides.append((("width", band), lambda band=band: batch.width(sm, kind, band, tb)))
                    sides.append((("long", band), lambda band=band: batch.long(sm, kind, band, tb)))
                t = rounds(args.repeats, sides)
                for band in WIDTHS:
                    (med_w, spread_w), (med_l, spread_l) = figures(t["width", band]), figures(t["long", band])
                    bar = med_w + spread_w + spread_l
                    ok = med_l <= bar
                    failed = failed or not ok
                    width_16384[kind, tb, band] = med_w
                    lines.append("%s band %4d width (parent) %s | long %s | x %.3f | bar %.3f ms: %s | %.1f G band cells/s"
                                 % (what, band, show(t["width", band]), show(t["long", band]), med_l / med_w, bar,
                                    "held" if ok else "** MISSED by %.3f ms **" % (med_l - bar), n * float(band) * length / (med_l * 1e-3) / 1e9))
        del batch
        swmi.banded_width.release_workspaces()
        swmi.banded_long.release_workspaces()
    # ---- against the full table ----
    for length, n in FULL_SHAPES:
        n = max(2, int(n * args.scale))
        batch = Batch(*pairs_of(np.random.default_rng(length), n, length, length))
        for name, kind in KINDS:
            for tb in (False, True):
                what = "%-6s %-9s n %6d %5d^2" % (name, "traceback" if tb else "ends-only", n, length)
                batch.full(sm, kind, tb)
                for band in WIDTHS:
                    batch.long(sm, kind, band, tb)
                    batch.same(tb)
                t = rounds(args.repeats, [("full", lambda: batch.full(sm, kind, tb))] +
                           [(band, lambda band=band: batch.long(sm, kind, band, tb)) for band in WIDTHS])
                med_f = figures(t["full"])[0]
                lines.append("%s full table %s" % (what, show(t["full"])))
                for band in WIDTHS:
                    med_l = figures(t[band])[0]
                    below = med_l < med_f
                    failed = failed or not below
                    lines.append("%s band %4d long %s | full table: %s" % (what, band, show(t[band]),
                                                                           ("below, x %.1f: held" % (med_f / med_l)) if below else "** ABOVE: MISSED **"))
        del batch
        swmi.banded_long.release_workspaces()
        swmi.local_long.local_long_affine_release_workspaces()
        swmi.global_long.global_long_affine_release_workspaces()
    # ---- report only ----
    length, n = REPORT_SHAPE
    n = max(4, int(n * args.scale))
    batch = Batch(*pairs_of(np.random.default_rng(length), n, length, length))
    for name, kind in KINDS:
        med = {}
        steps = 0.0
        for tb in (False, True):
            what = "%-6s %-9s n %6d %5d^2" % (name, "traceback" if tb else "ends-only", n, length)
            for band in WIDTHS:
                batch.long(sm, kind, band, tb)
            if tb:
                torch.cuda.synchronize()
                steps = float(batch.out["long"].host()[3].mean())
            t = rounds(args.repeats, [(band, lambda band=band: batch.long(sm, kind, band, tb)) for band in WIDTHS])
            for band in WIDTHS:
                med[band, tb] = figures(t[band])[0]
                lines.append("%s band %4d long %s | x %.2f of the width library's 16384^2 row (4 expected) | %.1f G band cells/s (report only)"
                             % (what, band, show(t[band]), med[band, tb] / width_16384[kind, tb, band], n * float(band) * length / (med[band, tb] * 1e-3) / 1e9))
        for band in WIDTHS:
            lines.append("%-6s %-9s n %6d %5d^2 band %4d walk %.1f ns per step (traceback - ends-only over %.0f mean steps; report only)"
                         % (name, "traceback", n, length, band, (med[band, True] - med[band, False]) * 1e6 / n / steps, steps))
    lines.append("# every bar held" if not failed else "# a bar was MISSED: see the rows marked **")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
