#!/usr/bin/env python3
"""What a band of 128 .. 1024 diagonals costs (swmi_banded_width_*_device) beside the 128-wide mixed-shape
entries (swmi_banded_ragged_*_device: the parent commit's code, profiles/banded_width_ab.json) and the full-table affine
aligners on the same resident buffers in one process; writes profiles/banded_width_rate.txt.

Inputs: related pairs (tools/banded_rate.py's: 8 % substitutions, 3 indel runs of 1 - 8 bases, so every path stays in the
narrowest band), parameters (2, -3), open 5, extend 1, the global kind under mask 0.  Results are asserted equal across all
widths and the ragged entry -- every field, and every move up to steps -- before any timing.  Timing: HIP events through the
*_time_device entries (the full-table aligners, which have no such entry for mixed batches: one device call between two events
on the same stream), one untimed call of each side, then `repeats` rounds of one single call of each side -- the ragged entry,
the four widths, the full table -- in turn; the median and the spread (max - min) of each side.

  shapes     1024 x 1024 (65 536 alignments), 4096 x 4096 (4096), 16 384 x 16 384 (1024), both kinds, ends-only and traceback.
  BAR 128    width 128 median <= ragged median + ragged spread + width spread.
  BAR scale  width W median <= (W / 128) ragged median + ragged spread + width spread.
  BAR full   at 4096 and 16 384 every width's median < the full-table affine aligner's on the same pairs (1024: report only).
  report     band cells per second per width; walk time per step at 16 384 (traceback minus ends-only over the mean steps).

    python tools/banded_width_rate.py [--repeats 5] [--scale 1.0] [--out profiles/banded_width_rate.txt]
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
DEV = "cuda:0"


class Batch:
    """n alignments of (length, length) on the device, one set of outputs per side"""

    def __init__(self, a, b):
        self.n, self.length = a.shape
        self.off = (self.length * np.arange(self.n + 1)).astype(np.uint64)
        self.t1, self.t2 = torch.from_numpy(a.reshape(-1)).to(DEV), torch.from_numpy(b.reshape(-1)).to(DEV)
        self.mo = swmi.banded_width.move_offsets(self.off, self.off)
        self.out = {side: Outputs(self.n, int(self.mo[-1])) for side in ("ragged", "width", "full")}

    def tail(self, side, tb):
        o = self.out[side]
        return o.scores, o.ends, o.moves if tb else None, o.steps if tb else None

    def ragged(self, sm, kind, tb):
        return swmi.banded_ragged.time_device(kind, self.t1, self.off, self.t2, self.off, sm, OPEN, EXTEND, 0, *self.tail("ragged", tb), iters=1)

    def width(self, sm, kind, band, tb):
        return swmi.banded_width.time_device(kind, self.t1, self.off, self.t2, self.off, band, sm, OPEN, EXTEND, 0, *self.tail("width", tb), iters=1)

    def full(self, sm, kind, tb):
        """the full-table affine aligner on the same pairs: torch events around one device call"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        p1, p2 = self.t1.data_ptr(), self.t2.data_ptr()
        tail = [None if t is None else t.data_ptr() for t in self.tail("full", tb)]          # (these entries take addresses)
        ev[0].record()
        if kind:
            swmi.global_ragged.global_full_affine_ragged_device(p1, self.off, p2, self.off, sm, OPEN, EXTEND, 0, *tail)
        else:
            swmi.local_full_affine_ragged_device(p1, self.off, p2, self.off, sm, OPEN, EXTEND, *tail)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def same(self, x, y, tb):
        torch.cuda.synchronize()
        a, b = self.out[x].host(), self.out[y].host()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][:, :2], b[1][:, :2]), "scores or end cells differ (%s, %s)" % (x, y)
        if tb:
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), "start cells or steps differ (%s, %s)" % (x, y)
            for k in range(0, self.n, max(1, self.n // 64)):
                same_moves(a[2][int(self.mo[k]):], b[2][int(self.mo[k]):], a[3][k])
            return float(a[3].mean())
        return 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_width_rate.txt"))
    args = ap.parse_args()
    swmi.init(0)
    sm = swmi.match_matrix(MATCH, MISMATCH)
    lines = ["# python tools/banded_width_rate.py --scale %g on one %s: swmi_banded_width_*_device at every width beside" % (args.scale, swmi.device_info()["arch"]),
             "# swmi_banded_ragged_*_device (band 128, the parent's code) and the full-table affine aligners on the same resident pairs,",
             "# (%d, %d) open %d extend %d, related pairs whose paths stay in 128 diagonals, global kind mask 0; every field and move equal" % (MATCH, MISMATCH, OPEN, EXTEND),
             "# before timing; HIP events, one untimed call of each side, then %d alternating single calls; spread = max - min." % args.repeats,
             "# bars: width 128 <= ragged + spreads; width W <= (W / 128) ragged + spreads; every width < full table at 4096 and 16384."]
    failed = False
    for length, n in SHAPES:
        n = max(4, int(n * args.scale))
        batch = Batch(*pairs_of(np.random.default_rng(length), n, length, length))
        for name, kind in KINDS:
            med = {}
            for tb in (False, True):
                what = "%-6s %-9s n %6d %5d^2" % (name, "traceback" if tb else "ends-only", n, length)
                batch.ragged(sm, kind, tb)
                steps = 0.0
                for band in WIDTHS:                                               # untimed, and compared
                    batch.width(sm, kind, band, tb)
                    steps = batch.same("width", "ragged", tb)
                batch.full(sm, kind, tb)
                batch.same("full", "ragged", tb)
                t_r, t_f, t_w = [], [], {band: [] for band in WIDTHS}
                for _ in range(args.repeats):                                     # every side once a round, in turn
                    t_r.append(batch.ragged(sm, kind, tb))
                    for band in WIDTHS:
                        t_w[band].append(batch.width(sm, kind, band, tb))
                    t_f.append(batch.full(sm, kind, tb))
                med_r, spread_r = figures(t_r)
                med_f = figures(t_f)[0]
                lines.append("%s ragged (parent) %s | full table %s" % (what, show(t_r), show(t_f)))
                for band in WIDTHS:
                    med_w, spread_w = figures(t_w[band])
                    med[band, tb] = med_w
                    bar = band / 128.0 * med_r + spread_r + spread_w
                    ok = med_w <= bar
                    below = med_w < med_f
                    failed = failed or not ok or (length >= 4096 and not below)
                    lines.append("%s band %4d %s | x %.2f of ragged | bar %.3f ms: %s | full table: %s | %.1f G band cells/s"
                                 % (what, band, show(t_w[band]), med_w / med_r, bar, "held" if ok else "** MISSED by %.3f ms **" % (med_w - bar),
                                    ("below, x %.1f" % (med_f / med_w)) if below else ("** ABOVE **" if length >= 4096 else "above (report only)"),
                                    n * float(band) * length / (med_w * 1e-3) / 1e9))
                if tb and steps:
                    for band in WIDTHS:
                        lines.append("%s band %4d walk %.1f ns per step (traceback - ends-only over %.0f mean steps; report only)"
                                     % (what, band, (med[band, True] - med[band, False]) * 1e6 / n / steps, steps))
        del batch
        swmi.banded_width.release_workspaces()
        swmi.banded_ragged.release_workspaces()
    lines.append("# every bar held" if not failed else "# a bar was MISSED: see the rows marked **")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
