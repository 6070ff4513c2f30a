#!/usr/bin/env python3
"""What one mixed-shape call of the banded aligners (swmi_banded_ragged_*_device) costs beside the fixed
entries (swmi_banded_local_device, swmi_banded_global_device) on the same resident buffers in one process; writes
profiles/banded_ragged_rate.txt.  The fixed entries' kernel objects are byte-identical to the parent commit's
(profiles/banded_ragged_ab.json), so they are the parent's code.

Everything is taken in one run.  Inputs: related pairs (tools/banded_rate.py's: 8 % substitutions, 3 indel runs of 1 - 8 bases),
parameters (2, -3), open 5, extend 1, the global kind under mask 0.  Results are asserted equal -- every field, and every move up
to steps -- before any timing.  Timing: HIP events through the *_time_device entries, one untimed call of each, then `repeats`
alternating single calls of each side; the median and the spread (max - min) of each side.

  per-call   n = 1, (1, 1): the ragged call's median minus the fixed call's.  It is the slot upload and the host's plan.
  equal      1024 x 1024 (65 536 alignments), 4096 x 4096 (4096), 16 384 x 16 384 (1024), both kinds, ends-only and traceback.
  mixed      16 384 alignments, a quarter each of (300, 300), (1000, 1100), (2048, 2000) and (4096, 4096), interleaved in caller
             order: one ragged call against the four fixed calls, summed.
  THE BAR of the equal and mixed rows: ragged median <= fixed median + per-call term + fixed spread + ragged spread.
  report only: the mixed batch with the planner's sort switched off (a fresh child process: the variable is read once), uniform
  lengths on [64, 4096], and the host entries against one fixed host call per alignment.

    python tools/banded_ragged_rate.py [--repeats 5] [--scale 1.0] [--out profiles/banded_ragged_rate.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libswmi.so: INTEGRATION.md 3)

import swmi  # noqa: E402
from banded_rate import DISTINCT, EXTEND, MATCH, MISMATCH, OPEN, SHAPES, related  # noqa: E402

MIXED = [(300, 300), (1000, 1100), (2048, 2000), (4096, 4096)]
MIXED_N = 16384
KINDS = [("local", 0), ("global", 1)]
DEV = "cuda:0"
SM = None                                   # the matrix, set by main()


def figures(xs):
    return float(np.median(xs)), max(xs) - min(xs)


def show(xs):
    return "median %.3f ms (spread %.3f)" % figures(xs)


def pairs_of(rng, n, len1, len2):
    """n related pairs of (len1, len2): tools/banded_rate.py's pairs of the longer length, cut (a prefix of a related pair is one)"""
    top = max(len1, len2, 8)
    a, b = related(rng, min(n, DISTINCT), top)
    reps = -(-n // len(a))
    return np.tile(a[:, :len1], (reps, 1))[:n].copy(), np.tile(b[:, :len2], (reps, 1))[:n].copy()


class Outputs:
    def __init__(self, n, words):
        self.scores = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.ends = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
        self.moves = torch.zeros(max(words, 2), dtype=torch.int64, device=DEV)
        self.steps = torch.zeros(n, dtype=torch.int32, device=DEV)

    def host(self):
        return self.scores.cpu().numpy(), self.ends.cpu().numpy(), self.moves.cpu().numpy().view(np.uint64), self.steps.cpu().numpy()


def same_moves(got, want, steps):
    """the first `steps` moves of two rows equal"""
    full, part = divmod(int(steps), 32)
    assert np.array_equal(got[:full], want[:full]), "moves differ"
    if part:
        m = np.uint64((1 << (2 * part)) - 1)
        assert (got[full] & m) == (want[full] & m), "moves differ"


class Group:
    """alignments of one (len1, len2) on the device, with the fixed entries' outputs"""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.n, self.len1 = a.shape
        self.len2 = b.shape[1]
        self.ta, self.tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        self.mw = swmi.local_full_move_words(self.len1, self.len2)
        self.out = Outputs(self.n, self.n * self.mw)

    def fixed(self, kind, tb, iters=1):
        o = self.out
        moves = o.moves[:self.n * self.mw].view(self.n, self.mw) if tb else None
        if kind:
            return swmi.banded_global.time_device(self.ta, self.tb, SM, OPEN, EXTEND, o.scores, o.ends, moves, o.steps if tb else None,
                                                  free_ends=0, iters=iters)
        return swmi.banded.time_device(self.ta, self.tb, SM, OPEN, EXTEND, o.scores, o.ends, moves, o.steps if tb else None, iters=iters)


class Ragged:
    """a mixed batch on the device: alignment k = member[k] of groups[which[k]]"""

    def __init__(self, groups, which, member):
        self.groups, self.which, self.member = groups, np.asarray(which), np.asarray(member)
        self.n = len(which)
        len1 = np.array([groups[g].len1 for g in which], np.int64)
        len2 = np.array([groups[g].len2 for g in which], np.int64)
        self.off1 = np.concatenate([[0], np.cumsum(len1)]).astype(np.uint64)
        self.off2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.uint64)
        cat1, cat2 = np.empty(int(self.off1[-1]), np.uint8), np.empty(int(self.off2[-1]), np.uint8)
        for k in range(self.n):
            g = groups[which[k]]
            cat1[int(self.off1[k]):int(self.off1[k + 1])] = g.a[member[k]]
            cat2[int(self.off2[k]):int(self.off2[k + 1])] = g.b[member[k]]
        self.cat1, self.cat2 = cat1, cat2
        self.t1, self.t2 = torch.from_numpy(cat1).to(DEV), torch.from_numpy(cat2).to(DEV)
        self.mo = swmi.banded_ragged.move_offsets(self.off1, self.off2)
        self.out = Outputs(self.n, int(self.mo[-1]))

    def time(self, kind, tb, iters=1):
        o = self.out
        return swmi.banded_ragged.time_device(kind, self.t1, self.off1, self.t2, self.off2, SM, OPEN, EXTEND, 0, o.scores, o.ends,
                                              o.moves if tb else None, o.steps if tb else None, iters=iters)

    def check(self, kind, tb):
        """every field and move of the ragged call equals the fixed calls' (both have just run)"""
        torch.cuda.synchronize()
        sc, ends, moves, steps = self.out.host()
        fixed = [g.out.host() for g in self.groups]
        w, m = self.which, self.member
        for g, f in enumerate(fixed):
            at = np.flatnonzero(w == g)
            assert np.array_equal(sc[at], f[0][m[at]]), "scores differ"
            assert np.array_equal(ends[at][:, :2], f[1][m[at]][:, :2]), "end cells differ"
            if tb:
                assert np.array_equal(ends[at], f[1][m[at]]) and np.array_equal(steps[at], f[3][m[at]]), "start cells or steps differ"
                mw = self.groups[g].mw
                for k in at[:: max(1, len(at) // 256)]:                           # (the batches repeat at most 1024 distinct pairs)
                    same_moves(moves[int(self.mo[k]):], f[2][int(m[k]) * mw:], steps[k])
        if tb:
            assert int(steps.max()) > 0


def measure(ragged, kind, tb, repeats):
    """(ragged times, fixed times summed over the groups) of `repeats` alternating single calls, after one untimed call of each
    whose results are compared"""
    ragged.time(kind, tb)
    for g in ragged.groups:
        g.fixed(kind, tb)
    ragged.check(kind, tb)
    t_r, t_f = [], []
    for _ in range(repeats):
        t_r.append(ragged.time(kind, tb))
        t_f.append(sum(g.fixed(kind, tb) for g in ragged.groups))
    return t_r, t_f


def verdict(t_r, t_f, per_call):
    med_r, spread_r = figures(t_r)
    med_f, spread_f = figures(t_f)
    bar = med_f + max(per_call, 0.0) + spread_f + spread_r
    return med_r <= bar, "ragged %s | fixed %s | ragged / fixed %.3f | bar %.3f ms: %s" % (
        show(t_r), show(t_f), med_r / med_f, bar, "held" if med_r <= bar else "** MISSED by %.3f ms **" % (med_r - bar))


def release():
    swmi.banded_ragged.release_workspaces()
    swmi.banded.release_workspaces()
    swmi.banded_global.release_workspaces()


def mixed_batch(scale):
    rng = np.random.default_rng(37)
    n = max(8, int(MIXED_N * scale)) // 4 * 4
    groups = [Group(*pairs_of(rng, n // 4, len1, len2)) for len1, len2 in MIXED]
    return Ragged(groups, [k % 4 for k in range(n)], [k // 4 for k in range(n)])


def child_unsorted(args):
    """the mixed batch in this (fresh) process, where SWMI_BANDED_RAGGED_NO_SORT=1 is set: one line per (kind, traceback)"""
    batch = mixed_batch(args.scale)
    for name, kind in KINDS:
        for tb in (False, True):
            batch.time(kind, tb)
            t = [batch.time(kind, tb) for _ in range(args.repeats)]
            print("UNSORTED %s %d %s" % (name, int(tb), " ".join("%.4f" % x for x in t)), flush=True)
    return 0


def main():
    global SM
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every batch size (smoke runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "banded_ragged_rate.txt"))
    ap.add_argument("--child-unsorted", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    swmi.init(0)
    SM = swmi.match_matrix(MATCH, MISMATCH)
    if args.child_unsorted:
        return child_unsorted(args)
    lines = ["# python tools/banded_ragged_rate.py on one %s: one swmi_banded_ragged_*_device call beside swmi_banded_local_device /" % swmi.device_info()["arch"],
             "# swmi_banded_global_device (mask 0) on the same resident inputs, (%d, %d) open %d extend %d, related pairs; every field and move" % (MATCH, MISMATCH, OPEN, EXTEND),
             "# equal before timing; HIP events, one untimed call of each, then %d alternating single calls of each; spread = max - min." % args.repeats,
             "# bar: ragged median <= fixed median + per-call term + fixed spread + ragged spread."]
    failed = False
    # the per-call term
    per_call = {}
    one = Ragged([Group(np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8))], [0], [0])
    for name, kind in KINDS:
        for tb in (False, True):
            t_r, t_f = measure(one, kind, tb, args.repeats)
            per_call[(kind, tb)] = figures(t_r)[0] - figures(t_f)[0]
            lines.append("per-call  n      1 (1, 1)        %-6s %-9s ragged %s | fixed %s | per-call term %.3f ms"
                         % (name, "traceback" if tb else "ends-only", show(t_r), show(t_f), per_call[(kind, tb)]))
    release()
    # equal shapes
    for length, n in SHAPES:
        n = max(4, int(n * args.scale))
        rng = np.random.default_rng(length)
        group = Group(*pairs_of(rng, n, length, length))
        batch = Ragged([group], np.zeros(n, np.int64), np.arange(n))
        for name, kind in KINDS:
            for tb in (False, True):
                t_r, t_f = measure(batch, kind, tb, args.repeats)
                ok, text = verdict(t_r, t_f, per_call[(kind, tb)])
                failed = failed or not ok
                lines.append("equal     n %6d %5d x %-5d %-6s %-9s %s | %.1f G band cells/s"
                             % (n, length, length, name, "traceback" if tb else "ends-only", text, n * 128.0 * length / (figures(t_r)[0] * 1e-3) / 1e9))
        del batch, group
        release()
    # mixed shapes
    batch = mixed_batch(args.scale)
    sorted_med = {}
    for name, kind in KINDS:
        for tb in (False, True):
            t_r, t_f = measure(batch, kind, tb, args.repeats)
            ok, text = verdict(t_r, t_f, per_call[(kind, tb)])
            failed = failed or not ok
            sorted_med[(name, int(tb))] = figures(t_r)[0]
            lines.append("mixed     n %6d four shapes    %-6s %-9s %s (fixed: four calls, summed)" % (batch.n, name, "traceback" if tb else "ends-only", text))
    # report only: host to host on a part of the mixed batch, one ragged host call against one fixed host call per alignment
    m = min(batch.n, 512)
    for name, kind in KINDS:
        s1 = (batch.cat1[:int(batch.off1[m])], batch.off1[:m + 1])
        s2 = (batch.cat2[:int(batch.off2[m])], batch.off2[:m + 1])
        call = (lambda x, y: swmi.banded_ragged.global_(x, y, SM, OPEN, EXTEND)) if kind else (lambda x, y: swmi.banded_ragged.local(x, y, SM, OPEN, EXTEND))
        fixed = (lambda x, y: swmi.banded_global.align(x, y, SM, OPEN, EXTEND)) if kind else (lambda x, y: swmi.banded.local(x, y, SM, OPEN, EXTEND))
        call(s1, s2)
        t0 = time.perf_counter()
        res = call(s1, s2)
        t_ragged = time.perf_counter() - t0
        rows = [(batch.groups[batch.which[k]].a[batch.member[k]][None], batch.groups[batch.which[k]].b[batch.member[k]][None]) for k in range(m)]
        fixed(*rows[0])
        t0 = time.perf_counter()
        each = [fixed(x, y) for x, y in rows]
        t_fixed = time.perf_counter() - t0
        assert np.array_equal(res[0], np.array([int(r[0][0]) for r in each])), "host scores differ"
        lines.append("host      n %6d four shapes    %-6s traceback one ragged host call %.1f ms | %d fixed host calls %.1f ms | x %.1f (report only)"
                     % (m, name, t_ragged * 1e3, m, t_fixed * 1e3, t_fixed / t_ragged))
    del batch
    release()
    # report only: the same batch with the planner's sort off, in a fresh process
    env = dict(os.environ, SWMI_BANDED_RAGGED_NO_SORT="1")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-unsorted", "--repeats", str(args.repeats), "--scale", str(args.scale)],
                           env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if child.returncode != 0:
        lines.append("unsorted  the child process failed (exit %d)" % child.returncode)
        failed = True
    for row in child.stdout.splitlines():
        if row.startswith("UNSORTED "):
            f = row.split()
            t = [float(x) for x in f[3:]]
            lines.append("unsorted  four shapes, caller order  %-6s %-9s ragged %s | unsorted / sorted %.3f (report only)"
                         % (f[1], "traceback" if f[2] == "1" else "ends-only", show(t), figures(t)[0] / sorted_med[(f[1], int(f[2]))]))
    # report only: uniform lengths on [64, 4096]
    rng = np.random.default_rng(64)
    n = max(8, int(MIXED_N * args.scale))
    pool = Group(*pairs_of(rng, min(n, DISTINCT), 4096, 4096))
    len1, len2 = rng.integers(64, 4097, n), rng.integers(64, 4097, n)
    off1 = np.concatenate([[0], np.cumsum(len1)]).astype(np.uint64)
    off2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.uint64)
    cat1 = np.concatenate([pool.a[k % pool.n, :len1[k]] for k in range(n)])
    cat2 = np.concatenate([pool.b[k % pool.n, :len2[k]] for k in range(n)])
    t1, t2 = torch.from_numpy(cat1).to(DEV), torch.from_numpy(cat2).to(DEV)
    out = Outputs(n, int(swmi.banded_ragged.move_offsets(off1, off2)[-1]))
    cells = float(np.sum(128.0 * np.minimum(len1, len2 + 64)))
    for name, kind in KINDS:
        for tb in (False, True):
            def run():
                return swmi.banded_ragged.time_device(kind, t1, off1, t2, off2, SM, OPEN, EXTEND, 0, out.scores, out.ends, out.moves if tb else None,
                                                      out.steps if tb else None, iters=1)
            run()
            t = [run() for _ in range(args.repeats)]
            lines.append("uniform   n %6d lengths 64..4096 %-6s %-9s ragged %s | %.1f G band cells/s (report only)"
                         % (n, name, "traceback" if tb else "ends-only", show(t), cells / (figures(t)[0] * 1e-3) / 1e9))
    release()
    lines.append("# every bar held" if not failed else "# a bar was MISSED: see the rows marked **")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
