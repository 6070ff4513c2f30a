#!/usr/bin/env python3
"""Long-running differential fuzz of the GPU scorer against the CPU oracle (and the real reference where present) --
the reference's own TestSimdSmithWaterman idea (source.cpp:2943-2982: fresh random pairs until bored), at GPU scale.

    python tests/fuzz_parity.py --seconds 240            # on the GPU box; writes a summary line per parameter set

Every round generates a fresh batch on the device (counter-based generator, new seed), scores it through the C ABI,
copies the inputs back and scores them with oracle/liboracle.so on all host cores (OpenMP); any mismatch is dumped.
A second phase does the same for the semi-global aligner against the reference's simd_mark4 (full tracebacks); a third
one for the banded affine extension against the oracle's scalar Gotoh (random lengths, matrices, open / extend, and the
shifted copies and gap runs of tests/banded_edges.py on the band's edge diagonals); a fourth
and a fifth for the local aligner and the exact semi-global aligner against their C restatements (tests/native/
local_oracle.c, sgfull_oracle.c): shapes from the grids of tests/table_edges.py and the inputs built there, every field;
a sixth and a seventh for the affine local aligner and the affine exact semi-global aligner against theirs
(local_affine_oracle.c, sgfull_affine_oracle.c): the grids and inputs of tests/affine_edges.py, random (open, extend) of
every family (extend < open, open < extend, either or both 0)."""
import argparse, ctypes, os, sys, time
from concurrent.futures import ThreadPoolExecutor
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # tests/ lives one level below the repo root
sys.path.insert(0, os.path.join(ROOT, "smith-waterman-simd_amd"))
import swmi, torch

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=120)
ap.add_argument("--batch", type=int, default=1 << 22)
ap.add_argument("--sg-seconds", type=float, default=60)
ap.add_argument("--ba-seconds", type=float, default=30)
ap.add_argument("--local-seconds", type=float, default=30)
ap.add_argument("--sgfull-seconds", type=float, default=60)
ap.add_argument("--local-affine-seconds", type=float, default=30)
ap.add_argument("--sgfull-affine-seconds", type=float, default=60)
args = ap.parse_args()
swmi.init(0)
vp = ctypes.c_void_p
orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
rng = np.random.default_rng(int(time.time()))
n = args.batch
d1 = torch.empty(n * 128, dtype=torch.uint8, device="cuda"); d2 = torch.empty(n * 128, dtype=torch.uint8, device="cuda")
out = torch.empty(n, dtype=torch.int32, device="cuda")
st = torch.cuda.current_stream().cuda_stream
t_end = time.time() + args.seconds
total = mism = rounds = 0
while time.time() < t_end:
    seed = int(rng.integers(0, 2**62)); first = int(rng.integers(0, 2**40))
    kind = rounds % 5
    if kind == 0: sm = swmi.match_matrix(10, -30); gap = 15
    elif kind == 1: sm = swmi.match_matrix(1, -1); gap = 1
    elif kind == 2: sm = rng.integers(-128, 128, 16).astype(np.int8); gap = int(rng.integers(0, 128))
    elif kind == 3: sm = rng.integers(-12, 13, 16).astype(np.int8); gap = int(rng.integers(0, 9))
    else:                    # every score + 2 gap in [0, 255], some score + gap < 0: the packed kernel's vertical-offset cell
        gap = int(rng.integers(1, 65))   # up to 64, where -128 + 2 gap = 0 and 127 + 2 gap = 255: both ends of the row byte
        sm = rng.integers(-2 * gap, min(127, 255 - 2 * gap) + 1, 16).astype(np.int8)
        lo_at, hi_at = (int(k) for k in rng.choice(16, 2, replace=False))
        sm[lo_at] = -2 * gap
        if 255 - 2 * gap <= 127: sm[hi_at] = 255 - 2 * gap
    L = [4, 4, 8, 4, 16, 2, 4, 32, 64][rounds % 9]      # L = 4 (the packed kernel unless a flag says otherwise) meets every parameter family
    swmi.set_schedule(L, int((0, 0, 1, 8)[int(rng.integers(0, 4))]))
    swmi.generate_pairs_device(d1.data_ptr(), d2.data_ptr(), n, seed, first, st)
    if rounds % 3 == 1:      # make half of the batch related pairs (mutated copies) so that long alignments occur
        m = torch.rand(n * 128, device="cuda") < 0.85
        half = (n // 2) * 128
        d2[:half] = torch.where(m[:half], d1[:half], d2[:half])
    entry = rounds % 5                   # the sibling entry points share the kernel template: MODE 0 / 1 / 2
    if entry == 3:                       # 2-bit packed inputs (source.cpp:1581), packed on the device
        def pack(d):
            v = d.view(n, 32, 4).to(torch.int32)
            return (v[..., 0] | (v[..., 1] << 2) | (v[..., 2] << 4) | (v[..., 3] << 6)).to(torch.uint8).contiguous()
        p1, p2 = pack(d1), pack(d2)
        swmi.score_batch_device(p1.data_ptr(), p2.data_ptr(), n, sm, gap, out.data_ptr(), st, packed=True)
    elif entry == 4:                     # every seq1 against ONE seq2 (source.cpp:1227)
        d2.view(n, 128)[:] = d2[:128].clone()
        swmi.score_one_vs_many_device(d1.data_ptr(), n, d2.data_ptr(), sm, gap, out.data_ptr(), st)
    else:
        swmi.score_batch_device(d1.data_ptr(), d2.data_ptr(), n, sm, gap, out.data_ptr(), st)
    torch.cuda.synchronize()
    a = d1.cpu().numpy(); b = d2.cpu().numpy(); got = out.cpu().numpy()
    want = np.zeros(n, np.int32)
    orc.sw_oracle_batch(a.ctypes.data_as(vp), b.ctypes.data_as(vp), ctypes.c_size_t(n), sm.ctypes.data_as(vp), gap, want.ctypes.data_as(vp))
    bad = int((got != want).sum())
    total += n; mism += bad; rounds += 1
    if bad:
        i = int(np.nonzero(got != want)[0][0])
        print("MISMATCH seed %d first %d L %d gap %d sm %s: pair %d got %d want %d (%d bad)" % (seed, first, L, gap, sm.tolist(), i, got[i], want[i], bad), flush=True)
    if rounds % 10 == 0:
        print("... %d rounds, %.0f M pairs, %d mismatches" % (rounds, total / 1e6, mism), flush=True)
print("SW128 fuzz: %d rounds, %d pairs, %d mismatches (all six schedules, folded and general cell, five parameter families, pairs / packed / one-vs-many entries)" % (rounds, total, mism), flush=True)

# ---- semi-global aligner against the real reference (if present) or the oracle --------------------------------------
ref_path = os.path.join(ROOT, "oracle", "_ref", "libswref.so")
ref = ctypes.CDLL(ref_path) if os.path.exists(ref_path) else None
t_end = time.time() + args.sg_seconds
sg_total = sg_bad = sg_simd_off = 0
workers = min(64, os.cpu_count() or 8)
def check(arg):
    """0: the GPU's result is the reference's; 1: it is not; 2: it is the scalar reference's (and the oracle's) but not simd_mark4's --
    the reference's SIMD variants drop a cell that holds exactly best - 70 (the scalar function keeps it, source.cpp:1938-1941), so on
    the no-match stretches below they end alignments the scalar function carries on: counted apart, the scalar function is what
    the library replaces."""
    a, b, score, tb = arg
    buf = np.zeros((32769, 2), np.int32); sc = ctypes.c_int32(); ln = ctypes.c_size_t()
    oob = ctypes.c_int()
    same = lambda: sc.value == score and ln.value == len(tb) and np.array_equal(buf[: ln.value], tb)
    orc.sg_oracle_xdrop(a.ctypes.data_as(vp), b.ctypes.data_as(vp), ctypes.byref(sc), buf.ctypes.data_as(vp), ctypes.c_size_t(32769), ctypes.byref(ln), ctypes.byref(oob))
    if ref is None or oob.value:              # (where the reference reads past its pads -- touched_oob, shifted starts get there -- the oracle's "pad" is the definition)
        return 0 if same() else 1
    ref.swref_semiglobal(4, a.ctypes.data_as(vp), b.ctypes.data_as(vp), ctypes.byref(sc), buf.ctypes.data_as(vp), ctypes.c_size_t(32769), ctypes.byref(ln))
    if same():
        return 0
    ref.swref_semiglobal(0, a.ctypes.data_as(vp), b.ctypes.data_as(vp), ctypes.byref(sc), buf.ctypes.data_as(vp), ctypes.c_size_t(32769), ctypes.byref(ln))
    return 2 if same() else 1
sg_iter = 0
while time.time() < t_end:
    m = 2048 - 17 * (sg_iter % 4)        # ragged batches too: the last sweep wavefront is partly filled (interleaved streams, tail lanes)
    a = rng.integers(0, 4, (m, 16384), dtype=np.uint8)
    p = rng.random((m, 1)) * 0.3
    b = np.where(rng.random((m, 16384)) < p, rng.integers(0, 4, (m, 16384), dtype=np.uint8), a).astype(np.uint8)
    for k in range(0, m, 7):             # indels: shift a tail of some sequences by a few bases
        cut = int(rng.integers(100, 16000)); sh = int(rng.integers(1, 40))
        b[k, cut:] = np.roll(b[k], sh)[cut:]
    for k in range(3, m, 5):             # runs of guaranteed mismatches around the X-drop limit of 70: some alignments die there, some
        for _ in range(int(rng.integers(1, 5))):        # scrape past -- cells at the threshold, dropped cells, dead lanes beside live ones
            lo = int(rng.integers(50, 16200)); run = int(rng.integers(30, 111))
            b[k, lo: lo + run] = (a[k, lo: lo + run] + 1 + (rng.integers(0, 3, len(a[k, lo: lo + run])) if rng.random() < 0.5 else 0)) & 3
    for k in range(1, m, 11):            # stretches that match at NO offset (0 against 1), 60 .. 80 long: the whole band sinks to the threshold,
        for _ in range(int(rng.integers(1, 4))):        # cells at exactly best - 70 beside dropped ones (tests/sg_edges.py has the fixed cases)
            lo = int(rng.integers(50, 16200)); run = int(rng.integers(60, 81))
            a[k, lo: lo + run] = 0; b[k, lo: lo + run] = 1
    for k in range(2, m, 13):            # shifted starts of 1 .. 31: the path begins in the outer cells of the band, either side
        sh = int(rng.integers(1, 32)); fill = rng.integers(0, 4, sh, dtype=np.uint8)
        b[k] = np.concatenate([b[k, sh:], fill]) if rng.random() < 0.5 else np.concatenate([fill, b[k, : 16384 - sh]])
    swmi.semiglobal_set_exact(sg_iter % 5 == 4)          # every fifth batch on the exact path only (no calm windows)
    swmi.semiglobal_set_mapping((41, 42, 43, 44, 21, 22, 23, 11, 12)[sg_iter % 9])
    sg_iter += 1
    if sg_iter % 2:                      # the entry that returns the walk's 2-bit moves, expanded on the host (round 4)
        scores, moves, lengths = swmi.semiglobal_xdrop_moves(a, b)
        tbs = [swmi.semiglobal_expand_moves(moves[k], int(lengths[k])) for k in range(m)]
    else:
        scores, tbs, lengths = swmi.semiglobal_xdrop(a, b)
    with ThreadPoolExecutor(workers) as ex:
        ok = list(ex.map(check, [(a[k], b[k], int(scores[k]), tbs[k]) for k in range(m)]))
    sg_total += m; sg_bad += ok.count(1); sg_simd_off += ok.count(2)
    print("... semi-global %d alignments, %d mismatches (%d where simd_mark4 leaves the scalar reference)" % (sg_total, sg_bad, sg_simd_off), flush=True)
swmi.semiglobal_set_exact(False)
print("semi-global fuzz vs %s: %d alignments (score + full traceback; positions entry and moves entry + host expansion in turn), %d mismatches; %d more where the reference's simd_mark4 differs from its scalar function and the GPU has the scalar's result" % ("reference simd_mark4, then scalar" if ref else "oracle", sg_total, sg_bad, sg_simd_off), flush=True)

# ---- banded affine extension vs oracle/sw_oracle.c (no reference counterpart: parity unpinned by the reference) ----
import banded_edges as be
orc.sw_oracle_banded_affine.restype = ctypes.c_int
ba_total = ba_bad = 0
ba_kernels = {}
ba_edges = {}
t_end = time.time() + args.ba_seconds
while time.time() < t_end:
    length = int(rng.choice([64, 65, 100, 128, 200, 333, 512, 1000, 1024, 1500, 1792]))
    m = int(rng.integers(1, 40))
    a = rng.integers(0, 4, (m, length), dtype=np.uint8)
    p = rng.random((m, 1)) * 0.4
    b = np.where(rng.random((m, length)) < p, rng.integers(0, 4, (m, length), dtype=np.uint8), a).astype(np.uint8)
    for k in range(0, m, 3):             # indels: offsets up to and beyond the band
        cut = int(rng.integers(1, length)); sh = int(rng.integers(1, 80))
        b[k, cut:] = np.roll(b[k], sh)[cut:]
    if length >= 100:                    # the band's edges (banded_edges.py): a copy on, or one gap run onto, diagonal -66 .. -62 / 62 .. 65
        for k in range(1, m, 3):
            s = int(rng.choice(be.SHIFTS))
            if length < 200 or rng.random() < 0.5:
                a[k], b[k] = be.shifted_pair(rng, length, s)
                edge = "shift %+d" % s
            else:
                a[k], b[k] = be.gap_run_pair(rng, length, abs(s), s > 0)
                edge = "%s %d" % ("insert" if s > 0 else "delete", abs(s))
            ba_edges[edge] = ba_edges.get(edge, 0) + 1
    kind = int(rng.integers(0, 4))       # any int8 matrix / match-mismatch with any gaps / the usual small gaps / small scores, any gaps
    if kind == 3:                        # scores small enough for the packed kernel at every length, either sign
        sm = rng.integers(-128 if rng.random() < 0.3 else -12, 15, 16).astype(np.int8)
    else:
        sm = (rng.integers(-128, 128, 16) if kind == 0 else
              np.where(np.eye(4, dtype=bool), rng.integers(0, 128), rng.integers(-128, 1)).reshape(16)).astype(np.int8)
    go, ge = (int(rng.integers(0, 20)), int(rng.integers(0, 8))) if kind == 2 else (int(rng.integers(0, 128)), int(rng.integers(0, 128)))
    ba_kernels[swmi.banded_affine_kernel_for(length, sm, go, ge)[0]] = ba_kernels.get(swmi.banded_affine_kernel_for(length, sm, go, ge)[0], 0) + m
    got = swmi.score_banded_affine(a, b, sm, go, ge)
    want = np.array([orc.sw_oracle_banded_affine(a[k].ctypes.data_as(vp), b[k].ctypes.data_as(vp), length, sm.ctypes.data_as(vp), go, ge)
                     for k in range(m)], np.int32)
    ba_total += m; ba_bad += int((got != want).sum())
print("banded affine fuzz vs oracle: %d alignments, %d mismatches (11 lengths 64..1792, random matrices, open/extend 0..127 either order); per kernel: %s" % (
    ba_total, ba_bad, ", ".join("%s %d" % kv for kv in sorted(ba_kernels.items()))), flush=True)
print("... of which at the band's edges: %s" % ", ".join("%s: %d" % kv for kv in sorted(ba_edges.items())), flush=True)

# ---- the table aligners vs their C restatements: grid shapes, random shapes, the constructed edge inputs ---------------
import tempfile
import table_edges as te
import affine_edges as ae
from local_affine_support import AffineOracle
from local_support import LocalOracle
from sgfull_affine_support import SgAffineOracle
from sgfull_support import SgFullOracle
_tmp = tempfile.mkdtemp()
lorc, sorc, laorc, saorc = LocalOracle(_tmp), SgFullOracle(_tmp), AffineOracle(_tmp), SgAffineOracle(_tmp)


def table_params():
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return rng.integers(-128, 128, 16).astype(np.int8), int(rng.integers(0, 128))
    if kind == 1:
        return rng.integers(-12, 13, 16).astype(np.int8), int(rng.integers(0, 9))
    if kind == 2:                        # ties are common
        return rng.integers(-1, 2, 16).astype(np.int8), int(rng.integers(0, 2))
    return swmi.match_matrix(int(rng.integers(1, 128)), -int(rng.integers(0, 129))), int(rng.integers(0, 128))


def affine_params():
    """a matrix of table_params and (open, extend) of one family: extend < open, open < extend, any, (g, 0), (0, g), (0, 0)"""
    sm, g = table_params()
    family = int(rng.integers(0, 6))
    h = int(rng.integers(0, 128)) if g > 8 else int(rng.integers(0, 9))
    return sm, ((max(g, h), min(g, h)), (min(g, h), max(g, h)), (g, h), (g, 0), (0, g), (0, 0))[family]


def table_round(kind, cases, draw, count_offset):
    """one batch: a constructed case (its own parameters, or random ones) every third round, else a drawn shape; returns
    (alignments, mismatching alignments).  gap: one penalty (the linear aligners) or (open, extend) (the affine ones)."""
    global table_iter
    table_iter += 1
    affine = kind.endswith("_affine")
    params = affine_params if affine else table_params
    if table_iter % 3 == 0:
        case = cases[int(rng.integers(0, len(cases)))]
        a, b = case.a, case.b
        sm, gap = (case.sm, case.gaps if affine else case.gap) if rng.random() < 0.5 else params()
    else:
        (a, b), (sm, gap) = draw(), params()
    tb = bool(rng.random() < 0.75)
    if kind.startswith("local"):
        got, want = (swmi.local_align_affine(a, b, sm, *gap, traceback=tb), laorc.align(a, b, sm, *gap)) if affine else \
            (swmi.local_align(a, b, sm, gap, traceback=tb), lorc.align(a, b, sm, gap))
        if not tb:
            got, want = (got[0], got[1][:, :2], None, None), (want[0], want[1][:, :2], None, None)
    elif affine:
        got, want = swmi.semiglobal_full_affine(a, b, sm, *gap, traceback=tb), saorc.align(a, b, sm, *gap, traceback=tb)
    else:
        got, want = swmi.semiglobal_full(a, b, sm, gap, traceback=tb), sorc.align(a, b, sm, gap, traceback=tb)
    bad = 0
    while True:                          # count every mismatching alignment, report the first
        diff = te.first_difference(got, want, count_offset, tb)
        if diff is None:
            break
        field, k = diff
        if bad == 0:
            print("MISMATCH %s %dx%d gap %s sm %s traceback %d: alignment %d %s" % (kind, a.shape[1], b.shape[1], gap, np.asarray(sm).tolist(),
                                                                                 tb, k, field), flush=True)
        bad += 1
        keep = np.arange(len(got[0])) != k
        got = tuple(None if x is None else x[keep] for x in got)
        want = tuple(None if x is None else x[keep] for x in want)
        a, b = a[keep], b[keep]
    return len(a) + bad, bad


def draw_local(len1s=te.LOC_LEN1, ns=te.LOC_N):
    len1 = int(rng.choice(len1s)) if rng.random() < 0.6 else int(rng.integers(1, te.LOC_MAX_LEN + 1))
    n = int(rng.choice(ns)) if len1 > 4096 else int(rng.integers(1, 300))
    return te.local_mixed_pairs(n, len1, int(rng.integers(0, 2**62)))


def draw_sgfull(grid=te.sg_shape_grid()):
    if rng.random() < 0.5:
        len1, len2, n = grid[int(rng.integers(0, len(grid)))]
    else:
        len1, len2 = int(rng.integers(1, te.SG_MAX_LEN + 1)), int(rng.integers(1, te.SG_MAX_LEN + 1))
        while len1 * len2 > 1 << 26:
            len1, len2 = max(1, len1 // 2), max(1, len2 // 2)
        n = max(1, min(16, (1 << 25) // (len1 * len2)))
    return te.sg_mixed_pairs(n, len1, len2, int(rng.integers(0, 2**62)))


table_iter = 0
for kind, seconds, cases, draw, offset in (
        ("local", args.local_seconds, lambda: te.local_insertion_cases() + te.local_tie_cases() + te.local_extreme_cases(), draw_local, 0),
        ("sgfull", args.sgfull_seconds, lambda: (te.sg_gap_run_cases() + te.sg_staircase_cases() + te.sg_corner_cases()
                                                 + te.sg_wave_edge_end_cases() + te.sg_tie_cases() + te.sg_pad_cases()), draw_sgfull, 1),
        ("local_affine", args.local_affine_seconds, lambda: [c for make in ae.LOCAL_GROUPS.values() for c in make()] + ae.local_extreme_cases(),
         lambda: draw_local(ae.LOCA_LEN1, ae.LOCA_N), 0),
        ("sgfull_affine", args.sgfull_affine_seconds, lambda: [c for make in ae.SG_GROUPS.values() for c in make()],
         lambda: draw_sgfull(ae.sg_shape_grid()), 1)):
    if seconds <= 0:
        continue
    built = cases()
    t_end = time.time() + seconds
    total = bad = rounds = 0
    while time.time() < t_end:
        m, b_ = table_round(kind, built, draw, offset)
        total += m
        bad += b_
        rounds += 1
    print("%s fuzz vs C restatement: %d rounds, %d alignments (grid and random shapes, random matrices and gaps, constructed "
          "edge inputs; traceback and ends-only), %d mismatches" % (kind, rounds, total, bad), flush=True)
