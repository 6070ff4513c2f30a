"""The global / free-end-gap aligner (swmi_global_full*) on the GPU, every field bit-exact against the C restatement
tests/native/global_full_oracle.c (the definition of these semantics; test_global_full_cpu.py ties it to numpy, to the
semi-global restatement and to fixture F8) and against F8 itself, the reference's SemiGlobal_111, whose every path is a
mask-0 alignment of the prefixes that end at its best cell.  Moves are compared up to `steps`; words past it are unspecified.

The length grid follows the kernel's constants (tile_sweep.h): 16 columns per lane and 64 lanes = 1024 columns per wavefront,
up to 16 wavefronts; 4 steps per trip, 32 per chunk, a lane 63 steps behind lane 0 (64), 128 rows per staging block of the
walk, 256 rows per ring between two wavefronts."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from global_full_support import (ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullOracle, assert_same, check_path,
                                 inputs, moves_of, path_from)
from local_support import random_matrix
from sgfull_support import K111, load_f8

pytestmark = pytest.mark.gpu

WAVE = 1024         # columns per wavefront
STAGE = 128         # rows of the walk's staging block
DIAG, UP, LEFT = 3, 2, 1
K54 = match_matrix(5, -4)
KMAX = match_matrix(127, -127)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullOracle(tmp_path_factory.mktemp("global_full_oracle"))


def _both(gpu, oracle, a, b, sm, gap, mask, what):
    """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
    want = oracle.align(a, b, sm, gap, mask)
    assert_same(gpu.global_full(a, b, sm, gap, mask), want, what)
    sc, ends, mv, st = gpu.global_full(a, b, sm, gap, mask, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    return want


# ---- 1. fixture F8: the reference pin -------------------------------------------------------------------------------------

def test_f8_prefixes_through_the_host_entry(gpu):
    """For each of the 25 F8 vectors whose best cell lies at (1, 1) or beyond, the mask-0 alignment of seq1[:end_i] and
    seq2[:end_j] is F8's: its score, end, start (0, 0), steps == lengths - 1 and moves.  The two vectors with score 0 have
    no prefixes to align."""
    f8 = load_f8()
    seen = 0
    for k in range(len(f8["scores"])):
        ei, ej = (int(x) for x in f8["ends"][k])
        if ei < 1 or ej < 1:
            assert f8["scores"][k] == 0
            continue
        seen += 1
        a, b = f8["seq1"][k:k + 1, :ei], f8["seq2"][k:k + 1, :ej]
        sc, ends, mv, st = gpu.global_full(a, b, K111, 1, GLOBAL)
        assert sc[0] == f8["scores"][k] and tuple(ends[0]) == (ei, ej, 0, 0) and st[0] == f8["lengths"][k] - 1, (k, f8["kind"][k])
        assert np.array_equal(path_from(mv[0], st[0], ei, ej), f8["paths"][k]), (k, f8["kind"][k])
        sc2, ends2, _, _ = gpu.global_full(a, b, K111, 1, GLOBAL, traceback=False)
        assert sc2[0] == sc[0] and tuple(ends2[0]) == (ei, ej, -1, -1), k
    assert seen == 25


# ---- 2. the length grid -----------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 16384), (16384, 1), (3, 1023), (4, 1024), (5, 1025), (33, 15361), (63, 2047), (65, 1041), (129, 2049),
          (257, 1024), (1500, 2100)]


def _grid_checks(a, b, sm, gap, mask, want, what):
    sc, ends, mv, st = want
    len1, len2 = a.shape[1], b.shape[1]
    kinds = [set(moves_of(mv[k], st[k]).tolist()) for k in range(len(a))]
    if mask == GLOBAL:
        # the mask-0 walk runs from (len1, len2) to (0, 0): through every wavefront's first column
        assert np.all(ends == np.array([len1, len2, 0, 0])), what
        for k in range(len(a)):
            assert path_from(mv[k], st[k], len1, len2)[:, 1].tolist().count(WAVE) >= 1 or len2 < WAVE, what
    for k in range(0, len(a), 5):
        check_path(a[k], b[k], sm, gap, mask, sc[k], ends[k], mv[k], st[k])
    return any(k == {DIAG, UP, LEFT} for k in kinds)


@pytest.mark.parametrize("len1,len2", SHAPES)
def test_length_grid_across_masks_and_parameter_sets(gpu, oracle, len1, len2):
    all_kinds = False
    for p, (sm, gap) in enumerate(((K111, 1), (K54, 0), (random_matrix(), 3))):
        a, b = inputs(6, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        for mask in ALL_MASKS:
            want = _both(gpu, oracle, a, b, sm, gap, mask, (len1, len2, p, mask))
            all_kinds |= _grid_checks(a, b, sm, gap, mask, want, (len1, len2, p, mask)) and mask == GLOBAL
    # the inputs must not let the grid pass on trivial walks: some mask-0 walk of the shape's batches holds all three kinds of
    # move.  (A table of one row cannot: its walk has one step that leaves the row, a diagonal or an up.  And where seq2 is
    # much the longer one and a mismatch costs less than two gaps, as at (1, -1, 1), no optimal walk holds an up move: it
    # needs one more left move, and the mismatch is cheaper than the two.  There the batches at (5, -4, 0) hold them.)
    if len2 > WAVE and len1 >= 2:
        assert all_kinds, (len1, len2)


@pytest.mark.parametrize("mask", [GLOBAL, FIT, OVERLAP])
def test_full_size(gpu, oracle, mask):
    for p, (sm, gap) in enumerate(((K111, 1), (KMAX, 127))):
        a, b = inputs(2, 16384, 16384, 7 + p)
        want = _both(gpu, oracle, a, b, sm, gap, mask, (16384, p, mask))
        assert _grid_checks(a, b, sm, gap, mask, want, (16384, p, mask)), "no walk with all three kinds of move"


# ---- 3. hand-built cases ----------------------------------------------------------------------------------------------------
# Background: seq1 all 0, seq2 all 1, so nothing matches but what a test plants with bases 2 and 3.

def _background(len1, len2, n=1):
    return np.zeros((n, len1), np.uint8), np.ones((n, len2), np.uint8)


def _expect(gpu, oracle, a, b, sm, gap, mask, score, ends, codes, what):
    """One alignment (row 0 of a, b): the hand-worked score, (end_i, end_j, start_i, start_j) and walking-order move codes,
    on the restatement and on the GPU."""
    want = _both(gpu, oracle, a, b, sm, gap, mask, what)
    for name, (sc, e, mv, st) in (("restatement", want), ("gpu", gpu.global_full(a, b, sm, gap, mask))):
        assert sc[0] == score and tuple(e[0]) == tuple(ends) and st[0] == len(codes), (what, name, sc[0], e[0], st[0])
        assert np.array_equal(moves_of(mv[0], st[0]), np.asarray(codes, np.int64)), (what, name)
    sc, e, _, _ = gpu.global_full(a, b, sm, gap, mask, traceback=False)
    assert sc[0] == score and tuple(e[0]) == (ends[0], ends[1], -1, -1), what


def test_negative_scores(gpu, oracle):
    """Global on an all-mismatch pair: H(i, j) = -max(i, j), so the walk takes len1 diagonals (the first choice wherever it
    holds), which end on row 0, and then is forced left."""
    for len1, len2 in ((3, 5), (130, 1025), (300, 2000)):
        a, b = _background(len1, len2)
        _expect(gpu, oracle, a, b, K111, 1, GLOBAL, -len2, (len1, len2, 0, 0), [DIAG] * len1 + [LEFT] * (len2 - len1),
                ("mismatch", len1, len2))


def _fit_case():
    L, off, len2 = 150, 1000, 2100
    P = np.random.default_rng(6).integers(2, 4, L).astype(np.uint8)
    a = P[None, :].copy()
    _, b = _background(L, len2)
    b[0, off:off + L] = P
    return L, off, len2, a, b


def test_fit(gpu, oracle):
    """All of seq1 = P inside seq2 at column offset 1000: L matches and nothing else to match, so the last row holds L at
    column 1150 only; the walk crosses column 1024 and ends on row 0, which is free."""
    L, off, len2, a, b = _fit_case()
    _expect(gpu, oracle, a, b, K111, 1, FIT, L, (L, off + L, 0, off), [DIAG] * L, "fit")


def test_fit_inputs_under_mask_0_force_a_run_along_row_0(gpu, oracle):
    """The same pair end to end: every base of seq2 outside P costs a gap (a mismatch costs as much and aligns nothing
    better), so the score is L - (len2 - L); the walk goes left to column 1150, takes the L diagonals to (0, 1000) and is
    forced left along row 0 for 1000 moves, which the count includes."""
    L, off, len2, a, b = _fit_case()
    _expect(gpu, oracle, a, b, K111, 1, GLOBAL, L - (len2 - L), (L, len2, 0, 0),
            [LEFT] * (len2 - off - L) + [DIAG] * L + [LEFT] * off, "fit under mask 0")


def test_overlap(gpu, oracle):
    """seq1 ends with P and seq2 begins with P (1100 bases: the end cell lies in wavefront 1): the diagonal from (len1 - L, 0)
    to (len1, L) holds every match there is."""
    L, len1, len2 = 1100, 1500, 2100
    P = np.random.default_rng(8).integers(2, 4, L).astype(np.uint8)
    a, b = _background(len1, len2)
    a[0, len1 - L:] = P
    b[0, :L] = P
    _expect(gpu, oracle, a, b, K111, 1, OVERLAP, L, (len1, L, len1 - L, 0), [DIAG] * L, "overlap")


def _column_fit_case():
    L, off, len1 = 1025, 200, 1500
    P = np.random.default_rng(9).integers(2, 4, L).astype(np.uint8)
    a, _ = _background(len1, L)
    a[0, off:off + L] = P
    return L, off, len1, a, P[None, :].copy()


def test_begin1_end1_ends_in_the_last_valid_column_of_a_padded_wavefront(gpu, oracle):
    """seq2 = P of 1025 bases inside a longer seq1: column 1025 is the only valid column of wavefront 1."""
    L, off, len1, a, b = _column_fit_case()
    _expect(gpu, oracle, a, b, K111, 1, BEGIN1 | END1, L, (off + L, L, off, 0), [DIAG] * L, "begin1 | end1")


def test_column_fit_inputs_under_mask_0_force_a_run_along_column_0(gpu, oracle):
    L, off, len1, a, b = _column_fit_case()
    _expect(gpu, oracle, a, b, K111, 1, GLOBAL, L - (len1 - L), (len1, L, 0, 0),
            [UP] * (len1 - off - L) + [DIAG] * L + [UP] * off, "column fit under mask 0")


def test_padding_columns_never_win_at_gap_0(gpu, oracle):
    """(5, -4, 0), len2 = 1025, the last 20 bases of both sequences match: at gap 0 the padding columns right of column 1025
    hold the corner's score too.  H = 5 x the longest common subsequence, 100 at (len1, 1025) only.  The walk takes the 20
    diagonals to (len1 - 20, 1005), where H = 0 = H above: up to row 0; with BEGIN2 it ends there, else it is forced left."""
    L, len1, len2 = 20, 100, 1025
    P = np.random.default_rng(10).integers(2, 4, L).astype(np.uint8)
    a, b = _background(len1, len2)
    a[0, len1 - L:] = P
    b[0, len2 - L:] = P
    _expect(gpu, oracle, a, b, K54, 0, END2, 5 * L, (len1, len2, 0, 0), [DIAG] * L + [UP] * (len1 - L) + [LEFT] * (len2 - L), "pad, END2")
    _expect(gpu, oracle, a, b, K54, 0, FIT, 5 * L, (len1, len2, 0, len2 - L), [DIAG] * L + [UP] * (len1 - L), "pad, FIT")


def test_end_cell_ties(gpu, oracle):
    """Homopolymer against homopolymer with every end free: H(i, j) = min(i, j).  The last column and the last row hold m =
    min(len1, len2) in many cells; the first of them in row-major order is (m, m)."""
    for len1, len2 in ((40, 1100), (1100, 40)):
        a = np.full((1, len1), 2, np.uint8)
        b = np.full((1, len2), 2, np.uint8)
        m = min(len1, len2)
        # (40, 1100): the last column holds min(i, 1100) = i, at most 40 in (40, 1100) itself; row 40 holds 40 from column 40 on
        # (1100, 40): the last column holds 40 from row 40 on, (40, 40) first
        _expect(gpu, oracle, a, b, K111, 1, OVERLAP, m, (m, m, 0, 0), [DIAG] * m, ("homopolymer", len1, len2))


def test_the_extremes_at_full_size(gpu):
    a = np.random.default_rng(46).integers(0, 4, (1, 16384), dtype=np.uint8)
    for mask in (GLOBAL, OVERLAP):
        sc, ends, mv, st = gpu.global_full(a, a.copy(), KMAX, 127, mask)
        assert sc[0] == 127 * 16384 == 2080768 and tuple(ends[0]) == (16384, 16384, 0, 0) and st[0] == 16384
        assert np.all(moves_of(mv[0], st[0]) == DIAG)
    # and the most negative score there is: nothing matches, every step costs 127
    z, o = _background(16384, 16384)
    sc, ends, mv, st = gpu.global_full(z, o, KMAX, 127, GLOBAL)
    assert sc[0] == -127 * 16384 and tuple(ends[0]) == (16384, 16384, 0, 0) and st[0] == 16384


# ---- 4. batch sizes and slices ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(gpu, oracle, n):
    a, b = inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    for mask in (GLOBAL, OVERLAP):
        assert_same(gpu.global_full(a, b, sm, 5, mask), oracle.align(a, b, sm, 5, mask), (n, mask))


def test_batch_across_a_slice_boundary(gpu, oracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets.  Four
    distinct pairs, repeated: the restatement runs on those."""
    n = 257
    assert gpu.global_full_slices_for(n, 16384, 16384, 1) == [256, 1]
    a4, b4 = inputs(4, 16384, 16384, 257)
    pick = np.arange(n) % 4
    got = gpu.global_full(a4[pick], b4[pick], K111, 1, FIT)
    gpu.global_full_release_workspaces()
    want = oracle.align(a4, b4, K111, 1, FIT)
    assert_same(got, tuple(x[pick] for x in want), "slices")


# ---- 5. / 6. the device entry, threads ---------------------------------------------------------------------------------------

def test_device_entry_equals_host_entry_on_two_streams(gpu):
    """swmi_global_full_device on torch buffers, two calls on two streams issued before either is waited for, each equal to
    the host entry; one traceback, one ends-only."""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, len2, n, seed, tb, mask in ((3000, 5000, 40, 1, True, FIT), (1023, 16384, 9, 2, False, OVERLAP)):
        a, b = inputs(n, len1, len2, seed)
        mw = gpu.global_full_move_words(len1, len2)
        t = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                 ends=torch.zeros((n, 4), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                 st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((len1, len2, n, a, b, t, tb, mask, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, len2, n, a, b, t, tb, mask, s in jobs:
        gpu.global_full_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 2, mask, t["sc"].data_ptr(), t["ends"].data_ptr(),
                               t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None, stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, mask, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["st"].cpu().numpy().view(np.uint32))
        want = gpu.global_full(a, b, sm, 2, mask)
        assert_same(got, want, ("device", len1, len2), traceback=tb)
    ms = gpu.global_full_time_device(jobs[0][5]["a"].data_ptr(), 3000, jobs[0][5]["b"].data_ptr(), 5000, 40, sm, 2, FIT,
                                     jobs[0][5]["sc"].data_ptr(), jobs[0][5]["ends"].data_ptr(), iters=2)
    assert ms > 0


def test_host_entry_from_two_threads(gpu, oracle):
    a, b = inputs(300, 900, 1500, 9)
    want = [oracle.align(a, b, K54, 0, mask) for mask in (GLOBAL, OVERLAP)]
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.global_full(a, b, K54, 0, (GLOBAL, OVERLAP)[k])
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert_same(out[k], want[k], k)


def test_bytes_are_taken_modulo_4(gpu):
    a, b = inputs(9, 300, 1500, 44)
    rng = np.random.default_rng(45)
    a2 = (a | (rng.integers(0, 64, a.shape) << 2)).astype(np.uint8)
    b2 = (b | (rng.integers(0, 64, b.shape) << 2)).astype(np.uint8)
    assert a2.max() > 250 and b2.max() > 250
    sm = random_matrix()
    for mask in (GLOBAL, FIT):
        assert_same(gpu.global_full(a2, b2, sm, 2, mask), gpu.global_full(a, b, sm, 2, mask), "modulo 4")


# ---- 7. the C++ overloads ----------------------------------------------------------------------------------------------------

def _checksum(path):
    want = 0
    for i, j in path:
        want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
    return want


def _run_compat(exe, tmp_path, name, a, b, sm, gap, mask, piece):
    data = tmp_path / name
    with open(data, "wb") as fh:
        fh.write(np.array([a.shape[0], a.shape[1], b.shape[1], gap], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(a.shape[0]):
            fh.write(a[k].tobytes() + b[k].tobytes())
    run = subprocess.run([exe, str(data), str(mask), str(piece)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-2:] == ["single 0", "ragged 1"], lines[-2:]
    rows = [tuple(map(int, line.split())) for line in lines[:-2]]
    assert len(rows) == a.shape[0]
    return rows


def test_cpp_overloads(gpu, oracle, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "compat_global_full")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_full.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a, b = inputs(10, 1200, 2300, 71)
    sm = random_matrix()
    for mask, piece in ((GLOBAL, 4), (FIT, 0)):
        sc, ends, mv, st = oracle.align(a, b, sm, 3, mask)
        rows = _run_compat(exe, tmp_path, "batch%d.bin" % mask, a, b, sm, 3, mask, piece)
        for k in range(10):
            path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), _checksum(path)), (mask, k)
