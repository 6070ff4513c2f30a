"""The affine global / free-end-gap aligner (swmi_global_full_affine*) on the GPU, every field bit-exact against the C
restatement tests/native/global_full_affine_oracle.c (the definition of these semantics; test_global_full_affine_cpu.py ties it
to a numpy three-matrix formulation, to the linear restatement at open = extend and to the affine semi-global one by the
mask-0 prefix identity), and against the linear GPU entry at open = extend.  Moves are compared up to `steps`; words past it
are unspecified.  Every case runs with traceback and ends-only.

The length grid follows the kernel's constants (tile_sweep.h): 16 columns per lane and 64 lanes = 1024 columns per wavefront,
up to 16 wavefronts; 4 steps per trip, 32 per chunk, a lane 63 steps behind lane 0, 128 rows x 32 lanes (512 columns) per
affine staging block of the walk, 256 rows per ring between two wavefronts."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from global_full_affine_support import (ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullAffineOracle, assert_same,
                                        check_path, gap_runs, moves_of, path_from)
from global_full_affine_edges import END_CELL_TIE_SHAPES, end_cell_tie_case, one_long_gap_case, padding_case
from global_full_affine_edges import background as _background, column_fit_case as _column_fit_case, fit_case as _fit_case
from global_full_support import inputs
from local_support import random_matrix

pytestmark = pytest.mark.gpu

WAVE = 1024         # columns per wavefront
DIAG, UP, LEFT = 3, 2, 1
K111 = match_matrix(1, -1)
K54 = match_matrix(5, -4)
KMAX = match_matrix(127, -127)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullAffineOracle(tmp_path_factory.mktemp("global_full_affine_oracle"))


@pytest.fixture(scope="module")
def ga(gpu):
    return gpu.global_affine


def _both(ga, oracle, a, b, sm, go, ge, mask, what):
    """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
    want = oracle.align(a, b, sm, go, ge, mask)
    assert_same(ga.global_full_affine(a, b, sm, go, ge, mask), want, what)
    sc, ends, mv, st = ga.global_full_affine(a, b, sm, go, ge, mask, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    return want


# ---- 1. the length grid -----------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 16384), (16384, 1), (3, 1023), (4, 1024), (5, 1025), (33, 15361), (63, 2047), (65, 1041), (129, 2049),
          (257, 1024), (300, 15361), (1500, 2100)]
PARAM_SETS = ((K111, 1, 1), (K54, 0, 0), (random_matrix(), 5, 2), (random_matrix(), 2, 5))


def _grid_checks(a, b, sm, go, ge, mask, want, what):
    """(some walk holds all three kinds of move, some walk holds a gap run of two or more)"""
    sc, ends, mv, st = want
    len1, len2 = a.shape[1], b.shape[1]
    codes = [moves_of(mv[k], st[k]) for k in range(len(a))]
    if mask == GLOBAL:
        # the mask-0 walk runs from (len1, len2) to (0, 0): through every wavefront's first column
        assert np.all(ends == np.array([len1, len2, 0, 0])), what
        for k in range(len(a)):
            assert path_from(mv[k], st[k], len1, len2)[:, 1].tolist().count(WAVE) >= 1 or len2 < WAVE, what
    for k in range(0, len(a), 5):
        check_path(a[k], b[k], sm, go, ge, mask, sc[k], ends[k], mv[k], st[k])
    return (any(set(c.tolist()) == {DIAG, UP, LEFT} for c in codes),
            any(code != DIAG and k >= 2 for c in codes for code, k in gap_runs(c)))


@pytest.mark.parametrize("len1,len2", SHAPES)
def test_length_grid_across_masks_and_parameter_sets(ga, oracle, len1, len2):
    all_kinds = long_run = False
    for p, (sm, go, ge) in enumerate(PARAM_SETS):
        a, b = inputs(6, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        for mask in ALL_MASKS:
            want = _both(ga, oracle, a, b, sm, go, ge, mask, (len1, len2, p, mask))
            kinds, run = _grid_checks(a, b, sm, go, ge, mask, want, (len1, len2, p, mask))
            all_kinds |= kinds and mask == GLOBAL
            long_run |= run
    # the inputs must not let the grid pass on trivial walks: some mask-0 walk of the shape's batches holds all three kinds of
    # move (a table of one row cannot: its walk has one step that leaves the row), and some walk holds a gap run of length two
    # or more (every shape but (1, 1) forces one under mask 0: |len1 - len2| >= 2, or the 5-base indel of every third pair)
    if len2 > WAVE and len1 >= 2:
        assert all_kinds, (len1, len2)
    if (len1, len2) != (1, 1):
        assert long_run, (len1, len2)


# ---- 2. open == extend against the linear GPU entry --------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(5, 1025), (129, 2049), (300, 15361), (1500, 2100)])
def test_open_equal_extend_is_the_linear_gpu_entry(gpu, ga, len1, len2):
    for p, (sm, g) in enumerate(((K111, 1), (K54, 0), (random_matrix(), 3))):
        a, b = inputs(6, len1, len2, 7 * p + len1 % 13)
        for mask in (GLOBAL, FIT, OVERLAP):
            want = gpu.global_full(a, b, sm, g, mask)
            assert_same(ga.global_full_affine(a, b, sm, g, g, mask), want, (len1, len2, p, mask))
            sc, ends, _, _ = ga.global_full_affine(a, b, sm, g, g, mask, traceback=False)
            assert_same((sc, ends, None, None), want, (len1, len2, p, mask, "ends-only"), traceback=False)


# ---- 3. hand-built cases ----------------------------------------------------------------------------------------------------
# The inputs come from global_full_affine_edges.py (the wide-alphabet edge tests relabel them).  Background: seq1 all 0, seq2 all
# 1, so nothing matches but what a case plants with bases 2 and 3.


def _expect(ga, oracle, a, b, sm, go, ge, mask, score, ends, codes, what):
    """One alignment (row 0 of a, b): the hand-worked score, (end_i, end_j, start_i, start_j) and walking-order move codes,
    on the restatement and on the GPU."""
    want = _both(ga, oracle, a, b, sm, go, ge, mask, what)
    for name, (sc, e, mv, st) in (("restatement", want), ("gpu", ga.global_full_affine(a, b, sm, go, ge, mask))):
        assert sc[0] == score and tuple(e[0]) == tuple(ends) and st[0] == len(codes), (what, name, sc[0], e[0], st[0])
        assert np.array_equal(moves_of(mv[0], st[0]), np.asarray(codes, np.int64)), (what, name)
    sc, e, _, _ = ga.global_full_affine(a, b, sm, go, ge, mask, traceback=False)
    assert sc[0] == score and tuple(e[0]) == (ends[0], ends[1], -1, -1), what


def test_fit(ga, oracle):
    """All of seq1 = P inside seq2 at column offset 1000: L matches and nothing else to match; the walk crosses column 1024
    and ends on row 0, which is free."""
    L, off, len2, a, b = _fit_case()
    _expect(ga, oracle, a, b, K111, 3, 1, FIT, L, (L, off + L, 0, off), [DIAG] * L, "fit")


def test_fit_inputs_under_mask_0(ga, oracle):
    """The same pair end to end: one gap of 950 after P and one of 1000 before it.  The F run of 950 goes through two wave
    boundaries and two 512-column staging blocks in state F; the 1000 lefts along the charged row 0 are forced."""
    L, off, len2, a, b = _fit_case()
    assert L - (3 + 999) - (3 + 949) == -1804
    _expect(ga, oracle, a, b, K111, 3, 1, GLOBAL, -1804, (L, len2, 0, 0), [LEFT] * (len2 - off - L) + [DIAG] * L + [LEFT] * off,
            "fit under mask 0")


def test_fit_inputs_where_a_mismatch_costs_127(ga, oracle):
    """Match 1 / mismatch -127: nothing but P may align, and P is not worth its gaps.  BEGIN2 alone: the last column's 150 up
    moves from the free row 0, an E run across a staging block's 128 rows that ends on row 0 in the last column.  END2 alone:
    the end cell is the closed-form border cell (len1, 0), and the whole walk is forced."""
    L, off, len2, a, b = _fit_case()
    sm = match_matrix(1, -127)
    _expect(ga, oracle, a, b, sm, 3, 1, BEGIN2, -(3 + 149), (L, len2, 0, len2), [UP] * L, "E run to the free row 0")
    _expect(ga, oracle, a, b, sm, 3, 1, END2, -(3 + 149), (L, 0, 0, 0), [UP] * L, "border end cell, forced walk")


def test_column_fit(ga, oracle):
    """seq2 = P of 1025 bases inside a longer seq1: column 1025 is the only valid column of wavefront 1."""
    L, off, len1, a, b = _column_fit_case()
    assert L - (3 + 199) - (3 + 274) == 546
    _expect(ga, oracle, a, b, K111, 3, 1, GLOBAL, 546, (len1, L, 0, 0), [UP] * (len1 - off - L) + [DIAG] * L + [UP] * off,
            "column fit under mask 0")
    _expect(ga, oracle, a, b, K111, 3, 1, BEGIN1 | END1, L, (off + L, L, off, 0), [DIAG] * L, "begin1 | end1")


def test_one_long_gap_beats_many(ga, oracle):
    """seq2 = seq1 without bases 100..139 at open 10, extend 1: 260 matches and one gap of 40, exactly one UP run; where it
    sits among equal bases follows the restatement."""
    x, y, sm = one_long_gap_case()
    assert x.shape == (1, 300) and y.shape == (1, 260) and np.array_equal(sm, match_matrix(2, -3))
    want = _both(ga, oracle, x, y, sm, 10, 1, GLOBAL, "one long gap")
    sc, ends, mv, st = ga.global_full_affine(x, y, sm, 10, 1, GLOBAL)
    assert sc[0] == 2 * 260 - (10 + 39) == 471 and tuple(ends[0]) == (300, 260, 0, 0)
    gaps = [(code, k) for code, k in gap_runs(moves_of(mv[0], st[0])) if code != DIAG]
    assert gaps == [(UP, 40)], gaps
    assert np.array_equal(moves_of(mv[0], st[0]), moves_of(want[2][0], want[3][0]))


def test_padding_columns_never_win_at_zero_gap_costs(ga, oracle):
    """(5, -4), open = extend = 0, len2 = 1025, the last 20 bases of both sequences match: at no gap cost the padding columns
    right of column 1025 hold the corner's score too.  The linear test's inputs and results."""
    L, len1, len2, a, b = padding_case()
    assert (L, len1, len2) == (20, 100, 1025)
    _expect(ga, oracle, a, b, K54, 0, 0, END2, 5 * L, (len1, len2, 0, 0), [DIAG] * L + [UP] * (len1 - L) + [LEFT] * (len2 - L), "pad, END2")
    _expect(ga, oracle, a, b, K54, 0, 0, FIT, 5 * L, (len1, len2, 0, len2 - L), [DIAG] * L + [UP] * (len1 - L), "pad, FIT")


def test_end_cell_ties(ga, oracle):
    """Homopolymer against homopolymer with every end free: H(i, j) = min(i, j).  The last column and the last row hold m =
    min(len1, len2) in many cells; the first of them in row-major order is (m, m)."""
    assert END_CELL_TIE_SHAPES == ((40, 1100), (1100, 40))
    for len1, len2 in END_CELL_TIE_SHAPES:
        a, b = end_cell_tie_case(len1, len2)
        m = min(len1, len2)
        _expect(ga, oracle, a, b, K111, 3, 1, OVERLAP, m, (m, m, 0, 0), [DIAG] * m, ("homopolymer", len1, len2))


def test_the_extremes_of_the_key_range(ga):
    """One 16384 x 16384 pair at match 127 / mismatch -127, open = extend = 127; closed forms, no restatement run."""
    a = np.random.default_rng(46).integers(0, 4, (1, 16384), dtype=np.uint8)
    for mask in (GLOBAL, OVERLAP):
        sc, ends, mv, st = ga.global_full_affine(a, a.copy(), KMAX, 127, 127, mask)
        assert sc[0] == 127 * 16384 == 2080768 and tuple(ends[0]) == (16384, 16384, 0, 0) and st[0] == 16384
        assert np.all(moves_of(mv[0], st[0]) == DIAG)
        sc, ends, _, _ = ga.global_full_affine(a, a.copy(), KMAX, 127, 127, mask, traceback=False)
        assert sc[0] == 2080768 and tuple(ends[0]) == (16384, 16384, -1, -1)
    # and the most negative score there is: nothing matches, every step costs 127
    z, o = _background(16384, 16384)
    sc, ends, mv, st = ga.global_full_affine(z, o, KMAX, 127, 127, GLOBAL)
    assert sc[0] == -127 * 16384 and tuple(ends[0]) == (16384, 16384, 0, 0) and st[0] == 16384
    sc, ends, _, _ = ga.global_full_affine(z, o, KMAX, 127, 127, GLOBAL, traceback=False)
    assert sc[0] == -127 * 16384 and tuple(ends[0]) == (16384, 16384, -1, -1)


# ---- 4. batch sizes and slices ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(ga, oracle, n):
    a, b = inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    for mask in (GLOBAL, OVERLAP):
        want = oracle.align(a, b, sm, 7, 2, mask)
        assert_same(ga.global_full_affine(a, b, sm, 7, 2, mask), want, (n, mask))
        sc, ends, _, _ = ga.global_full_affine(a, b, sm, 7, 2, mask, traceback=False)
        assert_same((sc, ends, None, None), want, (n, mask, "ends-only"), traceback=False)


def test_batch_across_a_slice_boundary(ga, oracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets.  Four
    distinct pairs, repeated: the restatement runs on those."""
    n = 257
    assert ga.global_full_affine_slices_for(n, 16384, 16384, 1) == [256, 1]
    a4, b4 = inputs(4, 16384, 16384, 257)
    pick = np.arange(n) % 4
    got = ga.global_full_affine(a4[pick], b4[pick], K111, 3, 1, FIT)
    ga.global_full_affine_release_workspaces()
    want = oracle.align(a4, b4, K111, 3, 1, FIT)
    assert_same(got, tuple(x[pick] for x in want), "slices")


# ---- 5. / 6. the device entry, threads ---------------------------------------------------------------------------------------

def test_device_entry_equals_host_entry_on_two_streams(gpu, ga):
    """swmi_global_full_affine_device on torch buffers, two calls on two streams issued before either is waited for, each
    equal to the host entry; one traceback, one ends-only.  Then the timer."""
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
        ga.global_full_affine_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 6, 2, mask, t["sc"].data_ptr(),
                                     t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None,
                                     stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, mask, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["st"].cpu().numpy().view(np.uint32))
        want = ga.global_full_affine(a, b, sm, 6, 2, mask)
        assert_same(got, want, ("device", len1, len2), traceback=tb)
    ms = ga.global_full_affine_time_device(jobs[0][5]["a"].data_ptr(), 3000, jobs[0][5]["b"].data_ptr(), 5000, 40, sm, 6, 2, FIT,
                                           jobs[0][5]["sc"].data_ptr(), jobs[0][5]["ends"].data_ptr(), iters=2)
    assert ms > 0


def test_host_entry_from_two_threads(gpu, ga, oracle):
    a, b = inputs(300, 900, 1500, 9)
    want = [oracle.align(a, b, K54, 4, 1, mask) for mask in (GLOBAL, OVERLAP)]
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = ga.global_full_affine(a, b, K54, 4, 1, (GLOBAL, OVERLAP)[k])
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert_same(out[k], want[k], k)


def test_bytes_are_taken_modulo_4(ga):
    a, b = inputs(9, 300, 1500, 44)
    rng = np.random.default_rng(45)
    a2 = (a | (rng.integers(0, 64, a.shape) << 2)).astype(np.uint8)
    b2 = (b | (rng.integers(0, 64, b.shape) << 2)).astype(np.uint8)
    assert a2.max() > 250 and b2.max() > 250
    sm = random_matrix()
    for mask in (GLOBAL, FIT):
        assert_same(ga.global_full_affine(a2, b2, sm, 5, 2, mask), ga.global_full_affine(a, b, sm, 5, 2, mask), "modulo 4")


# ---- 7. the C++ overloads ----------------------------------------------------------------------------------------------------

def _checksum(path):
    want = 0
    for i, j in path:
        want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
    return want


def _run_compat(exe, tmp_path, name, a, b, sm, go, ge, mask, piece):
    data = tmp_path / name
    with open(data, "wb") as fh:
        fh.write(np.array([a.shape[0], a.shape[1], b.shape[1], go, ge], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
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
    exe = str(tmp_path / "compat_global_full_affine")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_full_affine.cpp"), "-o", exe, "-L", lib, "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a, b = inputs(10, 1200, 2300, 71)
    sm = random_matrix()
    for mask, piece in ((GLOBAL, 4), (FIT, 0)):
        sc, ends, mv, st = oracle.align(a, b, sm, 6, 2, mask)
        rows = _run_compat(exe, tmp_path, "batch%d.bin" % mask, a, b, sm, 6, 2, mask, piece)
        for k in range(10):
            path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), _checksum(path)), (mask, k)
