"""The any-length local aligner (swmi_local_full*) on the GPU, every field bit-exact against the C restatement
tests/native/local_full_oracle.c (which test_local_full_cpu.py ties to fixture F7, the reference's SmithWaterman_111_long,
to the 128-column restatement, to numpy and to fixture F1), against F7 itself and against swmi_local_align at len2 = 128.
Moves are compared up to `steps`; words past it are unspecified.

The length grid follows the kernel's constants (local_full_kernels.hip): 16 columns per lane and 64 lanes = 1024 columns per
wavefront, up to 16 wavefronts; 4 steps per trip, 32 per chunk, a lane 63 steps behind lane 0 (64), 128 rows per staging
block of the walk, 256 rows per ring between two wavefronts."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_full_support import LocalFullOracle, assert_same, check_path, inputs, moves_of, path_from
from local_support import PARAMS, f7_by_length, random_matrix

pytestmark = pytest.mark.gpu

WAVE = 1024         # columns per wavefront
STAGE = 128         # rows of the walk's staging block
DIAG, UP, LEFT = 3, 2, 1


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LocalFullOracle(tmp_path_factory.mktemp("local_full_oracle"))


def _both(gpu, oracle, a, b, sm, gap, what):
    """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
    want = oracle.align(a, b, sm, gap)
    assert_same(gpu.local_full(a, b, sm, gap), want, what)
    sc, ends, mv, st = gpu.local_full(a, b, sm, gap, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    return want


# ---- 1. fixture F7 and swmi_local_align at len2 = 128 ----------------------------------------------------------------------

def test_f7_through_the_host_entry(gpu):
    for len1, (a, b, f7_scores, f7_paths) in f7_by_length().items():
        sc, ends, mv, st = gpu.local_full(a, b, match_matrix(1, -1), 1)
        assert np.array_equal(sc, f7_scores), len1
        for k, path in enumerate(f7_paths):
            assert st[k] == len(path) - 1 and tuple(ends[k]) == (*path[-1], *path[0]), (len1, k)
            assert np.array_equal(gpu.local_full_expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1]), path), (len1, k)
            assert np.array_equal(path_from(mv[k], st[k], ends[k, 0], ends[k, 1]), path), (len1, k)


def test_every_field_equals_local_align_at_128_columns(gpu):
    for len1, (a, b, _, _) in f7_by_length().items():
        for p, (m, x, g) in enumerate(PARAMS):
            sm = match_matrix(m, x)
            assert_same(gpu.local_full(a, b, sm, g), gpu.local_align(a, b, sm, g), (len1, p))
            sc, ends, _, _ = gpu.local_full(a, b, sm, g, traceback=False)
            wsc, wends, _, _ = gpu.local_align(a, b, sm, g, traceback=False)
            assert np.array_equal(sc, wsc) and np.array_equal(ends, wends), (len1, p)


# ---- 2. the length grid -----------------------------------------------------------------------------------------------------

SHAPES = [(1, 1), (1, 16384), (16384, 1), (2, 3),
          # len2 at the wavefront edges (and len2 mod 16 in 15 / 0 / 1), len1 around the trip
          (3, 1023), (4, 1024), (5, 1025),
          # two wavefronts and one column more; one valid column in the last of 16 wavefronts; all 16 full.  len1 around the chunk
          (31, 2048), (32, 2049), (33, 15361), (64, 16384),
          # len1 around lane 63's delay, the staging block and the ring; len2 mod 16 in 15 / 1 / 0 once more
          (63, 2047), (65, 1041), (127, 1040), (128, 1023), (129, 2049), (255, 1025), (256, 2048), (257, 1024),
          # both lengths past one wavefront and one staging block: the walks cross wavefronts and staging blocks
          (1500, 2100), (2048, 2049), (1100, 15361), (16384, 16384)]


@pytest.mark.parametrize("len1,len2", SHAPES)
def test_length_grid_across_parameter_sets(gpu, oracle, len1, len2):
    full = len1 == 16384 and len2 == 16384
    n = 2 if full else 12
    params = [(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(), 3)]
    for p, (sm, gap) in enumerate(params):
        if full and p not in (1, 2, 3):
            continue                                    # at 16384 x 16384: (1,-1,1), (5,-4,0) and (127,-127,127)
        a, b = inputs(n, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        sc, ends, mv, st = _both(gpu, oracle, a, b, sm, gap, (len1, len2, p))
        if len2 > WAVE and len1 >= WAVE and p < len(PARAMS):
            # the inputs must not let the grid pass on trivial walks: every planted pair's path crosses a wavefront's first
            # column, and some path leaves the staging block
            planted = [k for k in range(0, n, 3) if k % 7 != 1]
            for k in planted:
                end_j, start_j = int(ends[k, 1]), int(ends[k, 3])
                assert start_j // WAVE < end_j // WAVE, (len1, len2, p, k, start_j, end_j)
            assert int(st.max()) > STAGE, (len1, len2, p)
        for k in range(0, n, 5):
            check_path(a[k], b[k], sm, gap, sc[k], ends[k], mv[k], st[k])


# ---- 3. hand-built edges ----------------------------------------------------------------------------------------------------
# Background: seq1 all 0, seq2 all 1, so nothing matches but what a test plants with bases 2 and 3.

K111 = match_matrix(1, -1)
K54 = match_matrix(5, -4)


def _background(len1, len2, n=1):
    return np.zeros((n, len1), np.uint8), np.ones((n, len2), np.uint8)


def _expect(gpu, oracle, a, b, sm, gap, score, ends, codes, what):
    """One alignment (row 0 of a, b): the hand-worked score, (end_i, end_j, start_i, start_j) and walking-order move codes,
    against the GPU and beside the restatement's."""
    want = _both(gpu, oracle, a, b, sm, gap, what)
    for name, (sc, e, mv, st) in (("restatement", want), ("gpu", gpu.local_full(a, b, sm, gap))):
        assert sc[0] == score and tuple(e[0]) == tuple(ends) and st[0] == len(codes), (what, name, sc[0], e[0], st[0])
        assert np.array_equal(moves_of(mv[0], st[0]), np.asarray(codes, np.int64)), (what, name)
    sc, e, _, _ = gpu.local_full(a, b, sm, gap, traceback=False)
    assert sc[0] == score and tuple(e[0]) == (ends[0], ends[1], -1, -1), what


def test_all_mismatch_pair(gpu, oracle):
    for len1, len2 in ((300, 2000), (1, 1), (130, 1025)):
        a, b = _background(len1, len2)
        for sm, gap in ((K111, 1), (K54, 0)):
            _expect(gpu, oracle, a, b, sm, gap, 0, (0, 0, 0, 0), [], ("mismatch", len1, len2, gap))


@pytest.mark.parametrize("r0,c0", [(0, 0), (7, 1020), (200, 3070)])
def test_the_floor_wins_the_tie_at_zero(gpu, oracle, r0, c0):
    """A match (+1), a mismatch (-1), then 40 matches: the cell after the mismatch holds 0 and its diagonal candidate is 0
    too.  The path starts at that cell and does not continue through the first match."""
    L = 40
    P = np.random.default_rng(5).integers(2, 4, L).astype(np.uint8)
    a, b = _background(r0 + L + 30, c0 + L + 50)
    a[0, r0:r0 + 2 + L] = np.concatenate([[2, 0], P])
    b[0, c0:c0 + 2 + L] = np.concatenate([[2, 1], P])
    # any alignment through the first match and P pays for row r0 + 2, so L is reached at (r0 + 2 + L, c0 + 2 + L) only
    _expect(gpu, oracle, a, b, K111, 1, L, (r0 + 2 + L, c0 + 2 + L, r0 + 2, c0 + 2), [DIAG] * L, ("floor tie", r0, c0))


def test_the_walk_stops_on_row_0_and_on_column_0(gpu, oracle):
    L = 150                                             # more rows than one staging block
    P = np.random.default_rng(6).integers(2, 4, L).astype(np.uint8)
    for r0, c0 in ((0, 1030), (300, 0), (0, 0)):
        a, b = _background(r0 + L + 20, c0 + L + 20)
        a[0, r0:r0 + L] = P
        b[0, c0:c0 + L] = P
        # L matches and nothing else to match: the diagonal from (r0, c0), which lies on a border
        _expect(gpu, oracle, a, b, K111, 1, L, (r0 + L, c0 + L, r0, c0), [DIAG] * L, ("border", r0, c0))


def test_best_cell_ties(gpu, oracle):
    # homopolymer against homopolymer: H(i, j) = match * min(i, j), first at its largest in row min, column min
    for len1, len2 in ((40, 1100), (1100, 40), (40, 40)):
        a = np.full((1, len1), 2, np.uint8)
        b = np.full((1, len2), 2, np.uint8)
        m = min(len1, len2)
        _expect(gpu, oracle, a, b, K111, 1, m, (m, m, 0, 0), [DIAG] * m, ("homopolymer", len1, len2))
        _expect(gpu, oracle, a, b, K54, 0, 5 * m, (m, m, 0, 0), [DIAG] * m, ("homopolymer gap 0", len1, len2))
    # two blocks of 20 matches, one in wavefront 0 (bases 2) and one in wavefront 1 (bases 3), rows and columns disjoint and
    # further apart than a score of 20 decays: both corners hold 20, and the one in the smaller row is first in row-major order
    L = 20
    for rows0, rows1 in ((70, 30), (30, 70)):           # first row of the block in wavefront 0 / in wavefront 1
        a, b = _background(120, 1600)
        a[0, rows0:rows0 + L] = 2
        b[0, 100:100 + L] = 2
        a[0, rows1:rows1 + L] = 3
        b[0, 1500:1500 + L] = 3
        r, c = (rows1, 1500) if rows1 < rows0 else (rows0, 100)
        _expect(gpu, oracle, a, b, K111, 1, L, (r + L, c + L, r, c), [DIAG] * L, ("two wavefronts", rows0, rows1))
        if rows1 < rows0:                               # at gap 0 the first block's 100 spreads right and down, not to the left
            _expect(gpu, oracle, a, b, K54, 0, 5 * L, (r + L, c + L, r, c), [DIAG] * L, ("two wavefronts gap 0", rows0, rows1))
    # gap 0: the block's corner at column 1024 (lane 63 of wavefront 0) hands its score on to column 1025 (lane 0 of
    # wavefront 1) in the same row; the first of the two wins
    a, b = _background(90, 1300)
    a[0, 50:50 + L] = 2
    b[0, WAVE - L:WAVE] = 2
    _expect(gpu, oracle, a, b, K54, 0, 5 * L, (50 + L, WAVE, 50, WAVE - L), [DIAG] * L, "columns 1024 and 1025")


@pytest.mark.parametrize("len2", [1025, 15361])
def test_end_cell_in_the_last_valid_column(gpu, oracle, len2):
    """The columns right of len2 in the last wavefront are padding; at gap 0 they hold the end cell's score too."""
    L = 20
    a, b = _background(60, len2)
    a[0, 30:30 + L] = 2
    b[0, len2 - L:] = 2
    for sm, gap, match in ((K111, 1, 1), (K54, 0, 5)):
        _expect(gpu, oracle, a, b, sm, gap, match * L, (30 + L, len2, 30, len2 - L), [DIAG] * L, ("last column", len2, gap))


def test_single_gap_runs_longer_than_the_staging_block(gpu, oracle):
    """(5, -4), gap 1: 100 matches, a run of 200 gaps, 100 matches.  Every alignment that matches bases on both sides of the
    run pays at least 1 for each of its 200 bases, and 5 * 100 > 200, so the score is 1000 - 200 = 800 at the far corner
    only, and the 200 matching rows and columns pair up in one way."""
    r0, c0 = 10, 824                                    # the left run covers columns 925 .. 1124: it crosses column 1024
    a, b = _background(r0 + 200 + 20, c0 + 400 + 20)
    a[0, r0:r0 + 200] = 2
    b[0, c0:c0 + 100] = 2
    b[0, c0 + 300:c0 + 400] = 2
    _expect(gpu, oracle, a, b, K54, 1, 800, (r0 + 200, c0 + 400, r0, c0), [DIAG] * 100 + [LEFT] * 200 + [DIAG] * 100, "left run")
    r0, c0 = 100, 1500                                  # the up run covers rows 201 .. 400: it crosses the ring's 256 rows
    a, b = _background(r0 + 400 + 20, c0 + 200 + 20)
    b[0, c0:c0 + 200] = 2
    a[0, r0:r0 + 100] = 2
    a[0, r0 + 300:r0 + 400] = 2
    _expect(gpu, oracle, a, b, K54, 1, 800, (r0 + 400, c0 + 200, r0, c0), [DIAG] * 100 + [UP] * 200 + [DIAG] * 100, "up run")


def test_bytes_are_taken_modulo_4(gpu):
    a, b = inputs(9, 300, 1500, 44)
    rng = np.random.default_rng(45)
    a2 = (a | (rng.integers(0, 64, a.shape) << 2)).astype(np.uint8)
    b2 = (b | (rng.integers(0, 64, b.shape) << 2)).astype(np.uint8)
    assert a2.max() > 250 and b2.max() > 250
    sm = random_matrix()
    assert_same(gpu.local_full(a2, b2, sm, 2), gpu.local_full(a, b, sm, 2), "modulo 4")


def test_the_extremes_at_full_size(gpu):
    a = np.random.default_rng(46).integers(0, 4, (1, 16384), dtype=np.uint8)
    sc, ends, mv, st = gpu.local_full(a, a.copy(), match_matrix(127, -127), 127)
    assert sc[0] == 127 * 16384 == 2080768 and tuple(ends[0]) == (16384, 16384, 0, 0) and st[0] == 16384
    assert np.all(moves_of(mv[0], st[0]) == DIAG)


# ---- 4. batch sizes and slices ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(gpu, oracle, n):
    a, b = inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    assert_same(gpu.local_full(a, b, sm, 5), oracle.align(a, b, sm, 5), n)


def test_batch_across_a_slice_boundary(gpu, oracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets."""
    n = 257
    assert gpu.local_full_slices_for(n, 16384, 16384) == [256, 1]
    a, b = inputs(n, 16384, 16384, 257)
    got = gpu.local_full(a, b, K111, 1)
    gpu.local_full_release_workspaces()
    assert_same(got, oracle.align(a, b, K111, 1), "slices")


# ---- 5. / 6. the device entry, threads ---------------------------------------------------------------------------------------

def test_device_entry_equals_host_entry_on_two_streams(gpu):
    """swmi_local_full_device on torch buffers, two calls on two streams issued before either is waited for, each equal to
    the host entry; one traceback, one ends-only."""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, len2, n, seed, tb in ((3000, 5000, 40, 1, True), (1023, 16384, 9, 2, False)):
        a, b = inputs(n, len1, len2, seed)
        mw = gpu.local_full_move_words(len1, len2)
        t = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                 ends=torch.zeros((n, 4), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                 st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((len1, len2, n, a, b, t, tb, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, len2, n, a, b, t, tb, s in jobs:
        gpu.local_full_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 2, t["sc"].data_ptr(), t["ends"].data_ptr(),
                              t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None, stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["st"].cpu().numpy().view(np.uint32))
        want = gpu.local_full(a, b, sm, 2)
        assert_same(got, want, ("device", len1, len2), traceback=tb)
    ms = gpu.local_full_time_device(jobs[0][5]["a"].data_ptr(), 3000, jobs[0][5]["b"].data_ptr(), 5000, 40, sm, 2,
                                    jobs[0][5]["sc"].data_ptr(), jobs[0][5]["ends"].data_ptr(), iters=2)
    assert ms > 0


def test_host_entry_from_two_threads(gpu, oracle):
    a, b = inputs(300, 900, 1500, 9)
    sm = match_matrix(5, -4)
    want = oracle.align(a, b, sm, 0)
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.local_full(a, b, sm, 0)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert_same(out[k], want, k)


# ---- 7. the C++ overloads ----------------------------------------------------------------------------------------------------

def _checksum(path):
    want = 0
    for i, j in path:
        want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
    return want


def _run_compat(exe, tmp_path, name, a, b, sm, gap, piece):
    data = tmp_path / name
    with open(data, "wb") as fh:
        fh.write(np.array([a.shape[0], a.shape[1], b.shape[1], gap], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(a.shape[0]):
            fh.write(a[k].tobytes() + b[k].tobytes())
    run = subprocess.run([exe, str(data), str(piece)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-2:] == ["single 0", "ragged 1"], lines[-2:]
    rows = [tuple(map(int, line.split())) for line in lines[:-2]]
    assert len(rows) == a.shape[0]
    return rows


def test_cpp_overloads(gpu, oracle, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "compat_local_full")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local_full.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    # F7's reference paths at len2 = 128, in pieces of 5
    a, b, f7_scores, f7_paths = f7_by_length()[1000]
    rows = _run_compat(exe, tmp_path, "f7.bin", a, b, K111, 1, 5)
    for k, path in enumerate(f7_paths):
        assert rows[k] == (int(f7_scores[k]), len(path), int(path[-1][0]), int(path[-1][1]), _checksum(path)), k
    # one batch with len2 > 128 against the restatement, in one piece
    a, b = inputs(10, 1200, 2300, 71)
    sm = random_matrix()
    sc, ends, mv, st = oracle.align(a, b, sm, 3)
    rows = _run_compat(exe, tmp_path, "long.bin", a, b, sm, 3, 0)
    for k in range(10):
        path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
        assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), _checksum(path)), k
