"""The long wide-alphabet aligners (libswmi_wide_long.so, swmi.wide_long) on the GPU.  Every comparison is exact integer
equality; move words are compared up to `steps`.  Tests that touch striped shapes run once per shipped stripe width (1 and 4
wavefronts, through set_stripe_waves) and once under the library's own rule (0).

Both kinds, with a traceback and ends-only, against the C restatement tests/native/wide_affine_oracle.c at a stripe of one
column at every width, a wave edge inside a stripe and the stripe edges of 1024 and 4096 columns (and 2048, which is one of both), on all 32 letters with
junk in the bytes' high bits, under five matrices; shapes that are striped because of len1 alone; 65536 in either place; shapes
of the unstriped kernels in the same call; all 16 masks; a gap run and ties across stripe edges; zero lengths; the old domain
against swmi.wide; DNA-coded batches against the merged 4-letter long aligners, up to 65536 x 65536; the device entries on two
streams; the C++ overloads.

One case needs a note: at 65536 x 65536 the GLOBAL kind cannot take embed_dna's matrix, whose filler of -128 makes P = 128 and
P (len1 + len2) = 2^24, outside the kind's domain rule (include/swmi_wide_long.h).  That case embeds the same 4 x 4 matrix with a filler of -64 (P = 64, exactly 2^23); the letters are 0 .. 3, so the filler is never read and the
comparison with swmi.global_long is the same."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from wide_support import (ALL_MASKS, END2, GLOBAL, LOCAL, WideOracle, assert_same, asymmetric_matrix, concat, inputs, moves_of, offsets,
                          only_letter_31, scoring_matrix)

pytestmark = pytest.mark.gpu

LEN1S = [1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [4097, 4111, 4112, 4113, 5120, 5121, 6145, 8191, 8192, 8193, 12289]
GRID = [(p, q) for p in LEN1S for q in LEN2S]
# (2049, 8193) and (4500, 8300) lie at indices that are multiples of 3: their seq2 ends in a noisy copy of seq1 (wide_support.inputs)
EXTRA = [(2049, 8193), (16385, 1), (16385, 17), (4500, 8300), (20000, 1025), (200, 4096), (16384, 3)]
LONGEST = [(65536, 3), (3, 65536), (1, 65536)]
EDGE = [(3, 65533)] * 3              # the global kind's domain edge under the all -128 matrix: 128 * 65536 = 2^23
SHAPES = GRID + EXTRA + LONGEST
SHAPES_EDGE = GRID + EXTRA + EDGE
assert len(GRID) % 3 == 0 and SHAPES.index((2049, 8193)) % 3 == 0 and SHAPES.index((4500, 8300)) % 3 == 0
MATRICES = {"asymmetric": lambda: scoring_matrix(3), "random_int8": lambda: asymmetric_matrix(4), "all_-128": lambda: np.full(1024, -128, np.int8),
            "all_127": lambda: np.full(1024, 127, np.int8), "only_31": only_letter_31}
GAPS = {"asymmetric": (6, 1), "random_int8": (40, 9), "all_-128": (3, 2), "all_127": (0, 0), "only_31": (2, 1)}
WIDTHS = [0, 1, 4]


@pytest.fixture(scope="module")
def woracle(tmp_path_factory):
    return WideOracle(tmp_path_factory.mktemp("wide_long_gpu_oracle"))


@pytest.fixture(scope="module")
def wl(swmi_mod):
    """The library needs no swmi.init(): it runs on the current device."""
    swmi_mod.wide_long.load()
    return swmi_mod.wide_long


@pytest.fixture(params=WIDTHS)
def width(wl, request):
    wl.set_stripe_waves(request.param)
    yield request.param
    wl.set_stripe_waves(0)


@pytest.fixture(scope="module")
def batches():
    """The edge shapes in one batch (and the variant for the global kind under the all -128 matrix), with a permutation; never
    changed by a test."""
    out = {}
    for name, shapes in (("all", SHAPES), ("edge", SHAPES_EDGE)):
        a, b = inputs(shapes, seed=7)
        out[name] = (a, b, np.random.default_rng(8).permutation(len(a)))
    return out


_WANT = {}


def _want(woracle, key, kind, a, b, sm, gaps, mask, traceback=True):
    """The restatement's result, computed once per case and shared by the widths."""
    key = (key, kind, mask, traceback)
    if key not in _WANT:
        _WANT[key] = woracle.align(kind, a, b, sm, gaps[0], gaps[1], mask, traceback=traceback)
    return _WANT[key]


def _run(wl, kind, a, b, sm, gaps, mask, traceback):
    if kind == LOCAL:
        return wl.local(a, b, sm, gaps[0], gaps[1], traceback=traceback)
    return wl.global_(a, b, sm, gaps[0], gaps[1], mask, traceback=traceback)


@pytest.mark.parametrize("matrix", sorted(MATRICES))
@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_edges_equal_the_restatement(wl, woracle, batches, width, kind, matrix):
    sm, gaps = MATRICES[matrix](), GAPS[matrix]
    # the global kind's domain rule decides which batch it takes: with P = 128 (a matrix that holds -128) the three shapes with
    # a 65536 lie outside it and (3, 65533), its edge, stands in; the all 127 matrix with gaps (0, 0) keeps them
    P = max(1, int(np.abs(sm.astype(np.int32)).max()), *gaps)
    outside = kind == GLOBAL and P * 65539 > 1 << 23
    assert outside == (kind == GLOBAL and matrix in ("all_-128", "random_int8")) and (not outside or P * 65536 == 1 << 23)
    a, b, perm = batches["edge" if outside else "all"]
    for mask in ([0] if kind == LOCAL else [0, 15, 10, 5]):
        want = _want(woracle, matrix, kind, a, b, sm, gaps, mask)
        print(kind, matrix, mask, "width", width, "scores", int(want[0].min()), int(want[0].max()), "steps", int(want[4].max()))
        assert_same(_run(wl, kind, a, b, sm, gaps, mask, True), want, (kind, matrix, mask, width, "traceback"))
        ends_only = _want(woracle, matrix, kind, a, b, sm, gaps, mask, traceback=False)
        assert_same(_run(wl, kind, a, b, sm, gaps, mask, False), ends_only, (kind, matrix, mask, width, "ends-only"), traceback=False)
    # permuted: every result follows its alignment
    pa, pb = [a[k] for k in perm], [b[k] for k in perm]
    mask = 0 if kind == LOCAL else 10
    assert_same(_run(wl, kind, pa, pb, sm, gaps, mask, True), _want(woracle, matrix + "/perm", kind, pa, pb, sm, gaps, mask),
                (kind, matrix, width, "permuted"))


def test_the_letters_and_the_paths_are_not_trivial(woracle, batches):
    """What the comparisons above rest on: all 32 letters and junk bits occur; under the scoring matrix the paths hold all three
    kinds of move; a global path visits every column, so the paths of the widest shapes cross every stripe edge; and the LOCAL
    path of (4500, 8300) runs diagonally through column 4096, column 8192 and every multiple of 1024 between them."""
    a, b, _ = batches["all"]
    cat = np.concatenate(a + b)
    assert len(np.unique(cat & 31)) == 32 and len(np.unique(cat >> 5)) == 8
    sm, gaps = scoring_matrix(3), GAPS["asymmetric"]
    want = _want(woracle, "asymmetric", GLOBAL, a, b, sm, gaps, 0)
    kinds = set()
    for k in range(0, len(a), 3):
        kinds |= set(moves_of(want, k))
    assert kinds == {1, 2, 3}
    k = SHAPES.index((200, 12289))
    assert int(want[1][k, 1]) == 12289 and tuple(want[1][k, 2:]) == (0, 0) and int(want[4][k]) >= 12289
    local = _want(woracle, "asymmetric", LOCAL, a, b, sm, gaps, 0)
    k = SHAPES.index((4500, 8300))
    i, j = int(local[1][k, 0]), int(local[1][k, 1])
    diagonal_columns = set()
    for m in moves_of(local, k):
        if m == 3:
            diagonal_columns.add(j)
        i -= m != 1
        j -= m != 2
    assert (i, j) == tuple(local[1][k, 2:]) and j < 4096 and int(local[1][k, 1]) > 8192
    assert all(c in diagonal_columns or c + 1 in diagonal_columns for c in range(4096, 8193, 1024)), sorted(diagonal_columns)[:4]
    assert {1, 2} & set(moves_of(local, k))
    k = SHAPES.index((2049, 8193))      # its walk crosses staging blocks (128 rows, 512 columns) and stripe edges
    assert int(local[1][k, 0]) - int(local[1][k, 2]) > 3 * 128 and int(local[1][k, 3]) + 3 * 512 < int(local[1][k, 1]) and int(local[1][k, 3]) < 7168 < int(local[1][k, 1])


def test_all_16_masks(wl, woracle, width):
    shapes = [(p, q) for p in (1, 2, 31, 32) for q in (4097, 8193)]
    a, b = inputs(shapes, seed=17)
    sm = scoring_matrix(5)
    for mask in ALL_MASKS:
        assert_same(wl.global_(a, b, sm, 4, 1, mask), _want(woracle, "masks", GLOBAL, a, b, sm, (4, 1), mask), ("masks", mask, width))
        assert_same(wl.global_(a, b, sm, 4, 1, mask, traceback=False), _want(woracle, "masks", GLOBAL, a, b, sm, (4, 1), mask, traceback=False),
                    ("masks ends-only", mask, width), traceback=False)


def _left_runs(result, k):
    """(first column, last column) of every run of left moves on alignment k's path."""
    j = int(result[1][k, 1])
    runs, run_end = [], None
    for m in moves_of(result, k):
        if m == 1:
            run_end = j if run_end is None else run_end
        elif run_end is not None:
            runs.append((j + 1, run_end))
            run_end = None
        j -= m != 2
    if run_end is not None:
        runs.append((j + 1, run_end))
    return runs


@pytest.mark.parametrize("at", [4080, 5100])
def test_a_gap_across_a_stripe_edge(wl, woracle, width, at):
    """seq2 is seq1 with 40 letters inserted behind column `at`: one left-run over at + 1 .. at + 40, across column 4096 (a
    stripe edge at every width) or 5120 (at width 1).  With gaps (40, 1) a run that re-opened at the edge would cost 39 more."""
    rng = np.random.default_rng(at)
    x = rng.integers(0, 20, at + 300, dtype=np.uint8)
    y = np.concatenate([x[:at], rng.integers(20, 32, 40, dtype=np.uint8), x[at:]]).astype(np.uint8)
    sm = np.full((32, 32), -4, np.int8)
    np.fill_diagonal(sm, 5)
    sm = sm.reshape(-1)
    for kind in (LOCAL, GLOBAL):
        want = _want(woracle, ("gap", at), kind, [x], [y], sm, (40, 1), 0)
        assert (at + 1, at + 40) in _left_runs(want, 0), _left_runs(want, 0)
        assert int(want[0][0]) == 5 * len(x) - 40 - 39
        assert_same(_run(wl, kind, [x], [y], sm, (40, 1), 0, True), want, ("gap", at, kind, width))


def test_ties_across_stripes(wl, woracle, width):
    sm = np.full((32, 32), -3, np.int8)
    sm[31, 31] = sm[30, 30] = 5
    sm = sm.reshape(-1)
    # local kind: two equal best cells, the later stripe's at the smaller row -> that one; then equal rows -> the earlier column
    x1 = np.full(40, 1, np.uint8)
    x1[19], x1[9] = 31, 30                      # rows 20 and 10
    y1 = np.zeros(6000, np.uint8)
    y1[99], y1[4999] = 31, 30                   # columns 100 and 5000
    x2 = np.full(40, 1, np.uint8)
    x2[9] = 31
    y2 = np.zeros(6000, np.uint8)
    y2[99] = y2[4999] = 31
    want = _want(woracle, "ties local", LOCAL, [x1, x2], [y1, y2], sm, (2, 1), 0)
    assert want[0].tolist() == [5, 5] and want[1][:, :2].tolist() == [[10, 5000], [10, 100]]
    assert_same(wl.local([x1, x2], [y1, y2], sm, 2, 1), want, ("ties local", width))
    assert_same(wl.local([x1, x2], [y1, y2], sm, 2, 1, traceback=False), _want(woracle, "ties local", LOCAL, [x1, x2], [y1, y2], sm, (2, 1), 0, traceback=False),
                ("ties local ends-only", width), traceback=False)
    # global kind with seq2's end free: equal last-row cells in two stripes -> the earlier column; also at gaps (0, 0), where
    # every later cell of the last row ties
    mm = np.full((32, 32), -3, np.int8)
    np.fill_diagonal(mm, 5)
    mm = mm.reshape(-1)
    p = np.arange(8, 16, dtype=np.uint8)
    y = np.full(9000, 7, np.uint8)
    y[92:100] = p
    y[4992:5000] = p
    y[8492:8500] = p
    for gaps in ((4, 1), (0, 0)):
        for mask in (END2 | 2, END2):
            want = _want(woracle, ("ties global", gaps), GLOBAL, [p], [y], mm, gaps, mask)
            if mask == END2 | 2:
                assert int(want[0][0]) == 40 and want[1][0, :2].tolist() == [8, 100]
            assert int(want[1][0, 0]) == 8 and int(want[1][0, 1]) <= 4096
            assert_same(wl.global_([p], [y], mm, gaps[0], gaps[1], mask), want, ("ties global", gaps, mask, width))


def test_zero_lengths(wl, woracle):
    shapes = [(0, 0), (0, 65536), (65536, 0), (0, 4097), (16385, 0)]
    a, b = inputs(shapes, seed=23)
    sm = scoring_matrix(6)
    assert_same(wl.local(a, b, sm, 3, 1), woracle.align(LOCAL, a, b, sm, 3, 1), "zero local")
    assert_same(wl.local(a, b, sm, 3, 1, traceback=False), woracle.align(LOCAL, a, b, sm, 3, 1, traceback=False), "zero local", traceback=False)
    for mask in ALL_MASKS:
        assert_same(wl.global_(a, b, sm, 3, 1, mask), woracle.align(GLOBAL, a, b, sm, 3, 1, mask), ("zero global", mask))
        assert_same(wl.global_(a, b, sm, 3, 1, mask, traceback=False), woracle.align(GLOBAL, a, b, sm, 3, 1, mask, traceback=False),
                    ("zero global", mask), traceback=False)


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_the_old_domain_equals_swmi_wide(wl, swmi_mod, kind):
    """On test_wide_gpu.py's SHAPES batch every field and move is swmi.wide's: the same kernels run."""
    from test_wide_gpu import SHAPES as OLD_SHAPES
    wide = swmi_mod.wide
    a, b = inputs(OLD_SHAPES, seed=7)
    sm = scoring_matrix(3)
    for mask in ([0] if kind == LOCAL else [0, 10, 15]):
        for tb in (True, False):
            if kind == LOCAL:
                want = wide.local(a, b, sm, 6, 1, traceback=tb)
            else:
                want = wide.global_(a, b, sm, 6, 1, mask, traceback=tb)
            assert_same(_run(wl, kind, a, b, sm, (6, 1), mask, tb), want, ("old domain", kind, mask, tb), traceback=tb)


def _dna(n, len1, len2, seed):
    """seq2 a mutated copy of (the head of) seq1, cyclically extended: long paths with every kind of move."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = a[:, :len2] if len2 <= len1 else np.concatenate([a, rng.integers(0, 4, (n, len2 - len1), dtype=np.uint8)], axis=1)
    b = np.where(rng.random((n, len2)) < 0.9, b, rng.integers(0, 4, (n, len2), dtype=np.uint8)).astype(np.uint8)
    for k in range(n):                          # an indel each
        b[k, 1000:] = np.roll(b[k, 1000:], 7)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


DNA16 = np.asarray([2 if x == y else -3 for x in range(4) for y in range(4)], np.int8)


def _fixed_as_ragged(wl, a, b, r, traceback=True):
    if not traceback:
        return r[0], r[1], None, None, None
    mo = wl.move_offsets(offsets(list(a)), offsets(list(b)))
    return r[0], r[1], np.ascontiguousarray(r[2]).reshape(-1), mo, r[3]


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_dna_equals_the_merged_long_aligners(gpu, wl, width, kind):
    a, b = _dna(4, 5000, 20000, 31)
    sm32 = wl.embed_dna(DNA16)
    for tb in (True, False):
        if kind == LOCAL:
            want = gpu.local_long.local_long_affine(a, b, DNA16, 5, 1, traceback=tb)
            got = wl.local(list(a), list(b), sm32, 5, 1, traceback=tb)
        else:
            want = gpu.global_long.global_long_affine(a, b, DNA16, 5, 1, 0, traceback=tb)
            got = wl.global_(list(a), list(b), sm32, 5, 1, 0, traceback=tb)
        assert_same(got, _fixed_as_ragged(wl, a, b, want, tb), ("dna", kind, tb, width), traceback=tb)
        assert int(np.abs(want[0]).max()) > 1000


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_dna_at_65536_squared_equals_the_merged_long_aligners(gpu, wl, kind):
    """One alignment of 65536 x 65536 with a traceback, at the library's own stripe width.  (The module's docstring says why the
    global kind's filler is -64.)"""
    a, b = _dna(1, 65536, 65536, 33)
    if kind == LOCAL:
        sm32 = wl.embed_dna(DNA16)
        want = gpu.local_long.local_long_affine(a, b, DNA16, 5, 1)
        got = wl.local(list(a), list(b), sm32, 5, 1)
    else:
        sm32 = np.full((32, 32), -64, np.int8)
        sm32[:4, :4] = DNA16.reshape(4, 4)
        sm32 = sm32.reshape(-1)
        want = gpu.global_long.global_long_affine(a, b, DNA16, 5, 1, 0)
        got = wl.global_(list(a), list(b), sm32, 5, 1, 0)
    assert_same(got, _fixed_as_ragged(wl, a, b, want), ("dna 65536", kind))
    assert int(want[3][0]) >= 65536
    gpu.local_long.local_long_affine_release_workspaces()
    gpu.global_long.global_long_affine_release_workspaces()
    wl.release_workspaces()


def test_device_entries_on_two_streams_in_flight(wl, woracle, width):
    """Both device entries on torch buffers, four calls on two streams issued before either is waited for."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(41)
    sm = scoring_matrix(11)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    for x, (kind, tb, n, mask) in enumerate(((LOCAL, True, 30, 0), (GLOBAL, True, 20, 15), (LOCAL, False, 40, 0), (GLOBAL, False, 30, 10))):
        shapes = [(int(p), int(q)) for p, q in zip(rng.integers(0, 600, n), rng.integers(0, 9000, n))] + [(40, 4096), (33, 4097), (16400, 5)]
        a, b = inputs(shapes, seed=50 + x)
        off1, off2 = offsets(a), offsets(b)
        mo = wl.move_offsets(off1, off2)
        m = len(a)
        t = dict(a=torch.from_numpy(concat(a)).to(dev), b=torch.from_numpy(concat(b)).to(dev),
                 sc=torch.zeros(m, dtype=torch.int32, device=dev), ends=torch.zeros((m, 4), dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]) + 2, dtype=torch.int64, device=dev), st=torch.zeros(m, dtype=torch.int32, device=dev))
        jobs.append((kind, tb, mask, a, b, off1, off2, mo, t, streams[x % 2]))
    torch.cuda.synchronize()
    for kind, tb, mask, a, b, off1, off2, mo, t, s in jobs:
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None)
        if kind == LOCAL:
            wl.local_device(t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            wl.global_device(t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, mask, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for x, (kind, tb, mask, a, b, off1, off2, mo, t, s) in enumerate(jobs):
        want = _want(woracle, ("device", x), kind, a, b, sm, (7, 1), mask, traceback=tb)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64) if tb else None, mo if tb else None,
               t["st"].cpu().numpy().view(np.uint32) if tb else None)
        assert_same(got, want, ("device", kind, tb, width), traceback=tb)
        assert np.any(want[0] != 0)
    # the timer runs the same launches
    kind, tb, mask, a, b, off1, off2, mo, t, s = jobs[1]
    ms = wl.time_device(wl.GLOBAL, t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, mask, t["sc"].data_ptr(), t["ends"].data_ptr(),
                        t["mv"].data_ptr(), t["st"].data_ptr(), stream=s.cuda_stream, iters=2)
    assert ms > 0
    wl.release_workspaces()


def test_cpp_overloads_on_a_mixed_batch(wl, woracle, swmi_mod, tmp_path):
    """tests/native/compat_wide_long.cpp, built by g++ against the libraries: 20 mixed alignments in pieces of 8, (0, 5), (5, 0),
    (700, 5000) and (16400, 40) among them; it prints score, path length, start cell, end cell and a path checksum, which the
    restatement confirms."""
    assert shutil.which("g++") is not None
    rng = np.random.default_rng(61)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(0, 900, 16), rng.integers(0, 6000, 16))] + [(0, 5), (5, 0), (700, 5000), (16400, 40)]
    a, b = inputs(shapes, 62)
    sm = scoring_matrix(15)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.ascontiguousarray(sm, np.int8).tobytes())
        fh.write(np.int32(len(a)).tobytes())
        for x, y in zip(a, b):
            fh.write(np.int32([len(x), len(y)]).tobytes() + x.tobytes() + y.tobytes())
    exe = str(tmp_path / "compat_wide_long")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "compat_wide_long.cpp"),
                            "-o", exe, "-L", lib, "-lswmi_wide_long", "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "mismatches 0", lines[-1]

    def checksum(path):
        want = 0
        for i, j in path:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        return want

    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == 3 * len(a)
    at = 0
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0), (GLOBAL, 10)):
        sc, ends, moves, mo, steps = woracle.align(kind, a, b, sm, 7, 2, mask)
        for k in range(len(a)):
            row = moves[int(mo[k]):int(mo[k + 1])]
            path = swmi_mod.local_long.expand_moves(row, steps[k], ends[k, 0], ends[k, 1]) if steps[k] else ends[k, 2:].reshape(1, 2)
            assert rows[at + k] == (int(sc[k]), int(steps[k]) + 1, int(ends[k, 2]), int(ends[k, 3]), int(ends[k, 0]), int(ends[k, 1]),
                                    checksum(path)), (at, k)
        at += len(a)
