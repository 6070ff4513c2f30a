"""The exact semi-global aligners on a batch of mixed (len1, len2) (swmi_semiglobal_full_ragged*,
swmi_semiglobal_full_affine_ragged*) on the GPU.  Every comparison is exact integer equality; move words are compared up to
lengths - 1 steps (bits past the last step are unspecified).  Every field equal to the fixed-length entry called per shape and
to the C restatements tests/native/sgfull_oracle.c / sgfull_affine_oracle.c grouped by shape, at the wave-count edges in len2
(1024 columns per wave, 16 per lane) and the chunk (32 steps) and staging (128 rows) edges in len1; the zero lengths against the
restatements called with length 0 (score 0, ends (0, 0), lengths 1 -- not the local aligners' count of 0); wave counts 1, 2 and
16 side by side; permutations; a host call of two slices; the device entries on two streams; the C++ overloads.

The inputs put the similar region at the START of the sequences: every path of this aligner starts at (0, 0), so a seq2 that
copies its seq1 from position 0 puts the best cell deep in the table and gives the walk real work.  With the edge shapes alone
(len1 <= 200, and (16384, 3), (5, 16384)) no best cell can lie past column 1024 -- a cell (i, j) holds at most
20 min(i, j) - gap |i - j| -- so the edges batch also holds one (1100, 2049) copy pair, whose walk crosses a wave boundary and
several staging blocks; _assert_non_vacuous states what the batch must show, from the restatement's output alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_support import random_matrix
from sgfull_affine_support import SgAffineOracle
from sgfull_support import SgFullOracle

pytestmark = pytest.mark.gpu

LEN1S = [1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [1, 15, 16, 17, 1023, 1024, 1025, 2049]
EXTRA = [(16384, 3), (5, 16384), (1100, 2049, "copy")]
ZERO_SHAPES = [(0, 0), (0, 1), (1, 0), (0, 33), (33, 0), (0, 1025), (16384, 0), (0, 16384)]


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_ragged_oracle"))


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_ragged_affine_oracle"))


def _kind(k, shape):
    if len(shape) > 2:
        return shape[2]
    return "copy" if k % 3 == 0 else "homopolymer" if k % 7 == 1 else "random"


def _inputs(shapes, seed):
    """Pairs of the given (len1, len2[, kind]): every third seq2 starts with a 90 % copy of its seq1 FROM POSITION 0, with one
    deletion and one insertion of 5 bases where the length allows; every seventh pair a homopolymer against a mostly equal one
    (ties); the rest random.  Returns (seq1s, seq2s, kinds)."""
    rng = np.random.default_rng(seed)
    a, b, kinds = [], [], []
    for k, shape in enumerate(shapes):
        len1, len2 = shape[:2]
        kind = _kind(k, shape)
        x = rng.integers(0, 4, len1, dtype=np.uint8)
        y = rng.integers(0, 4, len2, dtype=np.uint8)
        w = min(len1, len2)
        if kind == "copy" and w:
            src = np.where(rng.random(len1) < 0.9, x, rng.integers(0, 4, len1)).astype(np.uint8)
            if w > 24:
                c1 = int(rng.integers(2, w // 2 - 5))
                c2 = int(rng.integers(w // 2, w - 6))
                src = np.concatenate([src[:c1], src[c1 + 5:c2], rng.integers(0, 4, 5, dtype=np.uint8), src[c2:]])
            y[:w] = src[:w]
        elif kind == "homopolymer":
            x[:] = k & 3
            y[rng.random(len2) < 0.8] = k & 3
        a.append(x)
        b.append(y)
        kinds.append(kind)
    return a, b, kinds


def _by_shape(a, b, fn, traceback=True):
    """What a fixed-shape aligner `fn(seq1s[m, len1], seq2s[m, len2])` gives, alignment by alignment, run once per distinct
    shape: (scores, ends[n, 2], lengths, list of move rows).  A shape with a zero length goes to `fn` as well (the restatements
    take length 0)."""
    n = len(a)
    sc = np.zeros(n, np.int32)
    ends = np.zeros((n, 2), np.int32)
    lengths = np.zeros(n, np.uint32)
    rows = [np.zeros(0, np.uint64)] * n
    groups = {}
    for k in range(n):
        groups.setdefault((len(a[k]), len(b[k])), []).append(k)
    for (len1, len2), idx in groups.items():
        r = fn(np.stack([a[k] for k in idx]).reshape(len(idx), len1), np.stack([b[k] for k in idx]).reshape(len(idx), len2))
        sc[idx], ends[idx] = r[0], r[1]
        if traceback:
            lengths[idx] = r[3]
            for x, k in enumerate(idx):
                rows[k] = r[2][x]
    return sc, ends, lengths, rows


def _assert_ragged(got, want, what, traceback=True):
    sc, ends, moves, mo, lengths = got
    wsc, wends, wlengths, wrows = want
    assert ends.shape == (len(sc), 2)
    assert np.array_equal(sc, wsc), (what, np.flatnonzero(sc != wsc)[:8])
    assert np.array_equal(ends, wends), (what, np.flatnonzero((ends != wends).any(axis=1))[:8])
    if not traceback:
        assert moves is None and mo is None and lengths is None
        return
    assert np.array_equal(lengths, wlengths), (what, np.flatnonzero(lengths != wlengths)[:8])
    for k in range(len(sc)):
        full, part = divmod(int(lengths[k]) - 1, 32)
        at = int(mo[k])
        assert np.array_equal(moves[at:at + full], wrows[k][:full]), (what, k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (moves[at + full] & mask) == (wrows[k][full] & mask), (what, k)


def _rows_of(result, n):
    return [result[2][int(result[3][k]):int(result[3][k + 1])] for k in range(n)]


def _codes_present(rows, lengths):
    seen = set()
    for row, length in zip(rows, lengths):
        t = np.arange(int(length) - 1)
        if len(t):
            seen |= set(np.unique((row[t // 32] >> (2 * (t % 32)).astype(np.uint64)) & np.uint64(3)).tolist())
    return seen


def _assert_non_vacuous(b, kinds, want):
    """From the restatement's output alone: some alignment with len2 >= 1025 ends past column 1024 with a path of more than 129
    cells (the walk crosses a wave boundary and a staging block); the batch's moves hold all three codes; some random pair has
    score 0 at (0, 0)."""
    sc, ends, lengths, rows = want
    assert any(len(b[k]) >= 1025 and ends[k, 1] > 1024 and lengths[k] > 129 for k in range(len(b)))
    assert _codes_present(rows, lengths) == {1, 2, 3}
    assert any(kinds[k] == "random" and sc[k] == 0 and tuple(ends[k]) == (0, 0) and lengths[k] == 1 for k in range(len(b)))


@pytest.fixture(scope="module")
def mixed():
    shapes = [(x, y) for x in LEN1S for y in LEN2S for _ in range(2)] + EXTRA
    order = np.random.default_rng(3).permutation(len(shapes))
    return _inputs([shapes[k] for k in order], 7)


@pytest.fixture(scope="module")
def mixed_restated(mixed, loracle, aoracle):
    """The restatements' results on the edges batch, computed once per parameter set and shared by both traceback modes."""
    a, b, _ = mixed
    done = {}

    def get(sm, *gaps):
        key = (bytes(np.asarray(sm, np.int8)), gaps)
        if key not in done:
            oracle = loracle if len(gaps) == 1 else aoracle
            done[key] = _by_shape(a, b, lambda x, y: oracle.align(x, y, sm, *gaps))
        return done[key]

    return get


@pytest.mark.parametrize("traceback", [True, False])
def test_edges_equal_the_fixed_entries_and_the_restatements(gpu, mixed, mixed_restated, traceback):
    """One shuffled batch of two pairs of every (len1, len2) of the edges, plus 16384 on either side and the deep copy pair:
    field by field the fixed-length entry called once per distinct shape and the C restatements grouped by shape, for linear
    (2, -3, 2) and a random matrix at gap 6 and for affine (5, 1) and (1, 4); open == extend equals the linear call."""
    a, b, kinds = mixed
    sr = gpu.semiglobal_ragged
    assert len(a) == 2 * len(LEN1S) * len(LEN2S) + 3
    linear = {}
    for sm, gap in ((match_matrix(2, -3), 2), (random_matrix(), 6)):
        got = sr.semiglobal_full_ragged(a, b, sm, gap, traceback=traceback)
        linear[gap] = (sm, got)
        _assert_ragged(got, _by_shape(a, b, lambda x, y: gpu.semiglobal_full(x, y, sm, gap, traceback=traceback), traceback),
                       ("linear", gap), traceback)
        want = mixed_restated(sm, gap)
        if gap == 2:
            _assert_non_vacuous(b, kinds, want)
        _assert_ragged(got, want if traceback else (want[0], want[1], None, None), ("linear restatement", gap), traceback)
    for sm, (go, ge) in ((match_matrix(2, -3), (5, 1)), (random_matrix(), (1, 4))):
        got = sr.semiglobal_full_affine_ragged(a, b, sm, go, ge, traceback=traceback)
        _assert_ragged(got, _by_shape(a, b, lambda x, y: gpu.semiglobal_full_affine(x, y, sm, go, ge, traceback=traceback), traceback),
                       ("affine", go, ge), traceback)
        want = mixed_restated(sm, go, ge)
        if (go, ge) == (5, 1):
            _assert_non_vacuous(b, kinds, want)
        _assert_ragged(got, want if traceback else (want[0], want[1], None, None), ("affine restatement", go, ge), traceback)
    for gap, (sm, lin) in linear.items():
        eq = sr.semiglobal_full_affine_ragged(a, b, sm, gap, gap, traceback=traceback)
        _assert_ragged(eq, (lin[0], lin[1], lin[4], _rows_of(lin, len(a)) if traceback else None), ("open = extend", gap), traceback)


@pytest.fixture(scope="module")
def with_zeros():
    shapes = ZERO_SHAPES + [(5, 7), (40, 1030), (3, 3), (1, 1)] + ZERO_SHAPES[1:4]
    order = np.random.default_rng(5).permutation(len(shapes))
    return _inputs([shapes[k] for k in order], 9)


def test_zero_lengths(gpu, loracle, aoracle, with_zeros):
    """The zero lengths, mixed with non-empty alignments: every field equal to the restatements called directly with length 0,
    which give score 0, ends (0, 0) and lengths == 1 (the one position (0, 0)), also at gap 0; ends-only the same score and
    ends.  A kernel with the local aligners' zero-length arm writes a count of 0 and fails `lengths == 1`."""
    a, b, _ = with_zeros
    sr = gpu.semiglobal_ragged
    sm = match_matrix(2, -3)
    n = len(a)
    zero = [k for k in range(n) if len(a[k]) == 0 or len(b[k]) == 0]
    assert len(zero) == len(ZERO_SHAPES) + 3
    cases = [("linear", (gap,)) for gap in (3, 0)] + [("affine", gaps) for gaps in ((5, 1), (0, 2), (4, 4))]
    for kind, gaps in cases:
        run = sr.semiglobal_full_ragged if kind == "linear" else sr.semiglobal_full_affine_ragged
        oracle = loracle if kind == "linear" else aoracle
        got = run(a, b, sm, *gaps)
        want = _by_shape(a, b, lambda x, y: oracle.align(x, y, sm, *gaps))
        assert np.all(want[0][zero] == 0) and np.all(want[1][zero] == 0) and np.all(want[2][zero] == 1)
        _assert_ragged(got, want, (kind, gaps, "restatement"))
        sc, ends, moves, mo, lengths = got
        assert np.all(sc[zero] == 0) and np.all(ends[zero] == 0), (kind, gaps)
        assert np.all(lengths[zero] == 1), (kind, gaps, lengths[zero])
        assert np.any(sc != 0)
        eo = run(a, b, sm, *gaps, traceback=False)
        assert eo[2] is None and eo[3] is None and eo[4] is None
        assert np.array_equal(eo[0], sc) and np.array_equal(eo[1], ends)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_extremes_side_by_side(gpu, loracle, aoracle, n):
    """Wave counts 1, 2 and 16 in one slice and rows 1 .. 16384 in adjacent workgroups, against the restatements."""
    cycle = [(1, 16384), (16384, 1), (33, 16384), (16384, 17), (2, 1025)]
    a, b, _ = _inputs([cycle[k % 5] for k in range(n)], 50 + n)
    sm = match_matrix(2, -3)
    sr = gpu.semiglobal_ragged
    _assert_ragged(sr.semiglobal_full_ragged(a, b, sm, 2), _by_shape(a, b, lambda x, y: loracle.align(x, y, sm, 2)), n)
    _assert_ragged(sr.semiglobal_full_affine_ragged(a, b, sm, 5, 1), _by_shape(a, b, lambda x, y: aoracle.align(x, y, sm, 5, 1)),
                   (n, "affine"))


def test_permuting_a_batch_permutes_its_results(gpu):
    rng = np.random.default_rng(11)
    a, b, _ = _inputs([(int(x), int(y)) for x, y in rng.integers(0, 1501, (300, 2))], 12)
    perm = rng.permutation(len(a))
    sm = match_matrix(2, -3)
    sr = gpu.semiglobal_ragged
    for run in (lambda x, y: sr.semiglobal_full_ragged(x, y, sm, 3), lambda x, y: sr.semiglobal_full_affine_ragged(x, y, sm, 6, 2)):
        sc, ends, moves, mo, lengths = run(a, b)
        assert sc.max() > 0 and lengths.max() > 33
        psc, pends, pmoves, pmo, plengths = run([a[k] for k in perm], [b[k] for k in perm])
        assert np.array_equal(psc, sc[perm]) and np.array_equal(pends, ends[perm]) and np.array_equal(plengths, lengths[perm])
        for x, k in enumerate(perm):
            w = (int(lengths[k]) - 1) // 32
            assert np.array_equal(pmoves[int(pmo[x]):int(pmo[x]) + w], moves[int(mo[k]):int(mo[k]) + w])


def _tiny_tables(cat1, off1, cat2, off2, match, mismatch, gap):
    """(scores, best cells) of n tables of at most 5 x 5 cells (lengths 0 .. 4), vectorised over the alignments: charged
    borders, the 16 inner cells in a closed loop, then the best-cell rule over the cells of the alignment's own table in
    row-major order (the first cell strictly above every earlier one, from 0 at (0, 0))."""
    n = len(off1) - 1
    len1 = (off1[1:] - off1[:-1]).astype(np.int64)
    len2 = (off2[1:] - off2[:-1]).astype(np.int64)
    pad1 = np.concatenate([cat1, np.zeros(8, np.uint8)])
    pad2 = np.concatenate([cat2, np.zeros(8, np.uint8)])
    H = np.zeros((n, 5, 5), np.int64)
    for x in range(1, 5):
        H[:, x, 0] = -x * gap
        H[:, 0, x] = -x * gap
    for i in range(1, 5):
        for j in range(1, 5):
            x = pad1[off1[:-1].astype(np.int64) + i - 1] & 3
            y = pad2[off2[:-1].astype(np.int64) + j - 1] & 3
            H[:, i, j] = np.maximum(H[:, i - 1, j - 1] + np.where(x == y, match, mismatch), np.maximum(H[:, i - 1, j], H[:, i, j - 1]) - gap)
    best = np.zeros(n, np.int64)
    end = np.zeros((n, 2), np.int64)
    for i in range(5):
        for j in range(5):
            better = (i <= len1) & (j <= len2) & (H[:, i, j] > best)
            best = np.where(better, H[:, i, j], best)
            end[better] = (i, j)
    return best.astype(np.int32), end.astype(np.int32)


def test_host_call_of_two_slices(gpu):
    """2^20 + 5 alignments with lengths in [0, 4], ends-only: two slices by the count cap.  (The budget-driven traceback split
    runs on the fake GPU, tests/test_sgfull_ragged_host_fake.py.)"""
    rng = np.random.default_rng(21)
    n = (1 << 20) + 5
    off1 = np.zeros(n + 1, np.uint64)
    off2 = np.zeros(n + 1, np.uint64)
    off1[1:] = np.cumsum(rng.integers(0, 5, n))
    off2[1:] = np.cumsum(rng.integers(0, 5, n))
    cat1 = rng.integers(0, 3, int(off1[-1]), dtype=np.uint8)
    cat2 = rng.integers(0, 3, int(off2[-1]), dtype=np.uint8)
    sr = gpu.semiglobal_ragged
    assert sr.semiglobal_full_ragged_slices_for(off1, off2, affine=False, traceback=False) == [1 << 20, 5]
    want_sc, want_end = _tiny_tables(cat1, off1, cat2, off2, 3, -2, 1)
    assert want_sc.max() == 12 and want_sc.min() == 0 and np.any((want_sc == 0) & (off1[1:] > off1[:-1]) & (off2[1:] > off2[:-1]))
    for affine in (False, True):                        # open == extend == 1: the linear table
        if affine:
            got = sr.semiglobal_full_affine_ragged((cat1, off1), (cat2, off2), match_matrix(3, -2), 1, 1, traceback=False)
        else:
            got = sr.semiglobal_full_ragged((cat1, off1), (cat2, off2), match_matrix(3, -2), 1, traceback=False)
        sc, ends, moves, mo, lengths = got
        assert moves is None and mo is None and lengths is None and ends.shape == (n, 2)
        assert np.array_equal(sc, want_sc), affine
        assert np.array_equal(ends, want_end), affine


def test_device_entries_on_two_streams_in_flight(gpu):
    """Both device entries on torch buffers, four calls (linear and affine, with and without traceback) on two streams issued
    before any is waited for, equal the host entry; the ends buffer holds two int32 per alignment and a guard row behind them."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    sm = random_matrix(5)
    sr = gpu.semiglobal_ragged
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    for x, (affine, tb, n, seed) in enumerate(((False, True, 257, 1), (True, True, 130, 2), (False, False, 300, 3), (True, False, 190, 4))):
        a, b, _ = _inputs([(int(p), int(q)) for p, q in rng.integers(0, 1101, (n, 2))], seed)
        cat1, off1, cat2, off2 = gpu._ragged_pair(a, b)
        mo = gpu.local_full_ragged_move_offsets(off1, off2)
        pad = np.zeros(16, np.uint8)
        t = dict(a=torch.from_numpy(np.concatenate([cat1, pad])).to(dev), b=torch.from_numpy(np.concatenate([cat2, pad])).to(dev),
                 sc=torch.zeros(n, dtype=torch.int32, device=dev), ends=torch.full((n + 2, 2), -77, dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]), dtype=torch.int64, device=dev), ln=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((affine, tb, a, b, off1, off2, t, streams[x % 2]))
    torch.cuda.synchronize()
    for affine, tb, a, b, off1, off2, t, s in jobs:
        args = (t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm)
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["ln"].data_ptr() if tb else None)
        if affine:
            sr.semiglobal_full_affine_ragged_device(*args, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            sr.semiglobal_full_ragged_device(*args, 4, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for affine, tb, a, b, off1, off2, t, s in jobs:
        n = len(a)
        want = sr.semiglobal_full_affine_ragged(a, b, sm, 7, 1, traceback=tb) if affine else sr.semiglobal_full_ragged(a, b, sm, 4, traceback=tb)
        ends = t["ends"].cpu().numpy()
        assert np.all(ends[n:] == -77)                  # nothing past ends[2 n]
        got = (t["sc"].cpu().numpy(), ends[:n], t["mv"].cpu().numpy().view(np.uint64) if tb else None, want[3] if tb else None,
               t["ln"].cpu().numpy().view(np.uint32) if tb else None)
        _assert_ragged(got, (want[0], want[1], want[4], _rows_of(want, n) if tb else None), ("device", affine, tb), tb)
        assert np.any(want[0] != 0)


def test_cpp_overloads_on_a_mixed_batch(gpu, loracle, aoracle, tmp_path):
    """tests/native/compat_sgfull_ragged.cpp, built with plain g++ against the library: 40 mixed alignments in pieces of 16,
    (0, 5), (5, 0) and (700, 2049) among them, linear and affine; it prints score, path length, end cell and a path checksum,
    which the restatements confirm."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    rng = np.random.default_rng(61)
    shapes = [(int(x), int(y)) for x, y in rng.integers(0, 1300, (36, 2))] + [(0, 5), (5, 0), (700, 2049, "copy"), (1, 1)]
    a, b, _ = _inputs(shapes, 62)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(len(a)).tobytes())
        for x, y in zip(a, b):
            fh.write(np.int32([len(x), len(y)]).tobytes() + x.tobytes() + y.tobytes())
    exe = str(tmp_path / "compat_sgfull_ragged")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_sgfull_ragged.cpp"), "-o", exe, "-L", lib, "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
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
    assert len(rows) == 2 * len(a)
    sm = match_matrix(2, -3)
    at = 0
    for fn in (lambda x, y: loracle.align(x, y, sm, 2), lambda x, y: aoracle.align(x, y, sm, 5, 1)):
        sc, ends, lengths, mrows = _by_shape(a, b, fn)
        for k in range(len(a)):
            path = gpu.semiglobal_expand_moves(mrows[k], lengths[k]) if lengths[k] > 1 else np.zeros((1, 2), np.int32)
            assert tuple(path[-1]) == tuple(ends[k]) and tuple(path[0]) == (0, 0)
            assert rows[at + k] == (int(sc[k]), int(lengths[k]), int(ends[k, 0]), int(ends[k, 1]), checksum(path)), (at, k)
        at += len(a)
