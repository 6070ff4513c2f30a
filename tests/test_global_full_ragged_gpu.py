"""The global / fit / overlap aligners on a batch of mixed (len1, len2) (swmi_global_full_ragged*,
swmi_global_full_affine_ragged*) on the GPU.  Every comparison is exact integer equality: every field equal to the
fixed-length entry called per shape and to the C restatements tests/native/global_full_oracle.c /
global_full_affine_oracle.c grouped by shape, under all 16 masks, at the wave-count edges in len2 (1024 columns per wave, 16
per lane) and the chunk (32 steps) and staging (128 rows) edges in len1; the zero lengths against the restatements called
with length 0 and against the closed form of include/swmi.h; wave counts 1, 2 and 16 side by side; permutations; a host call
of two slices; the device entries on two streams; the C++ overloads."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from global_full_affine_support import GlobalFullAffineOracle
from global_full_support import ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullOracle
from local_support import random_matrix

pytestmark = pytest.mark.gpu

LEN1S = [1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [1, 15, 16, 17, 1023, 1024, 1025, 2049]
EXTRA = [(16384, 3), (5, 16384)]
ZERO_SHAPES = [(0, 0), (0, 1), (1, 0), (0, 33), (33, 0), (0, 1025), (16384, 0), (0, 16384)]
UP_WORD, LEFT_WORD = np.uint64(0xAAAAAAAAAAAAAAAA), np.uint64(0x5555555555555555)


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return GlobalFullOracle(tmp_path_factory.mktemp("global_ragged_oracle"))


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return GlobalFullAffineOracle(tmp_path_factory.mktemp("global_ragged_affine_oracle"))


def _inputs(shapes, seed):
    """Pairs of the given (len1, len2), built the way global_full_support.inputs builds them: random; every third seq2 ends in
    a 90 % copy of (the end of) its seq1 with a 5-base indel, so that a global path runs through every wavefront and holds
    all three kinds of move; every seventh pair a homopolymer against a mostly equal one (ties); every sixth from the fifth a
    seq1 whose first base seq2 lacks (an up move however few rows the table has)."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for k, (len1, len2) in enumerate(shapes):
        x = rng.integers(0, 4, len1, dtype=np.uint8)
        y = rng.integers(0, 4, len2, dtype=np.uint8)
        w = min(len1, len2)
        if k % 3 == 0 and w:
            src = np.where(rng.random(w) < 0.9, x[len1 - w:], rng.integers(0, 4, w)).astype(np.uint8)
            if w > 8:
                cut = int(rng.integers(1, w - 1))
                src = np.concatenate([src[:cut], src[cut + min(5, w - cut - 1):], rng.integers(0, 4, min(5, w - cut - 1), dtype=np.uint8)])
            y[len2 - w:] = src[:w]
        elif k % 7 == 1:
            x[:] = k & 3
            y[rng.random(len2) < 0.8] = k & 3
        elif k % 6 == 4 and len1 >= 3 and len2:
            x[x == 3] = 0
            y[y == 3] = 0
            x[0] = 3
            w = min(len1 - 1, len2)
            y[:w] = x[1:1 + w]
        a.append(x)
        b.append(y)
    return a, b


def _closed_form(len1, len2, mask, cost, traceback=True):
    """include/swmi.h's table for an alignment with a zero length: (score, ends, steps, move word)."""
    up = len2 == 0
    L = len1 + len2
    begin, end = (BEGIN1, END1) if up else (BEGIN2, END2)
    score, ends, steps = 0, [0, 0, 0, 0], 0
    if L and not mask & end:
        ends[:2] = [len1, len2]
        if mask & begin:
            ends[2:] = [len1, len2]
        else:
            score, steps = -cost(L), L
    if not traceback:
        ends[2:] = [-1, -1]
    return score, ends, steps, UP_WORD if up else LEFT_WORD


def _linear_cost(gap):
    return lambda L: L * gap


def _affine_cost(gap_open, gap_extend):
    return lambda L: gap_open + (L - 1) * gap_extend


def _by_shape(a, b, fn, traceback=True, zero=None):
    """What a fixed-length aligner `fn(seq1s[m, len1], seq2s[m, len2])` gives, alignment by alignment, run once per distinct
    shape: (scores, ends, steps, list of move rows).  A shape with a zero length goes to `fn` as well (the restatements take
    length 0) unless `zero(len1, len2)`, a closed form, is given (the fixed-length GPU entries take none)."""
    n = len(a)
    sc = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    steps = np.zeros(n, np.uint32)
    rows = [np.zeros(0, np.uint64)] * n
    groups = {}
    for k in range(n):
        groups.setdefault((len(a[k]), len(b[k])), []).append(k)
    for (len1, len2), idx in groups.items():
        if zero is not None and (len1 == 0 or len2 == 0):
            score, e, st, word = zero(len1, len2)
            sc[idx], ends[idx], steps[idx] = score, e, st
            for k in idx:
                rows[k] = np.full((st + 31) // 32, word, np.uint64)
            continue
        r = fn(np.stack([a[k] for k in idx]).reshape(len(idx), len1), np.stack([b[k] for k in idx]).reshape(len(idx), len2))
        sc[idx], ends[idx] = r[0], r[1]
        if traceback:
            steps[idx] = r[3]
            for x, k in enumerate(idx):
                rows[k] = r[2][x]
    return sc, ends, steps, rows


def _assert_ragged(got, want, what, traceback=True):
    sc, ends, moves, mo, steps = got
    wsc, wends, wsteps, wrows = want
    assert np.array_equal(sc, wsc), (what, np.flatnonzero(sc != wsc)[:8])
    assert np.array_equal(ends, wends), (what, np.flatnonzero((ends != wends).any(axis=1))[:8])
    if not traceback:
        assert moves is None and steps is None
        return
    assert np.array_equal(steps, wsteps), (what, np.flatnonzero(steps != wsteps)[:8])
    for k in range(len(sc)):
        full, part = divmod(int(steps[k]), 32)
        at = int(mo[k])
        assert np.array_equal(moves[at:at + full], wrows[k][:full]), (what, k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (moves[at + full] & mask) == (wrows[k][full] & mask), (what, k)


def _rows_of(result, n):
    return [result[2][int(result[3][k]):int(result[3][k + 1])] for k in range(n)]


@pytest.fixture(scope="module")
def mixed():
    shapes = [(x, y) for x in LEN1S for y in LEN2S for _ in range(2)] + EXTRA
    np.random.default_rng(3).shuffle(shapes)
    return _inputs([tuple(s) for s in shapes], 7)


@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("mask", ALL_MASKS)
def test_edges_equal_the_fixed_entries_and_the_restatements(gpu, loracle, aoracle, mixed, mask, traceback):
    """One shuffled batch of two pairs of every (len1, len2) of the edges plus 16384 on either side, under one mask: field by
    field the fixed-length entry called once per distinct shape and the C restatements grouped by shape, for linear
    (2, -3, 2) and a random matrix at gap 6 and for affine (5, 1) and (1, 4); open == extend equals the linear call."""
    a, b = mixed
    gr = gpu.global_ragged
    assert len(a) == 2 * len(LEN1S) * len(LEN2S) + 2
    linear = {}
    for sm, gap in ((match_matrix(2, -3), 2), (random_matrix(), 6)):
        got = gr.global_full_ragged(a, b, sm, gap, mask, traceback=traceback)
        linear[gap] = (sm, got)
        _assert_ragged(got, _by_shape(a, b, lambda x, y: gpu.global_full(x, y, sm, gap, mask, traceback=traceback), traceback),
                       ("linear", gap, mask), traceback)
        if traceback:
            _assert_ragged(got, _by_shape(a, b, lambda x, y: loracle.align(x, y, sm, gap, mask)), ("linear restatement", gap, mask))
    for sm, (go, ge) in ((match_matrix(2, -3), (5, 1)), (random_matrix(), (1, 4))):
        got = gr.global_full_affine_ragged(a, b, sm, go, ge, mask, traceback=traceback)
        want = _by_shape(a, b, lambda x, y: gpu.global_affine.global_full_affine(x, y, sm, go, ge, mask, traceback=traceback), traceback)
        _assert_ragged(got, want, ("affine", go, ge, mask), traceback)
        if traceback:
            _assert_ragged(got, _by_shape(a, b, lambda x, y: aoracle.align(x, y, sm, go, ge, mask)), ("affine restatement", go, ge, mask))
    for gap, (sm, lin) in linear.items():
        eq = gr.global_full_affine_ragged(a, b, sm, gap, gap, mask, traceback=traceback)
        _assert_ragged(eq, (lin[0], lin[1], lin[4], _rows_of(lin, len(a)) if traceback else None), ("open = extend", gap, mask), traceback)


@pytest.fixture(scope="module")
def with_zeros():
    shapes = ZERO_SHAPES + [(5, 7), (40, 1030), (3, 3), (1, 1)] + ZERO_SHAPES[1:4]
    np.random.default_rng(5).shuffle(shapes)
    return _inputs([tuple(s) for s in shapes], 9)


@pytest.mark.parametrize("mask", ALL_MASKS)
def test_zero_lengths(gpu, loracle, aoracle, with_zeros, mask):
    """The zero lengths, mixed with non-empty alignments, under one mask: every field equal to the restatements called directly
    with length 0 and to the closed form of include/swmi.h (score 0 at (0, 0) with a free end; else the far corner, with
    score 0 and no step if that border's begin is free, else -cost(L) and L forced steps of one code); whole words of that
    code where L = 16384; ends-only the same score and end cell with start (-1, -1).  A kernel with the local aligners' arm
    gives score 0 where -cost(L) is due."""
    a, b = with_zeros
    gr = gpu.global_ragged
    sm = match_matrix(2, -3)
    n = len(a)
    zero = [k for k in range(n) if len(a[k]) == 0 or len(b[k]) == 0]
    assert len(zero) == len(ZERO_SHAPES) + 3
    cases = [("linear", (gap,), _linear_cost(gap)) for gap in (3, 0)]
    cases += [("affine", (go, ge), _affine_cost(go, ge)) for go, ge in ((5, 1), (0, 2), (4, 4))]
    for kind, gaps, cost in cases:
        run = gr.global_full_ragged if kind == "linear" else gr.global_full_affine_ragged
        oracle = loracle if kind == "linear" else aoracle
        got = run(a, b, sm, *gaps, mask)
        _assert_ragged(got, _by_shape(a, b, lambda x, y: oracle.align(x, y, sm, *gaps, mask)), (kind, gaps, mask, "restatement"))
        fixed = gpu.global_full if kind == "linear" else gpu.global_affine.global_full_affine
        _assert_ragged(got, _by_shape(a, b, lambda x, y: fixed(x, y, sm, *gaps, mask), zero=lambda p, q: _closed_form(p, q, mask, cost)),
                       (kind, gaps, mask, "closed form"))
        sc, ends, moves, mo, steps = got
        for k in zero:
            len1, len2 = len(a[k]), len(b[k])
            score, e, st, word = _closed_form(len1, len2, mask, cost)
            assert (int(sc[k]), list(ends[k]), int(steps[k])) == (score, e, st), (kind, gaps, mask, len1, len2)
            if st == 16384:                             # whole words of one code
                assert np.all(moves[int(mo[k]):int(mo[k]) + 512] == word), (kind, gaps, mask, len1, len2)
        if not mask & (END1 | BEGIN1):
            assert any(int(sc[k]) == -cost(16384) and len(b[k]) == 0 for k in zero)     # what a score of 0 would miss
        eo = run(a, b, sm, *gaps, mask, traceback=False)
        assert eo[2] is None and eo[3] is None and eo[4] is None
        assert np.array_equal(eo[0], sc) and np.array_equal(eo[1][:, :2], ends[:, :2]) and np.all(eo[1][:, 2:] == -1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_extremes_side_by_side(gpu, loracle, aoracle, n):
    """Wave counts 1, 2 and 16 in one slice and rows 1 .. 16384 in adjacent workgroups, against the restatements."""
    cycle = [(1, 16384), (16384, 1), (33, 16384), (16384, 17), (2, 1025)]
    a, b = _inputs([cycle[k % 5] for k in range(n)], 50 + n)
    sm = match_matrix(2, -3)
    gr = gpu.global_ragged
    for mask in (GLOBAL, FIT, OVERLAP):
        _assert_ragged(gr.global_full_ragged(a, b, sm, 2, mask), _by_shape(a, b, lambda x, y: loracle.align(x, y, sm, 2, mask)), (n, mask))
        _assert_ragged(gr.global_full_affine_ragged(a, b, sm, 5, 1, mask),
                       _by_shape(a, b, lambda x, y: aoracle.align(x, y, sm, 5, 1, mask)), (n, mask, "affine"))


def test_permuting_a_batch_permutes_its_results(gpu):
    rng = np.random.default_rng(11)
    a, b = _inputs([(int(x), int(y)) for x, y in rng.integers(0, 1501, (300, 2))], 12)
    perm = rng.permutation(len(a))
    sm = match_matrix(2, -3)        # every third seq2 ends in a copy of its seq1's end: a long overlap with a positive score
    gr = gpu.global_ragged
    for run in (lambda x, y: gr.global_full_ragged(x, y, sm, 3, OVERLAP), lambda x, y: gr.global_full_affine_ragged(x, y, sm, 6, 2, OVERLAP)):
        sc, ends, moves, mo, steps = run(a, b)
        assert sc.max() > 0 and steps.max() > 32
        psc, pends, pmoves, pmo, psteps = run([a[k] for k in perm], [b[k] for k in perm])
        assert np.array_equal(psc, sc[perm]) and np.array_equal(pends, ends[perm]) and np.array_equal(psteps, steps[perm])
        for x, k in enumerate(perm):
            w = int(steps[k]) // 32
            assert np.array_equal(pmoves[int(pmo[x]):int(pmo[x]) + w], moves[int(mo[k]):int(mo[k]) + w])


def _tiny_tables(cat1, off1, cat2, off2, match, mismatch, gap, mask):
    """(scores, end cells) of n tables of at most 5 x 5 cells (lengths 0 .. 4), vectorised over the alignments: the borders by
    the mask, the 16 inner cells in a closed loop, then the end rule over the 25 cells in row-major order (the first largest
    H among the cells the mask allows)."""
    n = len(off1) - 1
    len1 = (off1[1:] - off1[:-1]).astype(np.int64)
    len2 = (off2[1:] - off2[:-1]).astype(np.int64)
    pad1 = np.concatenate([cat1, np.zeros(8, np.uint8)])
    pad2 = np.concatenate([cat2, np.zeros(8, np.uint8)])
    H = np.zeros((n, 5, 5), np.int64)
    for x in range(1, 5):
        H[:, x, 0] = 0 if mask & BEGIN1 else -x * gap
        H[:, 0, x] = 0 if mask & BEGIN2 else -x * gap
    for i in range(1, 5):
        for j in range(1, 5):
            x = pad1[off1[:-1].astype(np.int64) + i - 1] & 3
            y = pad2[off2[:-1].astype(np.int64) + j - 1] & 3
            H[:, i, j] = np.maximum(H[:, i - 1, j - 1] + np.where(x == y, match, mismatch), np.maximum(H[:, i - 1, j], H[:, i, j - 1]) - gap)
    best = np.full(n, np.iinfo(np.int64).min)
    end = np.zeros((n, 2), np.int64)
    for i in range(5):
        for j in range(5):
            allowed = (i == len1) & (j == len2)
            if mask & END1:
                allowed |= (j == len2) & (i <= len1)
            if mask & END2:
                allowed |= (i == len1) & (j <= len2)
            better = allowed & (H[:, i, j] > best)
            best = np.where(better, H[:, i, j], best)
            end[better] = (i, j)
    return best.astype(np.int32), end.astype(np.int32)


def test_host_call_of_two_slices(gpu):
    """2^20 + 5 alignments with lengths in [0, 4], ends-only: two slices by the count cap.  (The budget-driven traceback split
    runs on the fake GPU, tests/test_global_full_ragged_host_fake.py.)"""
    rng = np.random.default_rng(21)
    n = (1 << 20) + 5
    off1 = np.zeros(n + 1, np.uint64)
    off2 = np.zeros(n + 1, np.uint64)
    off1[1:] = np.cumsum(rng.integers(0, 5, n))
    off2[1:] = np.cumsum(rng.integers(0, 5, n))
    cat1 = rng.integers(0, 3, int(off1[-1]), dtype=np.uint8)
    cat2 = rng.integers(0, 3, int(off2[-1]), dtype=np.uint8)
    assert len(gpu.global_ragged.global_full_ragged_slices_for(off1, off2, affine=False, traceback=False)) >= 2
    for mask in (GLOBAL, OVERLAP):
        want_sc, want_end = _tiny_tables(cat1, off1, cat2, off2, 3, -2, 1, mask)
        assert want_sc.max() == 12 and (want_sc.min() < 0 if mask == GLOBAL else want_sc.min() == 0)
        sc, ends, moves, mo, steps = gpu.global_ragged.global_full_ragged((cat1, off1), (cat2, off2), match_matrix(3, -2), 1, mask,
                                                                          traceback=False)
        assert moves is None and mo is None and steps is None
        assert np.array_equal(sc, want_sc), mask
        assert np.array_equal(ends[:, :2], want_end) and np.all(ends[:, 2:] == -1), mask


def test_device_entries_on_two_streams_in_flight(gpu):
    """Both device entries on torch buffers, four calls (linear and affine, with and without traceback) on two streams issued
    before any is waited for, equal the host entry."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    sm = random_matrix(5)
    gr = gpu.global_ragged
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    for x, (affine, tb, n, seed, mask) in enumerate(((False, True, 257, 1, FIT), (True, True, 130, 2, OVERLAP), (False, False, 300, 3, GLOBAL),
                                                     (True, False, 190, 4, FIT))):
        a, b = _inputs([(int(p), int(q)) for p, q in rng.integers(0, 1101, (n, 2))], seed)
        cat1, off1, cat2, off2 = gpu._ragged_pair(a, b)
        mo = gpu.local_full_ragged_move_offsets(off1, off2)
        pad = np.zeros(16, np.uint8)
        t = dict(a=torch.from_numpy(np.concatenate([cat1, pad])).to(dev), b=torch.from_numpy(np.concatenate([cat2, pad])).to(dev),
                 sc=torch.zeros(n, dtype=torch.int32, device=dev), ends=torch.zeros((n, 4), dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]), dtype=torch.int64, device=dev), st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((affine, tb, mask, a, b, off1, off2, t, streams[x % 2]))
    torch.cuda.synchronize()
    for affine, tb, mask, a, b, off1, off2, t, s in jobs:
        args = (t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm)
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None)
        if affine:
            gr.global_full_affine_ragged_device(*args, 7, 1, mask, *bufs, stream=s.cuda_stream)
        else:
            gr.global_full_ragged_device(*args, 4, mask, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for affine, tb, mask, a, b, off1, off2, t, s in jobs:
        want = gr.global_full_affine_ragged(a, b, sm, 7, 1, mask, traceback=tb) if affine else gr.global_full_ragged(a, b, sm, 4, mask, traceback=tb)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64) if tb else None, want[3],
               t["st"].cpu().numpy().view(np.uint32) if tb else None)
        _assert_ragged(got, (want[0], want[1], want[4], _rows_of(want, len(a)) if tb else None), ("device", affine, tb), tb)
        assert np.any(want[0] != 0)


def test_cpp_overloads_on_a_mixed_batch(gpu, loracle, aoracle, tmp_path):
    """tests/native/compat_global_full_ragged.cpp, built against the library: 40 mixed alignments in pieces of 16, (0, 5),
    (5, 0) and (700, 2049) among them, under GLOBAL and FIT, linear and affine; it prints score, path length, start cell, end
    cell and a path checksum, which the restatements confirm."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    rng = np.random.default_rng(61)
    shapes = [(int(x), int(y)) for x, y in rng.integers(0, 1300, (36, 2))] + [(0, 5), (5, 0), (700, 2049), (1, 1)]
    a, b = _inputs(shapes, 62)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(len(a)).tobytes())
        for x, y in zip(a, b):
            fh.write(np.int32([len(x), len(y)]).tobytes() + x.tobytes() + y.tobytes())
    exe = str(tmp_path / "compat_global_full_ragged")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_full_ragged.cpp"), "-o", exe, "-L", lib, "-lswmi",
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
    assert len(rows) == 4 * len(a)
    sm = match_matrix(2, -3)
    at = 0
    for fn in (lambda x, y, m: loracle.align(x, y, sm, 2, m), lambda x, y, m: aoracle.align(x, y, sm, 5, 1, m)):
        for mask in (GLOBAL, FIT):
            sc, ends, steps, mrows = _by_shape(a, b, lambda x, y: fn(x, y, mask))
            for k in range(len(a)):
                path = gpu.local_full_expand_moves(mrows[k], steps[k], ends[k, 0], ends[k, 1]) if steps[k] else ends[k, 2:].reshape(1, 2)
                assert rows[at + k] == (int(sc[k]), int(steps[k]) + 1, int(ends[k, 2]), int(ends[k, 3]), int(ends[k, 0]), int(ends[k, 1]),
                                        checksum(path)), (at, k)
            at += len(a)
