"""The any-length local aligners on a batch of mixed (len1, len2) (swmi_local_full_ragged*, swmi_local_full_affine_ragged*)
on the GPU: fixture F7, the reference's own SmithWaterman_111_long results, in one call; every field equal to the fixed-length
entry called per shape and to the C restatements tests/native/local_full_oracle.c / local_full_affine_oracle.c grouped by
shape, at the wave-count edges in len2 (1024 columns per wave, 16 per lane), the chunk (32 steps) and staging (128 rows)
edges in len1 and with several wave counts in one slice; wave counts 1, 2 and 16 side by side; permutations; a host call of
two slices; the device entries on two streams; the C++ overloads."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS
from local_full_affine_support import LocalFullAffineOracle
from local_full_support import LocalFullOracle
from local_support import PARAMS, load_f7, random_matrix

pytestmark = pytest.mark.gpu

LEN1S = [1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [1, 15, 16, 17, 1023, 1024, 1025, 2049]
EXTRA = [(16384, 3), (5, 16384), (0, 7), (7, 0), (0, 0)]


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalFullOracle(tmp_path_factory.mktemp("full_ragged_oracle"))


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return LocalFullAffineOracle(tmp_path_factory.mktemp("full_ragged_affine_oracle"))


def _inputs(shapes, seed):
    """Pairs of the given (len1, len2), built the way local_full_support.inputs builds them: random, every third seq2 a 90 %
    copy of its seq1 with a 5-base indel (long diagonal paths), every seventh pair a homopolymer (ties)."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for k, (len1, len2) in enumerate(shapes):
        x = rng.integers(0, 4, len1, dtype=np.uint8)
        y = rng.integers(0, 4, len2, dtype=np.uint8)
        w = min(len1, len2)
        if k % 3 == 0 and w:
            src = np.where(rng.random(w) < 0.9, x[:w], rng.integers(0, 4, w)).astype(np.uint8)
            if w > 8:
                cut = int(rng.integers(1, w - 1))
                src = np.concatenate([src[:cut], src[cut + min(5, w - cut - 1):], rng.integers(0, 4, min(5, w - cut - 1), dtype=np.uint8)])
            y[:w] = src[:w]
        elif k % 7 == 1:
            x[:] = k & 3
            y[rng.random(len2) < 0.8] = k & 3
        a.append(x)
        b.append(y)
    return a, b


def _by_shape(a, b, fn, traceback=True):
    """What a fixed-length aligner `fn(seq1s[m, len1], seq2s[m, len2])` gives, alignment by alignment, run once per distinct
    shape: (scores, ends, steps, list of move rows).  A shape with a zero length is the stated result."""
    n = len(a)
    sc = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    steps = np.zeros(n, np.uint32)
    rows = [np.zeros(0, np.uint64)] * n
    groups = {}
    for k in range(n):
        groups.setdefault((len(a[k]), len(b[k])), []).append(k)
    for (len1, len2), idx in groups.items():
        if len1 == 0 or len2 == 0:
            ends[idx] = (0, 0, 0, 0) if traceback else (0, 0, -1, -1)
            continue
        r = fn(np.stack([a[k] for k in idx]), np.stack([b[k] for k in idx]))
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


def test_f7_in_one_call_linear_and_affine(gpu):
    """The whole of F7 (252 alignments of 11 seq1 lengths against 128-mers) in ONE call at (1, -1, 1), linear and affine at
    open = extend = 1: scores, end cells, start cells and the reference's recorded paths, zero mismatches."""
    f7 = load_f7()
    a = [v["seq1"] for v in f7]
    b = [v["seq2"] for v in f7]
    assert len(f7) == 252 and len({len(x) for x in a}) == 11
    for name, run in (("linear", lambda: gpu.local_full_ragged(a, b, match_matrix(1, -1), 1)),
                      ("affine", lambda: gpu.local_full_affine_ragged(a, b, match_matrix(1, -1), 1, 1))):
        sc, ends, moves, mo, steps = run()
        bad = 0
        for k, v in enumerate(f7):
            p = v["path"]
            ok = int(sc[k]) == v["score"] and tuple(ends[k, :2]) == tuple(p[-1]) and tuple(ends[k, 2:]) == tuple(p[0])
            row = moves[int(mo[k]):int(mo[k + 1])]
            ok = ok and np.array_equal(gpu.local_full_expand_moves(row, steps[k], ends[k, 0], ends[k, 1]), p)
            bad += 0 if ok else 1
        assert bad == 0, name


@pytest.fixture(scope="module")
def mixed():
    shapes = [(x, y) for x in LEN1S for y in LEN2S for _ in range(2)] + EXTRA
    np.random.default_rng(3).shuffle(shapes)
    return _inputs([tuple(s) for s in shapes], 7)


@pytest.mark.parametrize("traceback", [True, False])
def test_mixed_shapes_equal_the_fixed_entries_and_the_restatements(gpu, loracle, aoracle, mixed, traceback):
    """One shuffled batch of every (len1, len2) of the edges, 16384 on either side and the zero lengths, per parameter set:
    field by field the fixed-length entry called once per distinct shape, and the C restatements grouped by shape."""
    a, b = mixed
    zero = [k for k in range(len(a)) if len(a[k]) == 0 or len(b[k]) == 0]
    assert len(zero) == 3
    mats = [match_matrix(m, x) for m, x, _ in PARAMS] + [random_matrix()]
    gaps = [g for _, _, g in PARAMS] + [6]
    linear = {}
    for sm, gap in zip(mats, gaps):
        got = gpu.local_full_ragged(a, b, sm, gap, traceback=traceback)
        linear[gap] = got
        _assert_ragged(got, _by_shape(a, b, lambda x, y: gpu.local_full(x, y, sm, gap, traceback=traceback), traceback),
                       ("linear", gap), traceback)
        if traceback:
            _assert_ragged(got, _by_shape(a, b, lambda x, y: loracle.align(x, y, sm, gap)), ("linear restatement", gap))
            assert not got[0][zero].any() and not got[1][zero].any() and not got[4][zero].any()
        else:
            assert not got[0][zero].any() and np.all(got[1][zero] == (0, 0, -1, -1))
    for g, (go, ge) in enumerate(AFFINE_GAPS):
        sm = mats[g % len(mats)]
        got = gpu.local_full_affine_ragged(a, b, sm, go, ge, traceback=traceback)
        _assert_ragged(got, _by_shape(a, b, lambda x, y: gpu.local_full_affine(x, y, sm, go, ge, traceback=traceback), traceback),
                       ("affine", go, ge), traceback)
        if traceback:
            _assert_ragged(got, _by_shape(a, b, lambda x, y: aoracle.align(x, y, sm, go, ge)), ("affine restatement", go, ge))
            assert not got[0][zero].any() and not got[1][zero].any() and not got[4][zero].any()
        else:
            assert not got[0][zero].any() and np.all(got[1][zero] == (0, 0, -1, -1))
    # open = extend: the affine call equals the linear one
    for sm, gap in zip(mats, gaps):
        eq = gpu.local_full_affine_ragged(a, b, sm, gap, gap, traceback=traceback)
        lin = linear[gap]
        rows = [lin[2][int(lin[3][k]):int(lin[3][k + 1])] for k in range(len(a))] if traceback else None
        _assert_ragged(eq, (lin[0], lin[1], lin[4], rows), ("open = extend", gap), traceback)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_extremes_side_by_side(gpu, loracle, aoracle, n):
    """Wave counts 1, 2 and 16 in one slice and rows 1 .. 16384 in adjacent workgroups, against the restatements."""
    cycle = [(1, 16384), (16384, 1), (33, 16384), (16384, 17), (2, 1025)]
    a, b = _inputs([cycle[k % 5] for k in range(n)], 50 + n)
    sm = match_matrix(2, -3)
    _assert_ragged(gpu.local_full_ragged(a, b, sm, 2), _by_shape(a, b, lambda x, y: loracle.align(x, y, sm, 2)), n)
    _assert_ragged(gpu.local_full_affine_ragged(a, b, sm, 5, 1), _by_shape(a, b, lambda x, y: aoracle.align(x, y, sm, 5, 1)), n)


def test_permuting_a_batch_permutes_its_results(gpu):
    rng = np.random.default_rng(11)
    a, b = _inputs([(int(x), int(y)) for x, y in rng.integers(0, 1501, (300, 2))], 12)
    perm = rng.permutation(len(a))
    sm = random_matrix(4)
    for run in (lambda x, y: gpu.local_full_ragged(x, y, sm, 3), lambda x, y: gpu.local_full_affine_ragged(x, y, sm, 6, 2)):
        sc, ends, moves, mo, steps = run(a, b)
        assert sc.max() > 0 and steps.max() > 32
        psc, pends, pmoves, pmo, psteps = run([a[k] for k in perm], [b[k] for k in perm])
        assert np.array_equal(psc, sc[perm]) and np.array_equal(pends, ends[perm]) and np.array_equal(psteps, steps[perm])
        for x, k in enumerate(perm):
            w = int(steps[k]) // 32
            assert np.array_equal(pmoves[int(pmo[x]):int(pmo[x]) + w], moves[int(mo[k]):int(mo[k]) + w])


def _tiny_tables(cat1, off1, cat2, off2, match, mismatch, gap):
    """(scores, end cells) of n tables of at most 4 x 4, vectorised over the alignments: a closed loop over the 16 cells."""
    n = len(off1) - 1
    len1 = (off1[1:] - off1[:-1]).astype(np.int64)
    len2 = (off2[1:] - off2[:-1]).astype(np.int64)
    pad1 = np.concatenate([cat1, np.zeros(8, np.uint8)])
    pad2 = np.concatenate([cat2, np.zeros(8, np.uint8)])
    H = np.zeros((n, 5, 5), np.int64)
    best = np.zeros(n, np.int64)
    end = np.zeros((n, 2), np.int64)
    for i in range(1, 5):
        for j in range(1, 5):
            x = pad1[off1[:-1].astype(np.int64) + i - 1] & 3
            y = pad2[off2[:-1].astype(np.int64) + j - 1] & 3
            h = np.maximum(np.maximum(0, H[:, i - 1, j - 1] + np.where(x == y, match, mismatch)),
                           np.maximum(H[:, i - 1, j], H[:, i, j - 1]) - gap)
            h = np.where((i <= len1) & (j <= len2), h, 0)
            H[:, i, j] = h
            better = h > best                           # row-major order: the first cell holding the maximum
            best = np.where(better, h, best)
            end[better] = (i, j)
    return best.astype(np.int32), end.astype(np.int32)


def test_host_call_of_two_slices(gpu):
    """2^20 + 5 alignments with lengths in [0, 4], ends-only: two slices by the count cap.  (The budget-driven traceback split
    runs on the fake GPU, tests/test_local_full_ragged_host_fake.py.)"""
    rng = np.random.default_rng(21)
    n = (1 << 20) + 5
    off1 = np.zeros(n + 1, np.uint64)
    off2 = np.zeros(n + 1, np.uint64)
    off1[1:] = np.cumsum(rng.integers(0, 5, n))
    off2[1:] = np.cumsum(rng.integers(0, 5, n))
    cat1 = rng.integers(0, 3, int(off1[-1]), dtype=np.uint8)
    cat2 = rng.integers(0, 3, int(off2[-1]), dtype=np.uint8)
    assert len(gpu.local_full_ragged_slices_for(off1, off2, affine=False, traceback=False)) >= 2
    want_sc, want_end = _tiny_tables(cat1, off1, cat2, off2, 3, -2, 1)
    assert want_sc.max() == 12 and (want_sc == 0).any()
    sc, ends, moves, mo, steps = gpu.local_full_ragged((cat1, off1), (cat2, off2), match_matrix(3, -2), 1, traceback=False)
    assert moves is None and mo is None and steps is None
    assert np.array_equal(sc, want_sc)
    assert np.array_equal(ends[:, :2], want_end) and np.all(ends[:, 2:] == -1)


def test_device_entries_on_two_streams_in_flight(gpu):
    """Both device entries on torch buffers, four calls (linear and affine, with and without traceback) on two streams issued
    before any is waited for, equal the host entry."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    sm = random_matrix(5)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    for x, (affine, tb, n, seed) in enumerate(((False, True, 257, 1), (True, True, 130, 2), (False, False, 300, 3), (True, False, 190, 4))):
        a, b = _inputs([(int(p), int(q)) for p, q in rng.integers(0, 1101, (n, 2))], seed)
        cat1, off1, cat2, off2 = gpu._ragged_pair(a, b)
        mo = gpu.local_full_ragged_move_offsets(off1, off2)
        pad = np.zeros(16, np.uint8)
        t = dict(a=torch.from_numpy(np.concatenate([cat1, pad])).to(dev), b=torch.from_numpy(np.concatenate([cat2, pad])).to(dev),
                 sc=torch.zeros(n, dtype=torch.int32, device=dev), ends=torch.zeros((n, 4), dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]), dtype=torch.int64, device=dev), st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((affine, tb, a, b, off1, off2, t, streams[x % 2]))
    torch.cuda.synchronize()
    for affine, tb, a, b, off1, off2, t, s in jobs:
        args = (t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm)
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None)
        if affine:
            gpu.local_full_affine_ragged_device(*args, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            gpu.local_full_ragged_device(*args, 4, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for affine, tb, a, b, off1, off2, t, s in jobs:
        want = gpu.local_full_affine_ragged(a, b, sm, 7, 1, traceback=tb) if affine else gpu.local_full_ragged(a, b, sm, 4, traceback=tb)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64) if tb else None, want[3],
               t["st"].cpu().numpy().view(np.uint32) if tb else None)
        rows = [want[2][int(want[3][k]):int(want[3][k + 1])] for k in range(len(a))] if tb else None
        _assert_ragged(got, (want[0], want[1], want[4], rows), ("device", affine, tb), tb)
        assert want[0].max() > 0


def test_cpp_overloads_reproduce_f7_and_a_mixed_batch(gpu, loracle, aoracle, tmp_path):
    """tests/native/compat_local_full_ragged.cpp, built against the library: F7 in one call of each overload, and a mixed batch
    of 40 alignments in pieces of 16 whose results it prints for the restatements to check."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    f7 = load_f7()
    rng = np.random.default_rng(61)
    shapes = [(int(x), int(y)) for x, y in rng.integers(0, 1300, (36, 2))] + [(0, 5), (5, 0), (700, 2049), (1, 1)]
    a, b = _inputs(shapes, 62)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(len(f7)).tobytes())
        for v in f7:
            fh.write(np.int32([len(v["seq1"]), len(v["seq2"])]).tobytes() + v["seq1"].tobytes() + v["seq2"].tobytes())
        fh.write(np.int32(len(a)).tobytes())
        for x, y in zip(a, b):
            fh.write(np.int32([len(x), len(y)]).tobytes() + x.tobytes() + y.tobytes())
    exe = str(tmp_path / "compat_local_full_ragged")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local_full_ragged.cpp"), "-o", exe, "-L", lib, "-lswmi",
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
    assert len(rows) == 2 * len(f7) + 2 * len(a)
    for which in range(2):                                  # linear, then affine at open = extend = 1
        for k, v in enumerate(f7):
            p = v["path"]
            assert rows[which * len(f7) + k] == (v["score"], len(p), int(p[0][0]), int(p[0][1]), int(p[-1][0]), int(p[-1][1]),
                                                 checksum(p)), (which, k)
    sm = match_matrix(2, -3)
    for which, fn in enumerate((lambda x, y: loracle.align(x, y, sm, 2), lambda x, y: aoracle.align(x, y, sm, 5, 1))):
        sc, ends, steps, mrows = _by_shape(a, b, fn)
        for k in range(len(a)):
            path = gpu.local_full_expand_moves(mrows[k], steps[k], ends[k, 0], ends[k, 1]) if steps[k] else ends[k, 2:].reshape(1, 2)
            assert rows[2 * len(f7) + which * len(a) + k] == (int(sc[k]), int(steps[k]) + 1, int(ends[k, 2]), int(ends[k, 3]),
                                                              int(ends[k, 0]), int(ends[k, 1]), checksum(path)), (which, k)
