"""The local aligners on a batch of mixed seq1 lengths (swmi_local_align_ragged*, swmi_local_align_affine_ragged*) on the GPU:
fixture F7, the reference's own SmithWaterman_111_long results, in one call; every field equal to the fixed-length entry
called per length and to the C restatements tests/native/local_oracle.c / local_affine_oracle.c grouped by length; lengths
0 .. 16384 side by side in one wavefront; permutations; several slices; the device entry on two streams; a fuzz."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle
from local_support import PARAMS, LocalOracle, load_f7, random_matrix

pytestmark = pytest.mark.gpu

MIX = [0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 1000, 16384]


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("ragged_local_oracle"))


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("ragged_affine_oracle"))


def _inputs(lens, seed):
    """seq1s of the given lengths (every third a noisy copy of a piece of its seq2, some homopolymers), seq2s (n, 128)"""
    rng = np.random.default_rng(seed)
    n = len(lens)
    b = rng.integers(0, 4, (n, 128), dtype=np.uint8)
    a = []
    for k, L in enumerate(lens):
        s = rng.integers(0, 4, L, dtype=np.uint8)
        if k % 3 == 0 and L:
            w = min(L, 128)
            at = int(rng.integers(0, L - w + 1))
            s[at:at + w] = np.where(rng.random(w) < 0.85, b[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        elif k % 7 == 1:
            s[:] = k & 3
            b[k, rng.random(128) < 0.8] = k & 3
        a.append(s)
    return a, b


def _by_length(a, b, fn, traceback=True):
    """What a fixed-length aligner `fn(seq1s[m, L], seq2s[m, 128])` gives, alignment by alignment, run once per length:
    (scores, ends, steps, list of move rows).  Length 0 is the stated result."""
    n = len(a)
    sc = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    steps = np.zeros(n, np.uint32)
    rows = [np.zeros(0, np.uint64)] * n
    lens = np.array([len(x) for x in a])
    for L in np.unique(lens):
        idx = np.nonzero(lens == L)[0]
        if L == 0:
            ends[idx] = (0, 0, 0, 0) if traceback else (0, 0, -1, -1)
            continue
        r = fn(np.stack([a[k] for k in idx]), b[idx])
        sc[idx], ends[idx] = r[0], r[1]
        if traceback:
            steps[idx] = r[3]
            for x, k in enumerate(idx):
                rows[k] = r[2][x]
    return sc, ends, steps, rows


def _assert_ragged(got, want, what, traceback=True):
    sc, ends, moves, mo, steps = got
    wsc, wends, wsteps, wrows = want
    assert np.array_equal(sc, wsc), what
    assert np.array_equal(ends, wends), what
    if not traceback:
        assert moves is None and steps is None
        return
    assert np.array_equal(steps, wsteps), what
    for k in range(len(sc)):
        words = (int(steps[k]) + 31) // 32
        assert np.array_equal(moves[int(mo[k]):int(mo[k]) + words], wrows[k][:words]), (what, k)


def test_f7_in_one_call_linear_and_affine(gpu):
    """The whole of F7 (252 alignments of 11 lengths) in ONE ragged call at (1, -1, 1), linear and affine at open = extend = 1:
    scores, end cells, start cells and the reference's recorded paths."""
    f7 = load_f7()
    a = [v["seq1"] for v in f7]
    b = np.stack([v["seq2"] for v in f7])
    assert len({len(x) for x in a}) > 1
    for name, run in (("linear", lambda: gpu.local_align_ragged(a, b, match_matrix(1, -1), 1)),
                      ("affine", lambda: gpu.local_align_affine_ragged(a, b, match_matrix(1, -1), 1, 1))):
        sc, ends, moves, mo, steps = run()
        bad = 0
        for k, v in enumerate(f7):
            p = v["path"]
            ok = int(sc[k]) == v["score"] and tuple(ends[k, :2]) == tuple(p[-1]) and tuple(ends[k, 2:]) == tuple(p[0])
            row = moves[int(mo[k]):int(mo[k + 1])]
            ok = ok and np.array_equal(gpu.local_expand_moves(row, steps[k], ends[k, 0], ends[k, 1]), p)
            bad += 0 if ok else 1
        assert bad == 0, name


@pytest.mark.parametrize("traceback", [True, False])
def test_mixed_lengths_equal_the_fixed_entries_and_the_restatements(gpu, loracle, aoracle, traceback):
    """One shuffled batch of lengths 0 .. 16384 per parameter set: field by field the fixed-length entry called per length,
    and the C restatements grouped by length."""
    rng = np.random.default_rng(3)
    lens = [L for L in MIX for _ in range(3 if L == 16384 else 9)]
    rng.shuffle(lens)
    a, b = _inputs(lens, 7)
    mats = [match_matrix(m, x) for m, x, _ in PARAMS] + [random_matrix()]
    gaps = [g for _, _, g in PARAMS] + [6]
    for sm, gap in zip(mats, gaps):
        got = gpu.local_align_ragged(a, b, sm, gap, traceback=traceback)
        _assert_ragged(got, _by_length(a, b, lambda x, y: gpu.local_align(x, y, sm, gap, traceback=traceback), traceback),
                       ("linear", gap), traceback)
        if traceback:
            _assert_ragged(got, _by_length(a, b, lambda x, y: loracle.align(x, y, sm, gap)), ("linear oracle", gap))
    for g, (go, ge) in enumerate(AFFINE_GAPS):
        sm = mats[g % len(mats)]
        got = gpu.local_align_affine_ragged(a, b, sm, go, ge, traceback=traceback)
        _assert_ragged(got, _by_length(a, b, lambda x, y: gpu.local_align_affine(x, y, sm, go, ge, traceback=traceback), traceback),
                       ("affine", go, ge), traceback)
        if traceback:
            _assert_ragged(got, _by_length(a, b, lambda x, y: aoracle.align(x, y, sm, go, ge)), ("affine oracle", go, ge))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 15])
def test_extremes_side_by_side_in_one_wavefront(gpu, loracle, aoracle, n):
    lens = [(1, 16384, 2, 16383)[k % 4] for k in range(n)]
    a, b = _inputs(lens, 50 + n)
    sm = match_matrix(2, -3)
    _assert_ragged(gpu.local_align_ragged(a, b, sm, 2), _by_length(a, b, lambda x, y: loracle.align(x, y, sm, 2)), n)
    _assert_ragged(gpu.local_align_affine_ragged(a, b, sm, 5, 1), _by_length(a, b, lambda x, y: aoracle.align(x, y, sm, 5, 1)), n)


def test_permuting_a_batch_permutes_its_results(gpu):
    rng = np.random.default_rng(11)
    lens = list(rng.integers(0, 700, 333))
    a, b = _inputs(lens, 12)
    perm = rng.permutation(len(a))
    sm = random_matrix(4)
    for run in (lambda x, y: gpu.local_align_ragged(x, y, sm, 3), lambda x, y: gpu.local_align_affine_ragged(x, y, sm, 6, 2)):
        sc, ends, moves, mo, steps = run(a, b)
        psc, pends, pmoves, pmo, psteps = run([a[k] for k in perm], b[perm])
        assert np.array_equal(psc, sc[perm]) and np.array_equal(pends, ends[perm]) and np.array_equal(psteps, steps[perm])
        for x, k in enumerate(perm):
            w = (int(steps[k]) + 31) // 32
            assert np.array_equal(pmoves[int(pmo[x]):int(pmo[x]) + w], moves[int(mo[k]):int(mo[k]) + w])


def test_host_call_of_several_slices(gpu):
    rng = np.random.default_rng(21)
    lens = [16384 if k % 3 == 0 else int(rng.integers(0, 16385)) for k in range(1500)]
    a, b = _inputs(lens, 22)
    _, off = gpu._ragged_seq1s(a)
    assert len(gpu.local_ragged_slices_for(off, affine=False, traceback=True)) >= 3
    sm = match_matrix(1, -1)
    _assert_ragged(gpu.local_align_ragged(a, b, sm, 1), _by_length(a, b, lambda x, y: gpu.local_align(x, y, sm, 1)), "slices")
    big = [16384] * 4200 + [int(x) for x in rng.integers(0, 3000, 300)]
    rng.shuffle(big)
    a3, b3 = _inputs(big, 23)
    _, off3 = gpu._ragged_seq1s(a3)
    assert len(gpu.local_ragged_slices_for(off3, affine=True, traceback=True)) >= 2
    _assert_ragged(gpu.local_align_affine_ragged(a3, b3, sm, 2, 1),
                   _by_length(a3, b3, lambda x, y: gpu.local_align_affine(x, y, sm, 2, 1)), "affine slices")


def test_device_entry_on_two_streams_in_flight(gpu):
    """Both device entries on torch buffers, four calls on two streams issued before any is waited for, equal the host entry."""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(31)
    sm = random_matrix(5)
    jobs = []
    for affine, n, top, seed in ((False, 4097, 3000, 1), (True, 1500, 16384, 2), (False, 700, 16384, 3), (True, 5000, 300, 4)):
        lens = [int(x) for x in rng.integers(0, top + 1, n)]
        a, b = _inputs(lens, seed)
        cat, off = gpu._ragged_seq1s(a)
        mo = gpu.local_ragged_move_offsets(off)
        t = dict(a=torch.from_numpy(np.concatenate([cat, np.zeros(16, np.uint8)])).to(dev), b=torch.from_numpy(b).to(dev),
                 sc=torch.zeros(n, dtype=torch.int32, device=dev), ends=torch.zeros((n, 4), dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]), dtype=torch.int64, device=dev), st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((affine, a, b, off, t, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    for affine, a, b, off, t, s in jobs:
        args = (t["a"].data_ptr(), off, t["b"].data_ptr(), sm)
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr(), t["st"].data_ptr())
        if affine:
            gpu.local_align_affine_ragged_device(*args, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            gpu.local_align_ragged_device(*args, 4, *bufs, stream=s.cuda_stream)
    for affine, a, b, off, t, s in jobs:
        s.synchronize()
        want = gpu.local_align_affine_ragged(a, b, sm, 7, 1) if affine else gpu.local_align_ragged(a, b, sm, 4)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64), want[3],
               t["st"].cpu().numpy().view(np.uint32))
        _assert_ragged(got, (want[0], want[1], want[4], [want[2][int(want[3][k]):int(want[3][k + 1])] for k in range(len(a))]),
                       ("device", affine))


def test_fuzz_200k_alignments_against_the_restatements(gpu, loracle, aoracle):
    rng = np.random.default_rng(41)
    n = 200_000
    lens = rng.integers(0, 2049, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    cat = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 128), dtype=np.uint8)
    for k in range(0, n, 5):               # a noisy copy of the seq2 in every fifth: long paths
        w = int(min(lens[k], 128))
        cat[int(off[k]):int(off[k]) + w] = np.where(rng.random(w) < 0.9, b[k, :w], cat[int(off[k]):int(off[k]) + w])
    sm = match_matrix(2, -3)
    a = [cat[int(off[k]):int(off[k + 1])] for k in range(n)]
    for name, got, fn in (("linear", gpu.local_align_ragged((cat, off), b, sm, 3), lambda x, y: loracle.align(x, y, sm, 3)),
                          ("affine", gpu.local_align_affine_ragged((cat, off), b, sm, 5, 1), lambda x, y: aoracle.align(x, y, sm, 5, 1))):
        sc, ends, moves, mo, steps = got
        wsc, wends, wsteps, wrows = _by_length(a, b, fn)
        bad = int((sc != wsc).sum()) + int((ends != wends).any(axis=1).sum()) + int((steps != wsteps).sum())
        for k in range(n):
            w = (int(steps[k]) + 31) // 32
            bad += 0 if np.array_equal(moves[int(mo[k]):int(mo[k]) + w], wrows[k][:w]) else 1
        assert bad == 0, name


def test_cpp_overloads_reproduce_f7_in_one_call(gpu, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    f7 = load_f7()
    data = tmp_path / "f7.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(len(f7)).tobytes())
        for v in f7:
            fh.write(np.int32(len(v["seq1"])).tobytes() + v["seq1"].tobytes() + v["seq2"].tobytes())
    exe = str(tmp_path / "compat_ragged")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_ragged.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "mismatches 0 0 0", lines[-1]
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == len(f7)
    for k, (score, length, si, sj, ei, ej, checksum) in enumerate(rows):
        p = f7[k]["path"]
        want = 0
        for i, j in p:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        assert (score, length, si, sj, ei, ej, checksum) == (f7[k]["score"], len(p), int(p[0][0]), int(p[0][1]), int(p[-1][0]),
                                                             int(p[-1][1]), want), k
