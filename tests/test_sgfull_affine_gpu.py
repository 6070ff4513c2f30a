"""The affine exact semi-global aligner (swmi_semiglobal_full_affine*) on the GPU, every field bit-exact against fixture F8
(the reference's SemiGlobal_111) at (1, -1, 1, 1), against the linear aligner at open = extend, and against the C
restatement tests/native/sgfull_affine_oracle.c (which test_sgfull_affine_cpu.py checks against an independent numpy Gotoh)
everywhere else."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS
from local_support import PARAMS, random_matrix
from sgfull_affine_support import SgAffineOracle
from sgfull_support import K111, load_f8, moves_to_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_affine_oracle"))


def _inputs(n, len1, len2, seed):
    """random pairs; every third seq2 a noisy copy of its seq1 with an indel of up to 40 bases (long E / F runs), every
    seventh pair a homopolymer (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 8:
            cut = int(rng.integers(1, w - 1))
            d = int(rng.integers(1, min(40, w - cut - 1) + 1)) if w - cut > 2 else 1
            src = np.concatenate([src[:cut], src[cut + d:], rng.integers(0, 4, d, dtype=np.uint8)]) if k % 2 else \
                np.concatenate([src[:cut], rng.integers(0, 4, d, dtype=np.uint8), src[cut:]])
        b[k, :w] = src[:w]
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b


def _mismatches(got, want, traceback=True):
    """alignments whose score, best cell, length or moves differ"""
    sc, ends, mv, ln = got
    wsc, wends, wmv, wln = want
    bad = (sc != wsc) | (ends != wends).any(axis=1)
    if traceback:
        bad |= ln != wln
        for k in np.flatnonzero(~bad):
            steps = int(ln[k]) - 1
            full, part = divmod(steps, 32)
            same = np.array_equal(mv[k, :full], wmv[k, :full])
            if part:
                mask = np.uint64((1 << (2 * part)) - 1)
                same = same and (mv[k, full] & mask) == (wmv[k, full] & mask)
            bad[k] = not same
    return np.flatnonzero(bad)


def _assert_same(got, want, what, traceback=True):
    bad = _mismatches(got, want, traceback)
    assert len(bad) == 0, (what, bad[:8])


def test_f8_through_the_host_entry(gpu):
    """(1, -1) with open = extend = 1 is SemiGlobal_111: F8's scores, best cells, lengths and paths."""
    f8 = load_f8()
    sc, ends, mv, ln = gpu.semiglobal_full_affine(f8["seq1"], f8["seq2"], K111, 1, 1)
    for k in range(len(f8["scores"])):
        assert sc[k] == f8["scores"][k] and tuple(ends[k]) == tuple(f8["ends"][k]) and ln[k] == f8["lengths"][k], (k, f8["kind"][k])
        path = f8["paths"][k]
        assert np.array_equal(gpu.semiglobal_expand_moves(mv[k], ln[k]), path), k
        assert np.array_equal(moves_to_path(mv[k], ln[k], ends[k, 0], ends[k, 1]), path), k
    sc2, ends2, _, _ = gpu.semiglobal_full_affine(f8["seq1"], f8["seq2"], K111, 1, 1, traceback=False)
    assert np.array_equal(sc2, sc) and np.array_equal(ends2, ends)
    gpu.semiglobal_full_affine_release_workspaces()


SHAPES = [(1, 1), (1, 16384), (16384, 1), (2, 3), (63, 65), (1000, 1000), (1023, 1025), (4096, 777), (16384, 16384)]


@pytest.mark.parametrize("len1,len2", SHAPES)
def test_length_grid_across_parameter_sets(gpu, aoracle, len1, len2):
    """Every (open, extend) of the grid with the PARAMS matrices in turn and one asymmetric matrix; at 16384 x 16384 a few."""
    big = len1 * len2 >= 1 << 26
    n = 2 if big else 12
    mats = [match_matrix(m, x) for m, x, _ in PARAMS] + [random_matrix(3)]
    cases = [(mats[q % len(mats)], go, ge) for q, (go, ge) in enumerate(AFFINE_GAPS)] + [(mats[-1], 6, 2), (mats[1], 1, 1)]
    if big:
        cases = [cases[3], cases[5], cases[-1]]          # (11, 1), (127, 127) and (1, 1) with (1, -1)
    for c, (sm, go, ge) in enumerate(cases):
        a, b = _inputs(n, len1, len2, 100 * c + len1 % 97 + len2 % 89)
        want = aoracle.align(a, b, sm, go, ge)
        _assert_same(gpu.semiglobal_full_affine(a, b, sm, go, ge), want, (len1, len2, c))
        sc, ends, _, _ = gpu.semiglobal_full_affine(a, b, sm, go, ge, traceback=False)
        _assert_same((sc, ends, None, None), want, (len1, len2, c, "ends-only"), traceback=False)
    if big:
        gpu.semiglobal_full_affine_release_workspaces()


@pytest.mark.parametrize("len1,len2", [(1, 1), (63, 65), (1023, 1025), (3000, 2000)])
def test_open_equal_extend_equals_the_linear_aligner(gpu, len1, len2):
    for p, (match, mismatch, g) in enumerate(PARAMS):
        sm = match_matrix(match, mismatch)
        a, b = _inputs(9, len1, len2, 7 * p + len1)
        _assert_same(gpu.semiglobal_full_affine(a, b, sm, g, g), gpu.semiglobal_full(a, b, sm, g), (len1, len2, p))


@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(gpu, aoracle, n):
    a, b = _inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    _assert_same(gpu.semiglobal_full_affine(a, b, sm, 7, 2), aoracle.align(a, b, sm, 7, 2), n)


def test_batch_across_a_slice_boundary(gpu, aoracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets."""
    n = 257
    assert gpu.semiglobal_full_affine_slices_for(n, 16384, 16384) == [256, 1]
    a, b = _inputs(n, 16384, 16384, 257)
    got = gpu.semiglobal_full_affine(a, b, K111, 3, 1)
    gpu.semiglobal_full_affine_release_workspaces()
    _assert_same(got, aoracle.align(a, b, K111, 3, 1), "slices")


def _device_buffers(a, b, n, len1, len2, gpu, dev):
    mw = gpu.semiglobal_full_move_words(len1, len2)
    return dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                ends=torch.zeros((n, 2), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                ln=torch.zeros(n, dtype=torch.int32, device=dev))


def _read(t):
    return (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64), t["ln"].cpu().numpy().view(np.uint32))


def test_device_entry_equals_host_entry_on_two_streams(gpu):
    """swmi_semiglobal_full_affine_device on torch buffers, two calls on two streams issued before either is waited for, each
    equal to the host entry; one traceback, one ends-only."""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, len2, n, seed, tb in ((3000, 5000, 40, 1, True), (1023, 16384, 9, 2, False)):
        a, b = _inputs(n, len1, len2, seed)
        jobs.append((len1, len2, n, a, b, _device_buffers(a, b, n, len1, len2, gpu, dev), tb, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, len2, n, a, b, t, tb, s in jobs:
        gpu.semiglobal_full_affine_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 9, 2, t["sc"].data_ptr(),
                                          t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["ln"].data_ptr() if tb else None,
                                          stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, s in jobs:
        s.synchronize()
        _assert_same(_read(t), gpu.semiglobal_full_affine(a, b, sm, 9, 2, traceback=tb), ("device", len1, len2), traceback=tb)


def test_host_entry_from_two_threads(gpu, aoracle):
    a, b = _inputs(300, 900, 1500, 9)
    sm = match_matrix(5, -4)
    want = aoracle.align(a, b, sm, 12, 0)
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.semiglobal_full_affine(a, b, sm, 12, 0)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        _assert_same(out[k], want, k)


def test_timer_runs_the_device_entry(gpu, aoracle):
    dev = torch.device("cuda:0")
    n, len1, len2 = 20, 2000, 3000
    a, b = _inputs(n, len1, len2, 4)
    t = _device_buffers(a, b, n, len1, len2, gpu, dev)
    sm = match_matrix(1, -1)
    ms = gpu.semiglobal_full_affine_time_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 5, 2, t["sc"].data_ptr(),
                                                t["ends"].data_ptr(), t["mv"].data_ptr(), t["ln"].data_ptr(), iters=3)
    assert ms > 0
    _assert_same(_read(t), aoracle.align(a, b, sm, 5, 2), "timer")


def test_cpp_overloads_equal_the_restatement(gpu, aoracle, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    n, len1, len2, go, ge = 13, 1500, 2200, 8, 1
    sm = random_matrix(7)
    a, b = _inputs(n, len1, len2, 13)
    data = tmp_path / "in.bin"
    with open(data, "wb") as fh:
        fh.write(np.asarray(sm, np.int8).tobytes() + np.array([go, ge, n, len1, len2], np.int32).tobytes())
        for k in range(n):
            fh.write(a[k].tobytes() + b[k].tobytes())
    exe = str(tmp_path / "compat_sgfull_affine")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_sgfull_affine.cpp"), "-o", exe, "-L", lib, "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "batch 0"
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == n
    sc, ends, mv, ln = aoracle.align(a, b, sm, go, ge)
    for k, (score, length, ei, ej, checksum) in enumerate(rows):
        p = moves_to_path(mv[k], ln[k], ends[k, 0], ends[k, 1])
        want = 0
        for i, j in p:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        assert (score, length, ei, ej, checksum) == (int(sc[k]), len(p), int(p[-1][0]), int(p[-1][1]), want), k


def test_seeded_fuzz(gpu, aoracle):
    """20 500 alignments over four shapes, each shape in chunks with a random matrix and random (open, extend)."""
    rng = np.random.default_rng(20260)
    total = bad = 0
    for len1, len2, n in ((37, 45, 8000), (130, 90, 8000), (260, 1100, 3000), (1500, 300, 1500)):
        for c in range(4):
            m = n // 4
            sm = rng.integers(-128, 128, 16).astype(np.int8)
            go, ge = (int(x) for x in rng.integers(0, 128, 2))
            if c == 0:
                go, ge = int(rng.integers(0, 20)), int(rng.integers(0, 5))
            a, b = _inputs(m, len1, len2, int(rng.integers(1 << 30)))
            want = aoracle.align(a, b, sm, go, ge)
            got = gpu.semiglobal_full_affine(a, b, sm, go, ge)
            bad += len(_mismatches(got, want))
            sc, ends, _, _ = gpu.semiglobal_full_affine(a, b, sm, go, ge, traceback=False)
            bad += len(_mismatches((sc, ends, None, None), want, traceback=False))
            total += m
    assert total >= 20000
    assert bad == 0
