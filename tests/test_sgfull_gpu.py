"""The exact semi-global aligner (swmi_semiglobal_full*) on the GPU, every field bit-exact against fixture F8 (the
reference's SemiGlobal_111) or the C restatement tests/native/sgfull_oracle.c, which reproduces F8 field for field
(test_sgfull_cpu.py).  For matrices other than (1,-1,1) and gaps other than 1 the best cell and the path rest on the stated
rule (row-major-first best cell; diagonal, then up, then left): the reference has no such function to pin them to."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_support import PARAMS, random_matrix
from sgfull_support import K111, SgFullOracle, load_f8, moves_to_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


def _inputs(n, len1, len2, seed):
    """random pairs; every third seq2 a noisy copy of its seq1 with an indel (long diagonal paths), every seventh pair a
    homopolymer (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 8:
            cut = int(rng.integers(1, w - 1))
            src = np.concatenate([src[:cut], src[cut + min(5, w - cut - 1):], rng.integers(0, 4, min(5, w - cut - 1), dtype=np.uint8)])
        b[k, :w] = src[:w]
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b


def _assert_same(got, want, what, traceback=True):
    sc, ends, mv, ln = got
    wsc, wends, wmv, wln = want
    assert np.array_equal(sc, wsc), (what, np.flatnonzero(sc != wsc)[:8])
    assert np.array_equal(ends, wends), (what, np.flatnonzero((ends != wends).any(axis=1))[:8])
    if traceback:
        assert np.array_equal(ln, wln), (what, np.flatnonzero(ln != wln)[:8])
        for k in range(len(sc)):
            steps = int(ln[k]) - 1
            full, part = divmod(steps, 32)
            assert np.array_equal(mv[k, :full], wmv[k, :full]), (what, k)
            if part:
                mask = np.uint64((1 << (2 * part)) - 1)
                assert (mv[k, full] & mask) == (wmv[k, full] & mask), (what, k)


def test_f8_through_the_host_entry(gpu):
    f8 = load_f8()
    sc, ends, mv, ln = gpu.semiglobal_full(f8["seq1"], f8["seq2"], K111, 1)
    for k in range(len(f8["scores"])):
        assert sc[k] == f8["scores"][k] and tuple(ends[k]) == tuple(f8["ends"][k]) and ln[k] == f8["lengths"][k], (k, f8["kind"][k])
        path = f8["paths"][k]
        assert np.array_equal(gpu.semiglobal_expand_moves(mv[k], ln[k]), path), k
        assert np.array_equal(moves_to_path(mv[k], ln[k], ends[k, 0], ends[k, 1]), path), k
    sc2, ends2, _, _ = gpu.semiglobal_full(f8["seq1"], f8["seq2"], K111, 1, traceback=False)
    assert np.array_equal(sc2, sc) and np.array_equal(ends2, ends)


SHAPES = [(1, 1), (1, 16384), (16384, 1), (2, 3), (63, 65), (1000, 1000), (1023, 1025), (4096, 777), (16384, 16384)]


@pytest.mark.parametrize("len1,len2", SHAPES)
def test_length_grid_across_parameter_sets(gpu, sgoracle, len1, len2):
    n = 2 if len1 * len2 >= 1 << 26 else 24
    params = [(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(3), 4)]
    for p, (sm, gap) in enumerate(params):
        if len1 * len2 >= 1 << 26 and p not in (1, 2, 3):
            continue                                    # at 16384 x 16384: (1,-1,1), gap 0 and (127,-127,127)
        a, b = _inputs(n, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        want = sgoracle.align(a, b, sm, gap)
        _assert_same(gpu.semiglobal_full(a, b, sm, gap), want, (len1, len2, p))
        sc, ends, _, _ = gpu.semiglobal_full(a, b, sm, gap, traceback=False)
        _assert_same((sc, ends, None, None), want, (len1, len2, p, "ends-only"), traceback=False)


@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(gpu, sgoracle, n):
    a, b = _inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    _assert_same(gpu.semiglobal_full(a, b, sm, 5), sgoracle.align(a, b, sm, 5), n)


def test_batch_across_a_slice_boundary(gpu, sgoracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets."""
    n = 257
    assert gpu.semiglobal_full_slices_for(n, 16384, 16384) == [256, 1]
    a, b = _inputs(n, 16384, 16384, 257)
    got = gpu.semiglobal_full(a, b, K111, 1)
    gpu.semiglobal_full_release_workspaces()
    _assert_same(got, sgoracle.align(a, b, K111, 1), "slices")


def test_device_entry_equals_host_entry_on_two_streams(gpu):
    """swmi_semiglobal_full_device on torch buffers, two calls on two streams issued before either is waited for, each
    equal to the host entry; one traceback, one ends-only."""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, len2, n, seed, tb in ((3000, 5000, 40, 1, True), (1023, 16384, 9, 2, False)):
        a, b = _inputs(n, len1, len2, seed)
        mw = gpu.semiglobal_full_move_words(len1, len2)
        t = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                 ends=torch.zeros((n, 2), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                 ln=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((len1, len2, n, a, b, t, tb, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, len2, n, a, b, t, tb, s in jobs:
        gpu.semiglobal_full_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 2, t["sc"].data_ptr(),
                                   t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["ln"].data_ptr() if tb else None,
                                   stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["ln"].cpu().numpy().view(np.uint32))
        _assert_same(got, gpu.semiglobal_full(a, b, sm, 2, traceback=tb), ("device", len1, len2), traceback=tb)


def test_host_entry_from_two_threads(gpu, sgoracle):
    a, b = _inputs(300, 900, 1500, 9)
    sm = match_matrix(5, -4)
    want = sgoracle.align(a, b, sm, 0)
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.semiglobal_full(a, b, sm, 0)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        _assert_same(out[k], want, k)


def test_cpp_overloads_reproduce_f8(gpu, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    f8 = load_f8()
    n = len(f8["scores"])
    data = tmp_path / "f8.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(n).tobytes())
        for k in range(n):
            fh.write(f8["seq1"][k].tobytes() + f8["seq2"][k].tobytes())
    exe = str(tmp_path / "compat_sgfull")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_sgfull.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "batch 0"
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == n
    for k, (score, length, ei, ej, checksum) in enumerate(rows):
        p = f8["paths"][k]
        want = 0
        for i, j in p:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        assert (score, length, ei, ej, checksum) == (int(f8["scores"][k]), len(p), int(p[-1][0]), int(p[-1][1]), want), k


def _generator_pairs(n, seed):
    """The reference's 70 %-identity generator (source.cpp:2748-2771): 10 % mismatch, 10 % insertion, 10 % deletion."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, 16384), dtype=np.uint8)
    b = np.empty_like(a)
    for k in range(n):
        p = rng.integers(0, 100, 3 * 16384)
        fresh = rng.integers(0, 4, 3 * 16384, dtype=np.uint8)
        i = j = t = 0
        while i < 16384:
            if j == 16384:
                b[k, i] = fresh[t]
                i += 1
            elif p[t] < 10:
                b[k, i] = fresh[t]
                i += 1
                j += 1
            elif p[t] < 20:
                b[k, i] = fresh[t]
                i += 1
            elif p[t] < 30:
                j += 1
            else:
                b[k, i] = a[k, j]
                i += 1
                j += 1
            t += 1
    return a, b


def test_exact_bounds_xdrop_on_generator_pairs(gpu):
    """256 pairs of the reference's generator: the exact score is at least the X-drop score on every pair (the agreement
    rate is what the reference's commented-out assert(ans1 == ans2) would have measured)."""
    a, b = _generator_pairs(256, 2748)
    exact, _, _, _ = gpu.semiglobal_full(a, b, K111, 1, traceback=False)
    xdrop, _, _ = gpu.semiglobal_xdrop(a, b, cap=1)
    assert np.all(exact >= xdrop), np.flatnonzero(exact < xdrop)[:8]
    print("exact == x-drop on %d of 256 generator pairs; mean exact - x-drop %.2f" % (int((exact == xdrop).sum()),
                                                                                     float((exact - xdrop).mean())))
