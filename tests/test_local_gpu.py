"""The local aligner with traceback (swmi_local_*) on the GPU, every field bit-exact against the C restatement
tests/native/local_oracle.c -- which itself reproduces fixture F7, the reference's SmithWaterman_111_long, field for field
(test_local_cpu.py).  For matrices other than (1,1,1) the end cell and the path rest on the stated rule (row-major-first end
cell; diagonal, then up, then left): the reference has no such function to pin them to."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_support import PARAMS, LocalOracle, f7_by_length, moves_to_path, random_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def _mixed_inputs(n, len1, seed):
    """random pairs, with every third seq1 carrying a noisy copy of its seq2 (long paths) and some homopolymers (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 128), dtype=np.uint8)
    for k in range(0, n, 3):
        w = min(len1, 128)
        src = np.where(rng.random(w) < 0.85, b[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        at = int(rng.integers(0, len1 - w + 1))
        a[k, at:at + w] = src
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(128) < 0.8] = k & 3
    return a, b


def _assert_same(gpu_result, want, what):
    sc, ends, moves, steps = gpu_result
    wsc, wends, wmoves, wsteps = want
    assert np.array_equal(sc, wsc), what
    assert np.array_equal(ends, wends), what
    assert np.array_equal(steps, wsteps), what
    for k in range(len(sc)):
        words = (int(steps[k]) + 31) // 32
        assert np.array_equal(moves[k, :words], wmoves[k, :words]), (what, k)


def _matrices():
    return [match_matrix(m, x) for m, x, _ in PARAMS] + [random_matrix()], [g for _, _, g in PARAMS] + [6]


@pytest.mark.parametrize("p", range(6))
def test_parameter_sets_against_the_restatement(gpu, loracle, p):
    mats, gaps = _matrices()
    for len1, n in ((128, 65), (1, 3), (63, 65), (300, 65), (1000, 17), (4096, 3)):
        a, b = _mixed_inputs(n, len1, 100 + p + len1)
        _assert_same(gpu.local_align(a, b, mats[p], gaps[p]), loracle.align(a, b, mats[p], gaps[p]), (p, len1))


def test_every_f7_vector(gpu, loracle):
    """Score, end cell, start cell and the reference's whole path, for every length and input kind of F7."""
    for len1, (a, b, scores, paths) in f7_by_length().items():
        sc, ends, moves, steps = gpu.local_align(a, b, match_matrix(1, -1), 1)
        assert np.array_equal(sc, scores), len1
        for k in range(len(scores)):
            assert tuple(ends[k, :2]) == tuple(paths[k][-1]) and tuple(ends[k, 2:]) == tuple(paths[k][0]), (len1, k)
            got = gpu.local_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1])
            assert np.array_equal(got, paths[k]), (len1, k)
            assert np.array_equal(moves_to_path(moves[k], steps[k], ends[k, 0], ends[k, 1]), paths[k]), (len1, k)


@pytest.mark.parametrize("n", [1, 3, 65, 4097])
def test_batch_sizes(gpu, loracle, n):
    a, b = _mixed_inputs(n, 128, n)
    sm = match_matrix(10, -30)
    _assert_same(gpu.local_align(a, b, sm, 15), loracle.align(a, b, sm, 15), n)


def test_batch_of_several_slices(gpu, loracle):
    len1 = 16384
    n = 1100
    assert len(gpu.local_slices_for(n, len1, True)) >= 3
    a, b = _mixed_inputs(n, len1, 5)
    sm = match_matrix(2, -3)
    _assert_same(gpu.local_align(a, b, sm, 5), loracle.align(a, b, sm, 5), "slices")


def test_ends_only_matches_traceback_mode(gpu):
    for len1, n in ((128, 4097), (129, 300), (16384, 40)):
        a, b = _mixed_inputs(n, len1, len1)
        for sm, gap in ((match_matrix(1, -1), 1), (random_matrix(3), 4)):
            sc, ends, _, _ = gpu.local_align(a, b, sm, gap)
            sc2, ends2, mv, st = gpu.local_align(a, b, sm, gap, traceback=False)
            assert mv is None and st is None
            assert np.array_equal(sc, sc2) and np.array_equal(ends[:, :2], ends2[:, :2])
            assert (ends2[:, 2:] == -1).all()


def test_scores_equal_the_128x128_scorer_on_1m_pairs(gpu):
    n = 1 << 20
    a, b = gpu.generate_pairs_host(n, 77, 0)
    for sm, gap in ((match_matrix(10, -30), 15), (match_matrix(1, -1), 1), (random_matrix(9), 3)):
        want = gpu.score_batch(a, b, sm, gap)
        got, _, _, _ = gpu.local_align(a, b, sm, gap, traceback=False)
        assert np.array_equal(got, want)
        got_tb, _, _, _ = gpu.local_align(a, b, sm, gap)
        assert np.array_equal(got_tb, want)


def test_device_entry_on_two_streams_in_flight(gpu, loracle):
    """swmi_local_align_device on torch buffers, two calls on two streams issued before either is waited for."""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, n, seed in ((128, 4097, 1), (1000, 513, 2)):
        a, b = _mixed_inputs(n, len1, seed)
        mw = gpu.local_move_words(len1)
        bufs = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                    ends=torch.zeros((n, 4), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                    st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((len1, n, a, b, bufs, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, n, a, b, t, s in jobs:
        gpu.local_align_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), n, sm, 2, t["sc"].data_ptr(), t["ends"].data_ptr(),
                               t["mv"].data_ptr(), t["st"].data_ptr(), stream=s.cuda_stream)
    for len1, n, a, b, t, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["st"].cpu().numpy().view(np.uint32))
        _assert_same(got, loracle.align(a, b, sm, 2), ("stream", len1))


def test_host_entry_from_two_threads(gpu, loracle):
    a, b = _mixed_inputs(700, 300, 9)
    sm = match_matrix(5, -4)
    want = loracle.align(a, b, sm, 0)
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.local_align(a, b, sm, 0)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        _assert_same(out[k], want, k)


def test_cpp_overloads_reproduce_f7(gpu, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    groups = f7_by_length()
    data = tmp_path / "f7.bin"
    paths = []
    with open(data, "wb") as fh:
        fh.write(np.int32(sum(len(g[2]) for g in groups.values())).tobytes())
        for len1, (a, b, scores, ps) in groups.items():
            for k in range(len(scores)):
                fh.write(np.int32(len1).tobytes() + a[k].tobytes() + b[k].tobytes())
                paths.append((int(scores[k]), ps[k]))
    exe = str(tmp_path / "compat_local")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "batch 0"
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == len(paths)
    for k, (score, length, si, sj, ei, ej, checksum) in enumerate(rows):
        want_score, p = paths[k]
        want = 0
        for i, j in p:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        assert (score, length, si, sj, ei, ej, checksum) == (want_score, len(p), int(p[0][0]), int(p[0][1]), int(p[-1][0]),
                                                             int(p[-1][1]), want), k
