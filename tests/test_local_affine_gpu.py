"""The affine local aligner (swmi_local_align_affine*) on the GPU, every field bit-exact against the C restatement
tests/native/local_affine_oracle.c -- which itself equals an independent numpy formulation, the linear restatement at
open = extend, and fixture F7 at (1, -1, 1, 1) (test_local_affine_cpu.py).  The lengths and batch sizes are the tiling edges
of tests/table_edges.py: one to three lanes' worth of columns past a row, one alignment past a wavefront and a workgroup."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle, hand_cases, mixed_inputs, moves_as_letters, runs
from local_support import f7_by_length, moves_to_path, random_matrix

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 1000, 16384]
BATCHES = [1, 3, 4, 5, 17, 65, 257]


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


def _assert_same(got, want, what):
    sc, ends, moves, steps = got
    wsc, wends, wmoves, wsteps = want
    assert np.array_equal(sc, wsc), what
    assert np.array_equal(ends, wends), what
    assert np.array_equal(steps, wsteps), what
    for k in range(len(sc)):
        words = (int(steps[k]) + 31) // 32
        assert np.array_equal(moves[k, :words], wmoves[k, :words]), (what, k)


def test_f7_at_open_equal_extend_one_is_the_reference(gpu):
    """Every F7 vector through the host entry at (1, -1, open 1, extend 1): the reference's SmithWaterman_111_long."""
    bad = 0
    for len1, (a, b, scores, paths) in f7_by_length().items():
        sc, ends, moves, steps = gpu.local_align_affine(a, b, match_matrix(1, -1), 1, 1)
        bad += int((sc != scores).sum())
        for k in range(len(scores)):
            ok = tuple(ends[k, :2]) == tuple(paths[k][-1]) and tuple(ends[k, 2:]) == tuple(paths[k][0])
            ok = ok and np.array_equal(gpu.local_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1]), paths[k])
            bad += 0 if ok else 1
    assert bad == 0


@pytest.mark.parametrize("g", range(len(AFFINE_GAPS)))
def test_parameter_grid_at_the_tiling_edges(gpu, aoracle, golden, g):
    f = golden("f1_random")
    go, ge = AFFINE_GAPS[g]
    mats = list(f["sm"]) + [random_matrix(g)]
    for x, len1 in enumerate(LENGTHS):
        n = BATCHES[(x + g) % len(BATCHES)] if len1 < 1000 else 1 + (x + g) % 5
        sm = mats[(x + 3 * g) % len(mats)]
        a, b = mixed_inputs(n, len1, 1000 * g + len1)
        _assert_same(gpu.local_align_affine(a, b, sm, go, ge), aoracle.align(a, b, sm, go, ge), (g, len1, n))


@pytest.mark.parametrize("n", BATCHES)
def test_batch_sizes(gpu, aoracle, n):
    a, b = mixed_inputs(n, 129, n)
    sm = match_matrix(2, -3)
    _assert_same(gpu.local_align_affine(a, b, sm, 5, 2), aoracle.align(a, b, sm, 5, 2), n)


def test_hand_checked_cases(gpu, aoracle):
    want_runs = {"deletion10": ("L", 10), "left100": ("L", 100), "up3000": ("U", 3000)}
    for name, a, b, sm, go, ge, score in hand_cases():
        got = gpu.local_align_affine(a, b, sm, go, ge)
        _assert_same(got, aoracle.align(a, b, sm, go, ge), name)
        sc, ends, moves, steps = got
        assert sc[0] == score, name
        assert [r for r in runs(moves_as_letters(moves[0], steps[0])) if r[0] != "D"] == [want_runs[name]], name
        if name == "deletion10":
            assert tuple(ends[0]) == (118, 128, 0, 0)


def test_all_mismatch_and_homopolymer_ties(gpu, aoracle):
    n, len1 = 65, 300
    a = np.zeros((n, len1), np.uint8)
    b = np.ones((n, 128), np.uint8)                              # every cell a mismatch: score 0, end (0,0)
    sm = match_matrix(3, -2)
    for go, ge in AFFINE_GAPS:
        got = gpu.local_align_affine(a, b, sm, go, ge)
        _assert_same(got, aoracle.align(a, b, sm, go, ge), ("mismatch", go, ge))
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[3] == 0).all()
    a = np.full((n, len1), 2, np.uint8)                          # one base everywhere: ties at every cell
    b = np.full((n, 128), 2, np.uint8)
    b[::2, 40:50] = 1
    for sm, go, ge in ((match_matrix(1, -1), 1, 1), (match_matrix(2, -2), 0, 0), (match_matrix(4, -1), 3, 0),
                       (random_matrix(2), 2, 5)):
        _assert_same(gpu.local_align_affine(a, b, sm, go, ge), aoracle.align(a, b, sm, go, ge), ("homopolymer", go, ge))


def test_ends_only_matches_traceback_mode(gpu):
    for len1, n in ((128, 4097), (129, 300), (16384, 40)):
        a, b = mixed_inputs(n, len1, len1)
        for sm, go, ge in ((match_matrix(1, -1), 1, 1), (random_matrix(3), 7, 2), (match_matrix(2, -3), 0, 4)):
            sc, ends, _, _ = gpu.local_align_affine(a, b, sm, go, ge)
            sc2, ends2, mv, st = gpu.local_align_affine(a, b, sm, go, ge, traceback=False)
            assert mv is None and st is None
            assert np.array_equal(sc, sc2) and np.array_equal(ends[:, :2], ends2[:, :2])
            assert (ends2[:, 2:] == -1).all()


def _device_buffers(gpu, a, b, dev):
    n, len1 = a.shape
    mw = gpu.local_move_words(len1)
    return dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                ends=torch.zeros((n, 4), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                st=torch.zeros(n, dtype=torch.int32, device=dev))


def _from_device(t):
    return (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64), t["st"].cpu().numpy().view(np.uint32))


def test_device_entry_equals_host_entry_on_two_streams_in_flight(gpu):
    """swmi_local_align_affine_device on torch buffers, two calls on two streams issued before either is waited for."""
    dev = torch.device("cuda:0")
    sm = random_matrix(5)
    jobs = []
    for len1, n, seed, go, ge in ((128, 4097, 1, 6, 1), (1000, 513, 2, 2, 9)):
        a, b = mixed_inputs(n, len1, seed)
        jobs.append((a, b, go, ge, _device_buffers(gpu, a, b, dev), torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    for a, b, go, ge, t, s in jobs:
        gpu.local_align_affine_device(t["a"].data_ptr(), a.shape[1], t["b"].data_ptr(), a.shape[0], sm, go, ge, t["sc"].data_ptr(),
                                      t["ends"].data_ptr(), t["mv"].data_ptr(), t["st"].data_ptr(), stream=s.cuda_stream)
    for a, b, go, ge, t, s in jobs:
        s.synchronize()
        _assert_same(_from_device(t), gpu.local_align_affine(a, b, sm, go, ge), ("stream", a.shape))


def test_timer_runs_the_device_entry(gpu, aoracle):
    dev = torch.device("cuda:0")
    a, b = mixed_inputs(257, 200, 8)
    t = _device_buffers(gpu, a, b, dev)
    sm = match_matrix(2, -3)
    ms = gpu.local_affine_time_device(t["a"].data_ptr(), 200, t["b"].data_ptr(), 257, sm, 5, 2, t["sc"].data_ptr(), t["ends"].data_ptr(),
                                      t["mv"].data_ptr(), t["st"].data_ptr(), iters=3)
    assert ms > 0
    _assert_same(_from_device(t), aoracle.align(a, b, sm, 5, 2), "timer")


def test_host_call_of_several_slices(gpu, aoracle):
    len1, n = 16384, 4096 + 5
    assert gpu.local_affine_slices_for(n, len1, True) == [4096, 5]
    a, b = mixed_inputs(n, len1, 5)
    sm = match_matrix(2, -3)
    _assert_same(gpu.local_align_affine(a, b, sm, 5, 2), aoracle.align(a, b, sm, 5, 2), "slices")


def test_fuzz_200k_alignments(gpu, aoracle):
    """262 144 alignments in four groups of lengths and parameters: 0 mismatches in any field."""
    rng = np.random.default_rng(2026)
    mismatches = 0
    for len1, sm, go, ge in ((128, match_matrix(2, -3), 5, 2), (64, random_matrix(21), 3, 7), (200, match_matrix(1, -1), 11, 1),
                             (37, random_matrix(22), 0, 5)):
        n = 1 << 16
        a, b = mixed_inputs(n, len1, int(rng.integers(1 << 30)))
        sc, ends, moves, steps = gpu.local_align_affine(a, b, sm, go, ge)
        wsc, wends, wmoves, wsteps = aoracle.align(a, b, sm, go, ge)
        bad = (sc != wsc) | (ends != wends).any(axis=1) | (steps != wsteps)
        words = (int(wsteps.max()) + 31) // 32
        mask = (np.arange(words)[None, :] * 32) < wsteps[:, None].astype(np.int64)
        bad |= ((moves[:, :words] != wmoves[:, :words]) & mask).any(axis=1)
        mismatches += int(bad.sum())
    assert mismatches == 0


def test_cpp_overloads_against_the_restatement(gpu, aoracle, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    sm, go, ge = random_matrix(4), 4, 1
    groups = [mixed_inputs(n, len1, len1) for len1, n in ((1, 2), (129, 7), (3000, 4))]
    data = tmp_path / "in.bin"
    want = []
    with open(data, "wb") as fh:
        fh.write(sm.astype(np.int8).tobytes() + np.int32(go).tobytes() + np.int32(ge).tobytes())
        fh.write(np.int32(sum(len(a) for a, _ in groups)).tobytes())
        for a, b in groups:
            sc, ends, moves, steps = aoracle.align(a, b, sm, go, ge)
            for k in range(len(a)):
                fh.write(np.int32(a.shape[1]).tobytes() + a[k].tobytes() + b[k].tobytes())
                want.append((int(sc[k]), moves_to_path(moves[k], steps[k], ends[k, 0], ends[k, 1])))
    exe = str(tmp_path / "compat_affine")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_affine.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "batch 0"
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == len(want)
    for k, (score, length, si, sj, ei, ej, checksum) in enumerate(rows):
        ws, p = want[k]
        s = 0
        for i, j in p:
            s = (s * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        assert (score, length, si, sj, ei, ej, checksum) == (ws, len(p), int(p[0][0]), int(p[0][1]), int(p[-1][0]), int(p[-1][1]), s), k
