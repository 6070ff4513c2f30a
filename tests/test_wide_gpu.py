"""The wide-alphabet aligners (libswmi_wide.so, swmi.wide) on the GPU.  Every comparison is exact integer equality.  Both kinds,
with a traceback and ends-only, against the C restatement tests/native/wide_affine_oracle.c at the lane (16 columns), wave
(1024), chunk (32 rows) and staging (128 rows) edges and at the last column the profile holds (4096), on all 32 letters with
junk in the bytes' high bits, under four matrices; the global kind under all 16 masks at the small shapes; DNA-coded batches
with an embedded 4 x 4 matrix against the merged 4-letter ragged aligners, zero lengths included, field by field and move by
move; wave counts 1 - 4 side by side; the device entries on two streams; a host call of two slices; the C++ overloads."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from local_support import random_matrix
from wide_support import (ALL_MASKS, GLOBAL, LOCAL, WideOracle, assert_same, asymmetric_matrix, concat, inputs, moves_of, offsets,
                          only_letter_31, scoring_matrix)

pytestmark = pytest.mark.gpu

LEN1S = [1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [1, 15, 16, 17, 1023, 1024, 1025, 2049, 3073, 4096]
EXTRA = [(16384, 3), (5, 4096)]
SHAPES = [(p, q) for p in LEN1S for q in LEN2S] + EXTRA
SMALL = [(p, q) for p in LEN1S for q in LEN2S[:4]]
ZERO_SHAPES = [(0, 0), (0, 1), (1, 0), (0, 33), (33, 0), (0, 1025), (16384, 0), (0, 4096)]
MATRICES = {"asymmetric": lambda: scoring_matrix(3), "random_int8": lambda: asymmetric_matrix(4), "all_-128": lambda: np.full(1024, -128, np.int8),
            "all_127": lambda: np.full(1024, 127, np.int8), "only_31": only_letter_31}
GAPS = {"asymmetric": (6, 1), "random_int8": (40, 9), "all_-128": (3, 2), "all_127": (0, 0), "only_31": (2, 1)}


@pytest.fixture(scope="module")
def woracle(tmp_path_factory):
    return WideOracle(tmp_path_factory.mktemp("wide_gpu_oracle"))


@pytest.fixture(scope="module")
def wide(swmi_mod):
    """The library needs no swmi.init(): it runs on the current device."""
    swmi_mod.wide.load()
    return swmi_mod.wide


@pytest.fixture(scope="module")
def batch():
    """The shapes above in one batch, and a permutation of it; never changed by a test."""
    a, b = inputs(SHAPES, seed=7)
    perm = np.random.default_rng(8).permutation(len(a))
    return a, b, perm


def _run(wide, kind, a, b, sm, gaps, mask, traceback):
    if kind == LOCAL:
        return wide.local(a, b, sm, gaps[0], gaps[1], traceback=traceback)
    return wide.global_(a, b, sm, gaps[0], gaps[1], mask, traceback=traceback)


@pytest.mark.parametrize("matrix", sorted(MATRICES))
@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_every_field_equals_the_restatement(wide, woracle, batch, kind, matrix):
    a, b, perm = batch
    sm, gaps = MATRICES[matrix](), GAPS[matrix]
    for mask in ([0] if kind == LOCAL else [0, 15, 10, 5]):
        want = woracle.align(kind, a, b, sm, gaps[0], gaps[1], mask)
        print(kind, matrix, mask, "scores", int(want[0].min()), int(want[0].max()), "steps", int(want[4].max()))
        assert_same(_run(wide, kind, a, b, sm, gaps, mask, True), want, (kind, matrix, mask, "traceback"))
        ends_only = woracle.align(kind, a, b, sm, gaps[0], gaps[1], mask, traceback=False)
        assert_same(_run(wide, kind, a, b, sm, gaps, mask, False), ends_only, (kind, matrix, mask, "ends-only"), traceback=False)
    # permuted: every result follows its alignment
    pa, pb = [a[k] for k in perm], [b[k] for k in perm]
    mask = 0 if kind == LOCAL else 10
    assert_same(_run(wide, kind, pa, pb, sm, gaps, mask, True), woracle.align(kind, pa, pb, sm, gaps[0], gaps[1], mask), (kind, matrix, "permuted"))


def test_the_letters_and_the_paths_are_not_trivial(woracle, batch):
    """What the comparisons above rest on: all 32 letters and junk bits occur, and under the scoring matrix the paths hold all
    three kinds of move and cross every wave boundary."""
    a, b, _ = batch
    cat = np.concatenate(a + b)
    assert len(np.unique(cat & 31)) == 32 and len(np.unique(cat >> 5)) == 8
    want = woracle.align(GLOBAL, a, b, scoring_matrix(3), 6, 1, 0)
    k = SHAPES.index((128, 4096))          # a seq2 that ends in a noisy copy of its seq1: the path crosses all four waves
    assert k % 3 == 0
    codes = moves_of(want, k)
    assert {1, 3} <= set(codes) and codes.count(3) > 60 and int(want[1][k, 1]) == 4096
    assert any(2 in moves_of(want, x) for x in range(0, len(a), 3))
    local = woracle.align(LOCAL, a, b, only_letter_31(), 2, 1)
    assert local[0].max() >= 5 and local[0].min() == 0


def test_global_kind_under_all_16_masks_at_the_small_shapes(wide, woracle):
    a, b = inputs(SMALL, seed=17)
    sm = scoring_matrix(5)
    for mask in ALL_MASKS:
        assert_same(wide.global_(a, b, sm, 4, 1, mask), woracle.align(GLOBAL, a, b, sm, 4, 1, mask), ("masks", mask))
        assert_same(wide.global_(a, b, sm, 4, 1, mask, traceback=False), woracle.align(GLOBAL, a, b, sm, 4, 1, mask, traceback=False),
                    ("masks ends-only", mask), traceback=False)


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_dna_batches_with_embed_dna_equal_the_merged_ragged_aligners(gpu, wide, kind):
    """Pins the tie rules to merged code: swmi_local_full_affine_ragged / swmi_global_full_affine_ragged on the same batch."""
    shapes = SHAPES + ZERO_SHAPES
    a, b = inputs(shapes, seed=27, letters=4, junk=False)
    perm = np.random.default_rng(28).permutation(len(a))
    a, b = [a[k] for k in perm], [b[k] for k in perm]
    for x, (sm16, gaps) in enumerate(((random_matrix(5), (5, 1)), (np.asarray([2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2], np.int8), (0, 0)),
                       (random_matrix(9), (1, 3)))):
        sm32 = wide.embed_dna(sm16)
        for mask in ([0] if kind == LOCAL else ALL_MASKS if x == 0 else [0, 6, 15]):
            for tb in (True, False):
                if kind == LOCAL:
                    want = gpu.local_full_affine_ragged(a, b, sm16, gaps[0], gaps[1], traceback=tb)
                else:
                    want = gpu.global_ragged.global_full_affine_ragged(a, b, sm16, gaps[0], gaps[1], mask, traceback=tb)
                assert_same(_run(wide, kind, a, b, sm32, gaps, mask, tb), want, ("dna", kind, mask, tb, gaps), traceback=tb)


def test_wave_counts_one_to_four_side_by_side(wide, woracle):
    shapes = [(70, 100), (70, 1500), (70, 2500), (70, 4000), (300, 4096), (300, 1), (0, 7), (150, 3072), (150, 2048), (150, 1024)] * 3
    a, b = inputs(shapes, seed=37)
    sm = scoring_matrix(9)
    assert_same(wide.local(a, b, sm, 5, 2), woracle.align(LOCAL, a, b, sm, 5, 2), "waves local")
    assert_same(wide.global_(a, b, sm, 5, 2, 12), woracle.align(GLOBAL, a, b, sm, 5, 2, 12), "waves global")


def test_device_entries_on_two_streams_in_flight(wide, woracle, swmi_mod):
    """Both device entries on torch buffers, four calls on two streams issued before either is waited for."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(41)
    sm = scoring_matrix(11)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    for x, (kind, tb, n, mask) in enumerate(((LOCAL, True, 130, 0), (GLOBAL, True, 90, 15), (LOCAL, False, 200, 0), (GLOBAL, False, 150, 10))):
        shapes = [(int(p), int(q)) for p, q in rng.integers(0, 1101, (n, 2))] + [(40, 4096), (33, 2049)]
        a, b = inputs(shapes, seed=50 + x)
        off1, off2 = offsets(a), offsets(b)
        mo = swmi_mod.local_full_ragged_move_offsets(off1, off2)
        m = len(a)
        t = dict(a=torch.from_numpy(concat(a)).to(dev), b=torch.from_numpy(concat(b)).to(dev),
                 sc=torch.zeros(m, dtype=torch.int32, device=dev), ends=torch.zeros((m, 4), dtype=torch.int32, device=dev),
                 mv=torch.zeros(int(mo[-1]) + 2, dtype=torch.int64, device=dev), st=torch.zeros(m, dtype=torch.int32, device=dev))
        jobs.append((kind, tb, mask, a, b, off1, off2, mo, t, streams[x % 2]))
    torch.cuda.synchronize()
    for kind, tb, mask, a, b, off1, off2, mo, t, s in jobs:
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None)
        if kind == LOCAL:
            wide.local_device(t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            wide.global_device(t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, mask, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    for kind, tb, mask, a, b, off1, off2, mo, t, s in jobs:
        want = woracle.align(kind, a, b, sm, 7, 1, mask, traceback=tb)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64) if tb else None, mo if tb else None,
               t["st"].cpu().numpy().view(np.uint32) if tb else None)
        assert_same(got, want, ("device", kind, tb), traceback=tb)
        assert np.any(want[0] != 0)
    # the timer runs the same launches
    kind, tb, mask, a, b, off1, off2, mo, t, s = jobs[1]
    ms = wide.time_device(wide.GLOBAL, t["a"].data_ptr(), off1, t["b"].data_ptr(), off2, sm, 7, 1, mask, t["sc"].data_ptr(), t["ends"].data_ptr(),
                          t["mv"].data_ptr(), t["st"].data_ptr(), stream=s.cuda_stream, iters=2)
    assert ms > 0
    wide.release_workspaces()


def test_host_call_of_two_slices_by_the_count_cap(wide, woracle):
    """2^20 + 5 alignments with lengths in [0, 4], ends-only: two slices, results at the caller's positions."""
    rng = np.random.default_rng(21)
    n = (1 << 20) + 5
    off1 = np.zeros(n + 1, np.uint64)
    off2 = np.zeros(n + 1, np.uint64)
    off1[1:] = np.cumsum(rng.integers(0, 5, n))
    off2[1:] = np.cumsum(rng.integers(0, 5, n))
    cat1 = rng.integers(0, 256, int(off1[-1]) + 16, dtype=np.uint8) & np.uint8(0xE3)      # letters 0 - 3, junk above
    cat2 = rng.integers(0, 256, int(off2[-1]) + 16, dtype=np.uint8) & np.uint8(0xE3)
    assert wide.slices_for(off1, off2, traceback=False) == [1 << 20, 5]
    sm = scoring_matrix(13)
    P = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0), (GLOBAL, 15)):
        want_sc = np.zeros(n, np.int32)
        want_ends = np.zeros((n, 4), np.int32)
        assert woracle.lib.wide_affine_oracle_ragged(kind, P(cat1), P(off1), P(cat2), P(off2), ctypes.c_size_t(n), P(np.ascontiguousarray(sm)), 3, 1, mask,
                                                     P(want_sc), P(want_ends), None, None, None) == 0
        sc, ends, moves, mo, steps = _run(wide, kind, (cat1, off1), (cat2, off2), sm, (3, 1), mask, False)
        assert moves is None and mo is None and steps is None
        assert np.array_equal(sc, want_sc) and np.array_equal(ends, want_ends), (kind, mask)
        assert want_sc.max() > 0 and (kind == LOCAL or mask or want_sc.min() < 0)


def test_cpp_overloads_on_a_mixed_batch(wide, woracle, swmi_mod, tmp_path):
    """tests/native/compat_wide.cpp, built by g++ against both libraries: 40 mixed alignments in pieces of 16, (0, 5), (5, 0)
    and (700, 2049) among them; it prints score, path length, start cell, end cell and a path checksum, which the restatement
    confirms."""
    assert shutil.which("g++") is not None
    rng = np.random.default_rng(61)
    shapes = [(int(x), int(y)) for x, y in rng.integers(0, 1300, (36, 2))] + [(0, 5), (5, 0), (700, 2049), (1, 1)]
    a, b = inputs(shapes, 62)
    sm = scoring_matrix(15)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.ascontiguousarray(sm, np.int8).tobytes())
        fh.write(np.int32(len(a)).tobytes())
        for x, y in zip(a, b):
            fh.write(np.int32([len(x), len(y)]).tobytes() + x.tobytes() + y.tobytes())
    exe = str(tmp_path / "compat_wide")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "compat_wide.cpp"),
                            "-o", exe, "-L", lib, "-lswmi_wide", "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
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
            path = swmi_mod.local_full_expand_moves(row, steps[k], ends[k, 0], ends[k, 1]) if steps[k] else ends[k, 2:].reshape(1, 2)
            assert rows[at + k] == (int(sc[k]), int(steps[k]) + 1, int(ends[k, 2]), int(ends[k, 3]), int(ends[k, 0]), int(ends[k, 1]),
                                    checksum(path)), (at, k)
        at += len(a)
