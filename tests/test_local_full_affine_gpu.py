"""The any-length affine local aligner (swmi_local_full_affine*) on the GPU, every field bit-exact against the C restatement
tests/native/local_full_affine_oracle.c (which test_local_full_affine_cpu.py ties to fixture F7, to the 128-column affine
restatement, to the linear any-length restatement and to numpy), with a traceback and ends-only, through the host entry and
the device entry.  Moves are compared up to `steps`; words past it are unspecified.

The length grid and the hand-built edges come from local_full_affine_edges.py, which derives them from the kernel's constants
(local_full_affine_kernels.hip); test_local_full_affine_edges_cpu.py checks every expected field and every claimed edge of
them without a device."""
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

import affine_edges as ae
import local_full_affine_edges as lfe
from conftest import PKG, ROOT, match_matrix
from local_full_affine_support import LocalFullAffineOracle, assert_same, check_path, inputs, moves_of, path_from
from local_affine_support import AFFINE_GAPS
from local_support import PARAMS, f7_by_length, random_matrix

pytestmark = pytest.mark.gpu

K111 = match_matrix(1, -1)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LocalFullAffineOracle(tmp_path_factory.mktemp("local_full_affine_oracle"))


def _device(gpu, a, b, sm, go, ge, traceback=True):
    """the device entry on torch buffers, synchronised: (scores, ends, moves, steps) as numpy"""
    dev = torch.device("cuda:0")
    n, len1 = a.shape
    len2 = b.shape[1]
    mw = gpu.local_full_move_words(len1, len2)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    ends = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv = torch.zeros((n, mw), dtype=torch.int64, device=dev) if traceback else None
    st = torch.zeros(n, dtype=torch.int32, device=dev) if traceback else None
    torch.cuda.synchronize()
    gpu.local_full_affine_device(ta.data_ptr(), len1, tb.data_ptr(), len2, n, sm, go, ge, sc.data_ptr(), ends.data_ptr(),
                                 mv.data_ptr() if traceback else None, st.data_ptr() if traceback else None)
    torch.cuda.synchronize()
    return (sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64) if traceback else None,
            st.cpu().numpy().view(np.uint32) if traceback else None)


def _both(gpu, oracle, a, b, sm, go, ge, what, device=False):
    """The host entry (and, device=True, the device entry) with traceback and ends-only against the restatement; returns the
    restatement's results."""
    want = oracle.align(a, b, sm, go, ge)
    assert_same(gpu.local_full_affine(a, b, sm, go, ge), want, what)
    sc, ends, mv, st = gpu.local_full_affine(a, b, sm, go, ge, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    if device:
        assert_same(_device(gpu, a, b, sm, go, ge), want, (what, "device"))
        assert_same(_device(gpu, a, b, sm, go, ge, traceback=False), want, (what, "device ends-only"), traceback=False)
    return want


# ---- 1. identities across entries, on the same inputs ------------------------------------------------------------------------

def test_f7_at_open_equal_extend_equal_1(gpu):
    for len1, (a, b, f7_scores, f7_paths) in f7_by_length().items():
        sc, ends, mv, st = gpu.local_full_affine(a, b, K111, 1, 1)
        assert np.array_equal(sc, f7_scores), len1
        for k, path in enumerate(f7_paths):
            assert st[k] == len(path) - 1 and tuple(ends[k]) == (*path[-1], *path[0]), (len1, k)
            assert np.array_equal(gpu.local_full_expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1]), path), (len1, k)


def test_every_field_equals_local_align_affine_at_128_columns(gpu):
    for len1, (a, b, _, _) in f7_by_length().items():
        for p, (m, x, _) in enumerate(PARAMS):
            sm = match_matrix(m, x)
            for go, ge in AFFINE_GAPS:
                assert_same(gpu.local_full_affine(a, b, sm, go, ge), gpu.local_align_affine(a, b, sm, go, ge), (len1, p, go, ge))
                sc, ends, _, _ = gpu.local_full_affine(a, b, sm, go, ge, traceback=False)
                wsc, wends, _, _ = gpu.local_align_affine(a, b, sm, go, ge, traceback=False)
                assert np.array_equal(sc, wsc) and np.array_equal(ends, wends), (len1, p, go, ge)


@pytest.mark.parametrize("len1,len2", [(700, 2100), (2100, 700), (129, 1025), (3000, 5000)])
def test_every_field_equals_local_full_at_open_equal_extend(gpu, len1, len2):
    a, b = inputs(12, len1, len2, len1 + 3 * len2)
    for p, (sm, g) in enumerate([(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(), 3)]):
        assert_same(gpu.local_full_affine(a, b, sm, g, g), gpu.local_full(a, b, sm, g), (len1, len2, p))
        sc, ends, _, _ = gpu.local_full_affine(a, b, sm, g, g, traceback=False)
        wsc, wends, _, _ = gpu.local_full(a, b, sm, g, traceback=False)
        assert np.array_equal(sc, wsc) and np.array_equal(ends, wends), (len1, len2, p)


# ---- 2. the length grid -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", lfe.shape_grid())
def test_length_grid_across_parameter_sets(gpu, oracle, len1, len2):
    full = len1 == lfe.MAX_LEN and len2 == lfe.MAX_LEN
    index = lfe.shape_grid().index((len1, len2))
    n = 2 if full else 12
    for p, (sm, go, ge) in enumerate(lfe.grid_params(index)):
        if full and p not in (0, 1, 2):
            continue                                    # at 16384 x 16384: the three gap families
        a, b = inputs(n, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        sc, ends, mv, st = _both(gpu, oracle, a, b, sm, go, ge, (len1, len2, p, go, ge), device=p < 3)
        if len2 > lfe.WAVE_COLS and len1 >= lfe.WAVE_COLS:
            # the inputs must not let the grid pass on trivial walks: a planted pair's path crosses a wavefront's first column
            # and some path is longer than a staging block is wide (so higher, too)
            lfe.assert_grid_edges(sc, ends, st, (len1, len2, p))
        for k in range(0, n, 5):
            check_path(a[k], b[k], sm, go, ge, sc[k], ends[k], mv[k], st[k])


# ---- 3. hand-built edges ------------------------------------------------------------------------------------------------------

def _expect(gpu, oracle, h):
    """one hand-built alignment: the worked-out score, ends and (where pinned) move codes against the GPU, through both
    entries, beside the restatement's"""
    want = _both(gpu, oracle, h.a, h.b, h.sm, h.gap_open, h.gap_extend, h, device=True)
    for name, (sc, e, mv, st) in (("restatement", want), ("gpu", gpu.local_full_affine(h.a, h.b, h.sm, h.gap_open, h.gap_extend))):
        assert sc[0] == h.score and tuple(e[0]) == h.ends, (h, name, sc[0], e[0], st[0])
        if h.codes is not None:
            assert st[0] == len(h.codes) and np.array_equal(moves_of(mv[0], st[0]), np.asarray(h.codes, np.int64)), (h, name)
    sc, e, _, _ = gpu.local_full_affine(h.a, h.b, h.sm, h.gap_open, h.gap_extend, traceback=False)
    assert sc[0] == h.score and tuple(e[0]) == (h.ends[0], h.ends[1], -1, -1), h


@pytest.mark.parametrize("group", sorted(lfe.hand_groups()))
def test_hand_built_edges(gpu, oracle, group):
    for h in lfe.hand_groups()[group]():
        _expect(gpu, oracle, h)


def test_all_mismatch_pair(gpu, oracle):
    for len1, len2 in ((300, 2000), (1, 1), (130, 1025)):
        a, b = np.zeros((1, len1), np.uint8), np.ones((1, len2), np.uint8)
        for sm, go, ge in ((K111, 3, 1), (lfe.K54, 0, 0), (lfe.K54, 0, 9)):
            _expect(gpu, oracle, lfe.Hand("mismatch", a, b, sm, go, ge, 0, (0, 0, 0, 0), []))


def test_path_ties_beyond_column_128_and_across_a_wave_edge(gpu, oracle):
    """section 14's ties between two candidates of a path cell (and the floor's two), in columns 961 .. 1088: the small
    pairs' results shifted by the columns in front of them"""
    for shifted, small in lfe.shifted_path_tie_cases():
        c0 = shifted.b.shape[1] - small.b.shape[1]
        got = gpu.local_full_affine(shifted.a, shifted.b, shifted.sm, *shifted.gaps)
        assert_same(got, oracle.align(shifted.a, shifted.b, shifted.sm, *shifted.gaps), shifted)
        sc, ends, mv, st = gpu.local_align_affine(small.a, small.b, small.sm, *small.gaps)
        moved = ends + np.where(sc > 0, c0, 0)[:, None] * np.array([0, 1, 0, 1], np.int32)
        assert np.array_equal(got[0], sc) and np.array_equal(got[1], moved) and np.array_equal(got[3], st), shifted
        for k in range(len(sc)):
            assert np.array_equal(moves_of(got[2][k], got[3][k]), moves_of(mv[k], st[k])), (shifted, k)
        assert_same(_device(gpu, shifted.a, shifted.b, shifted.sm, *shifted.gaps), got, (shifted, "device"))


def test_the_extremes_at_full_size(gpu, oracle):
    """16384 x 16384 at the bounds the keys are argued from, on an identical, a shifted and a random pair"""
    a, b = ae.te._pair_kinds(3, lfe.MAX_LEN, lfe.MAX_LEN, 28800)
    for name, sm, go, ge in ae.EXTREME_PARAMS:
        want = _both(gpu, oracle, a, b, sm, go, ge, name)
        if name.startswith("diag+127"):                  # the identical pair: 16384 matches of 127
            assert want[0][0] == 127 * 16384 == 2080768 and tuple(want[1][0]) == (16384, 16384, 0, 0) and want[3][0] == 16384
            assert np.all(moves_of(want[2][0], want[3][0]) == lfe.DIAG)
        if name.startswith("all-128"):
            assert np.all(want[0] == 0) and np.all(want[1] == 0) and np.all(want[3] == 0)


def test_bytes_are_taken_modulo_4(gpu):
    a, b = inputs(9, 300, 1500, 44)
    rng = np.random.default_rng(45)
    a2 = (a | (rng.integers(0, 64, a.shape) << 2)).astype(np.uint8)
    b2 = (b | (rng.integers(0, 64, b.shape) << 2)).astype(np.uint8)
    assert a2.max() > 250 and b2.max() > 250 and a2.min() == 0
    sm = random_matrix()
    assert_same(gpu.local_full_affine(a2, b2, sm, 6, 2), gpu.local_full_affine(a, b, sm, 6, 2), "modulo 4")


# ---- 4. batch sizes and slices --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256])
def test_batch_sizes(gpu, oracle, n):
    a, b = inputs(n, 700, 2100, n)
    sm = match_matrix(2, -3)
    assert_same(gpu.local_full_affine(a, b, sm, 7, 1), oracle.align(a, b, sm, 7, 1), n)


def test_batch_across_a_slice_boundary(gpu, oracle):
    """257 alignments of 16384 x 16384 with traceback: two slices (256 + 1) on the host entry's two buffer sets."""
    n = 257
    assert gpu.local_full_affine_slices_for(n, 16384, 16384) == [256, 1]
    a, b = inputs(n, 16384, 16384, 257)
    got = gpu.local_full_affine(a, b, K111, 4, 1)
    gpu.local_full_affine_release_workspaces()
    assert_same(got, oracle.align(a, b, K111, 4, 1), "slices")


# ---- 5. streams and threads -----------------------------------------------------------------------------------------------------

def test_device_entry_on_two_streams(gpu):
    """two calls on two streams issued before either is waited for, each equal to the host entry; one traceback, one
    ends-only; then the timer"""
    dev = torch.device("cuda:0")
    jobs = []
    for len1, len2, n, seed, tb in ((3000, 5000, 40, 1, True), (1023, 16384, 9, 2, False)):
        a, b = inputs(n, len1, len2, seed)
        mw = gpu.local_full_move_words(len1, len2)
        t = dict(a=torch.from_numpy(a).to(dev), b=torch.from_numpy(b).to(dev), sc=torch.zeros(n, dtype=torch.int32, device=dev),
                 ends=torch.zeros((n, 4), dtype=torch.int32, device=dev), mv=torch.zeros((n, mw), dtype=torch.int64, device=dev),
                 st=torch.zeros(n, dtype=torch.int32, device=dev))
        jobs.append((len1, len2, n, a, b, t, tb, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize()
    sm = random_matrix(5)
    for len1, len2, n, a, b, t, tb, s in jobs:
        gpu.local_full_affine_device(t["a"].data_ptr(), len1, t["b"].data_ptr(), len2, n, sm, 9, 2, t["sc"].data_ptr(),
                                     t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None,
                                     stream=s.cuda_stream)
    for len1, len2, n, a, b, t, tb, s in jobs:
        s.synchronize()
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64),
               t["st"].cpu().numpy().view(np.uint32))
        assert_same(got, gpu.local_full_affine(a, b, sm, 9, 2), ("device", len1, len2), traceback=tb)
    t = jobs[0][5]
    ms = gpu.local_full_affine_time_device(t["a"].data_ptr(), 3000, t["b"].data_ptr(), 5000, 40, sm, 9, 2, t["sc"].data_ptr(),
                                           t["ends"].data_ptr(), iters=2)
    assert ms > 0


def test_host_entry_from_two_threads(gpu, oracle):
    a, b = inputs(300, 900, 1500, 9)
    sm = match_matrix(5, -4)
    want = oracle.align(a, b, sm, 8, 0)
    out = [None, None]

    def run(k):
        gpu.use_gpu(0)
        out[k] = gpu.local_full_affine(a, b, sm, 8, 0)
    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert_same(out[k], want, k)


# ---- 6. the C++ overloads -------------------------------------------------------------------------------------------------------

def _checksum(path):
    want = 0
    for i, j in path:
        want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
    return want


def _run_compat(exe, tmp_path, name, a, b, sm, go, ge, piece):
    data = tmp_path / name
    with open(data, "wb") as fh:
        fh.write(np.array([a.shape[0], a.shape[1], b.shape[1], go, ge], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(a.shape[0]):
            fh.write(a[k].tobytes() + b[k].tobytes())
    run = subprocess.run([exe, str(data), str(piece)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-3:] == ["single 0", "ragged 1", "linear 0"], lines[-3:]
    rows = [tuple(map(int, line.split())) for line in lines[:-3]]
    assert len(rows) == a.shape[0]
    return rows


def test_cpp_overloads(gpu, tmp_path):
    """single and batch overloads against the C entry, in pieces of 3 and in one piece"""
    assert shutil.which("g++") is not None
    exe = str(tmp_path / "compat_local_full_affine")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local_full_affine.cpp"), "-o", exe, "-L", lib, "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a, b = inputs(10, 1200, 2300, 71)
    sm = random_matrix()
    sc, ends, mv, st = gpu.local_full_affine(a, b, sm, 6, 1)
    for piece in (3, 0):
        rows = _run_compat(exe, tmp_path, "long%d.bin" % piece, a, b, sm, 6, 1, piece)
        for k in range(10):
            path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), _checksum(path)), (piece, k)


# ---- 7. a seeded fuzz -----------------------------------------------------------------------------------------------------------

def test_seeded_fuzz(gpu, oracle):
    """about 20000 alignments: 180 batches of 100 of small random shapes, 20 of 40 to 100 of larger ones, every parameter drawn"""
    rng = np.random.default_rng(20240)
    total = 0
    for t in range(200):
        small = t < 180
        len1, len2 = (int(x) for x in (rng.integers(1, 300, 2) if small else rng.integers(300, 3000, 2)))
        if t % 10 == 3:
            len2 = int(rng.choice([1023, 1024, 1025, 2048, 2049])) if small else len2
        n = 100 if small else int(rng.integers(40, 101))
        kind = t % 4
        sm = (rng.integers(-128, 128, 16) if kind == 0 else rng.integers(-6, 7, 16) if kind == 1 else
              match_matrix(int(rng.integers(1, 20)), -int(rng.integers(0, 20)))).astype(np.int8)
        go, ge = (int(x) for x in rng.integers(0, 128, 2)) if t % 5 == 0 else (int(x) for x in rng.integers(0, 12, 2))
        a, b = inputs(n, len1, len2, 7000 + t)
        if t % 3 == 0:                                  # a small alphabet: ties
            a, b = a & 1, b & 1
        want = oracle.align(a, b, sm, go, ge)
        assert_same(gpu.local_full_affine(a, b, sm, go, ge), want, (t, len1, len2, go, ge, sm.tolist()))
        if t % 4 == 0:
            assert_same(_device(gpu, a, b, sm, go, ge, traceback=False), want, (t, "ends-only"), traceback=False)
        total += n
    assert total >= 19000
