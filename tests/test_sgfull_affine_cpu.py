"""The affine exact semi-global aligner (swmi_semiglobal_full_affine*, include/swmi.h) without a device: the C restatement
tests/native/sgfull_affine_oracle.c against an independent numpy Gotoh, against the linear restatement at open = extend and
against fixture F8 (the reference's SemiGlobal_111) at (1, -1, 1, 1); hand-checked gap runs; the slicing rule; the C ABI
surface and its argument errors; the C++ header."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS, moves_as_letters, runs
from local_support import PARAMS
from sgfull_affine_support import SgAffineOracle, gotoh_numpy, hand_cases, per_alignment
from sgfull_support import K111, SgFullOracle, load_f8, move_words, moves_to_path

NEW_SYMBOLS = ("swmi_semiglobal_full_affine", "swmi_semiglobal_full_affine_device", "swmi_semiglobal_full_affine_slices_for",
               "swmi_semiglobal_full_affine_time_device", "swmi_semiglobal_full_affine_release_workspaces")


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_affine_oracle"))


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


@pytest.mark.parametrize("gaps", AFFINE_GAPS)
def test_restatement_equals_numpy_gotoh(aoracle, golden, gaps):
    """Every F1 matrix crossed with the (open, extend) grid on small random sizes, one pair of each size related."""
    f = golden("f1_random")
    rng = np.random.default_rng(sum(gaps) * 37 + gaps[0])
    for p in range(len(f["gap"])):
        for len1, len2 in ((1, 1), (1, int(rng.integers(2, 9))), (int(rng.integers(2, 9)), 1), (int(rng.integers(5, 30)), int(rng.integers(5, 30)))):
            a = rng.integers(0, 4, (3, len1), dtype=np.uint8)
            b = rng.integers(0, 4, (3, len2), dtype=np.uint8)
            w = min(len1, len2)
            a[1, :w] = f["seq1"][p, :w]
            b[1, :w] = f["seq1"][p, :w]                   # a similar pair
            a[2] = 0
            b[2, : len2 // 2] = 0                          # ties
            sc, ends, moves, lengths = aoracle.align(a, b, f["sm"][p], *gaps)
            sc2, ends2, _, _ = aoracle.align(a, b, f["sm"][p], *gaps, traceback=False)
            assert np.array_equal(sc, sc2) and np.array_equal(ends, ends2)
            for k in range(3):
                score, cell, letters = gotoh_numpy(a[k], b[k], f["sm"][p], *gaps)
                what = (gaps, p, len1, len2, k)
                assert sc[k] == score and tuple(ends[k]) == cell, what
                assert lengths[k] == len(letters) + 1, what
                assert moves_as_letters(moves[k], lengths[k] - 1) == letters, what


@pytest.mark.parametrize("p", range(len(PARAMS)))
def test_open_equal_extend_is_the_linear_aligner(aoracle, sgoracle, p):
    """open = extend = g: every field equals the linear restatement's (tests/native/sgfull_oracle.c)."""
    match, mismatch, g = PARAMS[p]
    sm = match_matrix(match, mismatch)
    rng = np.random.default_rng(p)
    for len1, len2 in ((1, 1), (7, 300), (300, 7), (129, 131), (600, 500)):
        a = rng.integers(0, 4, (8, len1), dtype=np.uint8)
        b = rng.integers(0, 4, (8, len2), dtype=np.uint8)
        w = min(len1, len2)
        b[::2, :w] = np.where(rng.random((4, w)) < 0.85, a[::2, :w], b[::2, :w])
        want = sgoracle.align(a, b, sm, g)
        got = aoracle.align(a, b, sm, g, g)
        for x, y in zip(got[:2] + got[3:], want[:2] + want[3:]):
            assert np.array_equal(x, y), (p, len1, len2)
        for k in range(len(a)):
            assert moves_as_letters(got[2][k], got[3][k] - 1) == moves_as_letters(want[2][k], want[3][k] - 1), (p, len1, len2, k)


def test_restatement_reproduces_f8_at_one_one(aoracle):
    """(1, -1) with open = extend = 1 is SemiGlobal_111: F8's scores, best cells, lengths and whole paths."""
    f8 = load_f8()
    sc, ends, moves, lengths = aoracle.align(f8["seq1"], f8["seq2"], K111, 1, 1)
    for k in range(len(f8["scores"])):
        assert sc[k] == f8["scores"][k], k
        assert tuple(ends[k]) == tuple(f8["ends"][k]) == tuple(f8["paths"][k][-1]), k
        assert lengths[k] == f8["lengths"][k] == len(f8["paths"][k]), k
        assert np.array_equal(moves_to_path(moves[k], lengths[k], ends[k, 0], ends[k, 1]), f8["paths"][k]), k


def test_hand_checked_cases(aoracle):
    """One deletion and one insertion of 100 bases at open 10, extend 1: one gap run of 100, charged 10 + 99."""
    for name, a, b, sm, go, ge, score, cell, run in hand_cases():
        sc, ends, moves, lengths = aoracle.align(a, b, sm, go, ge)
        assert sc[0] == score and tuple(ends[0]) == cell, name
        letters = moves_as_letters(moves[0], lengths[0] - 1)
        assert [r for r in runs(letters) if r[0] != "D"] == [run], (name, runs(letters))
        assert gotoh_numpy(a[0], b[0], sm, go, ge) == (score, cell, letters), name
        # the linear model charges every base of the run: the same pair scores 100 * 10 - 109 lower at gap 10
        lin = aoracle.align(a, b, sm, go, go)[0][0]
        assert lin < score, name


def test_all_mismatch_and_identical(aoracle):
    rng = np.random.default_rng(5)
    sm = match_matrix(3, -2)
    a = np.zeros((1, 200), np.uint8)
    b = np.ones((1, 300), np.uint8)
    sc, ends, _, lengths = aoracle.align(a, b, sm, 4, 1)
    assert sc[0] == 0 and tuple(ends[0]) == (0, 0) and lengths[0] == 1
    x = rng.integers(0, 4, (1, 257), dtype=np.uint8)
    sc, ends, moves, lengths = aoracle.align(x, x, sm, 4, 1)
    assert sc[0] == 3 * 257 and tuple(ends[0]) == (257, 257) and lengths[0] == 258
    assert moves_as_letters(moves[0], 257) == ["D"] * 257


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name


@pytest.mark.parametrize("len1,len2", [(1, 1), (1000, 1000), (16384, 1), (4096, 777), (16384, 16384)])
@pytest.mark.parametrize("traceback", [True, False])
def test_slices_cover_every_alignment_within_the_bound(swmi_mod, len1, len2, traceback):
    bound = 256 * per_alignment(16384, 16384, True) if traceback else 256 << 20
    per = per_alignment(len1, len2, traceback)
    for n in (0, 1, 3, 257, 1 << 20, 3 * (1 << 20) + 5):
        sizes = swmi_mod.semiglobal_full_affine_slices_for(n, len1, len2, traceback)
        assert sum(sizes) == n and all(s >= 1 for s in sizes)
        assert all(s * per <= bound and s <= 1 << 20 for s in sizes)
        assert all(s == sizes[0] for s in sizes[:-1]) and (not sizes or sizes[-1] <= sizes[0])
    for bad in ((0, 5), (5, 0), (16385, 5), (5, 16385)):
        assert swmi_mod.semiglobal_full_affine_slices_for(10, *bad) == []


def test_a_full_size_traceback_slice_gives_every_cu_a_workgroup(swmi_mod):
    assert swmi_mod.semiglobal_full_affine_slices_for(600, 16384, 16384, True) == [256, 256, 88]
    assert 256 * per_alignment(16384, 16384, True) < 32.2 * (1 << 30)         # about 32.1 GiB
    assert swmi_mod.semiglobal_full_affine_slices_for(3 << 20, 1, 1, True)[0] == 1 << 20
    assert swmi_mod.semiglobal_full_affine_slices_for(3 << 20, 1, 1, False)[0] == 1 << 20
    assert swmi_mod.semiglobal_full_affine_slices_for(9000, 16384, 16384, False)[0] == (256 << 20) // per_alignment(16384, 16384, False)


def test_argument_and_domain_errors_without_a_device(swmi_mod):
    lib = swmi_mod.load()
    sm = match_matrix(1, -1)
    a = np.zeros((2, 100), np.uint8)
    b = np.zeros((2, 70), np.uint8)
    sc = np.zeros(2, np.int32)
    ends = np.zeros((2, 2), np.int32)
    mv = np.zeros((2, move_words(100, 70)), np.uint64)
    ln = np.zeros(2, np.uint32)
    P = lambda x: x.ctypes.data  # noqa: E731

    def call(len1=100, len2=70, s1=P(a), s2=P(b), go=5, ge=2, moves=P(mv), lengths=P(ln), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_semiglobal_full_affine(s1, len1, s2, len2, n, m, go, ge, scores, e, moves, lengths)
    INV, DOM = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN
    for l1, l2 in ((0, 70), (100, 0), (16385, 70), (100, 16385)):
        assert call(len1=l1, len2=l2) == INV, (l1, l2)
    for go, ge in ((-1, 0), (0, -1), (128, 0), (0, 128), (1000, 1)):
        assert call(go=go, ge=ge) == DOM, (go, ge)
    assert b"gap_open" in lib.swmi_last_error()
    for kw in ("s1", "s2", "m", "scores", "e"):
        assert call(**{kw: None}) == INV, kw
    assert call(lengths=None) == INV and call(moves=None) == INV          # only one of moves / lengths
    assert call(n=0, s1=None, s2=None, scores=None, e=None) == swmi_mod.OK
    assert call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, lengths=None) == swmi_mod.OK
    dev = lib.swmi_semiglobal_full_affine_device
    assert dev(P(a), 0, P(b), 70, 2, P(sm), 1, 1, P(sc), P(ends), None, None, None) == INV
    assert dev(P(a), 100, P(b), 16385, 2, P(sm), 1, 1, P(sc), P(ends), None, None, None) == INV
    assert dev(P(a), 100, P(b), 70, 2, P(sm), 128, 1, P(sc), P(ends), None, None, None) == DOM
    assert dev(P(a), 100, P(b), 70, 2, P(sm), 1, -2, P(sc), P(ends), None, None, None) == DOM
    assert dev(P(a), 100, P(b), 70, 2, P(sm), 1, 1, P(sc), P(ends), P(mv), None, None) == INV
    assert dev(None, 100, None, 70, 0, P(sm), 1, 1, None, None, None, None, None) == swmi_mod.OK
    ms = ctypes.c_float()
    timer = lib.swmi_semiglobal_full_affine_time_device
    assert timer(P(a), 100, P(b), 70, 2, P(sm), 1, 1, P(sc), P(ends), None, None, None, 1, None) == INV
    assert timer(P(a), 100, P(b), 70, 0, P(sm), 1, 1, P(sc), P(ends), None, None, None, 1, ctypes.byref(ms)) == INV
    assert timer(P(a), 100, P(b), 70, 2, P(sm), 1, 200, P(sc), P(ends), None, None, None, 1, ctypes.byref(ms)) == DOM
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.semiglobal_full_affine(a, b, sm, 300, 1)
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)
        assert lib.swmi_semiglobal_full_affine_release_workspaces() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_sgfull_affine.cpp"), "-o", str(tmp_path / "compat"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
