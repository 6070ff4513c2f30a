"""The affine local aligner (swmi_local_align_affine*, include/swmi.h) without a device: the C restatement
tests/native/local_affine_oracle.c against an independent numpy formulation, against the linear restatement at
open = extend and against fixture F7 (the reference's SmithWaterman_111_long) at (1, -1, 1, 1); three hand-checked
alignments; and the library's slicing rule, argument and domain errors, no-op and C++ header."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle, gotoh_numpy, hand_cases, moves_as_letters, runs
from local_support import PARAMS, LocalOracle, f7_by_length, move_words, moves_to_path

NEW_SYMBOLS = ("swmi_local_align_affine", "swmi_local_align_affine_device", "swmi_local_affine_slices_for",
               "swmi_local_affine_time_device")


@pytest.fixture(scope="module")
def aoracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


@pytest.mark.parametrize("gaps", AFFINE_GAPS)
def test_restatement_equals_numpy_gotoh(aoracle, golden, gaps):
    """Every F1 matrix crossed with the (open, extend) grid, on small random sizes and on F1's own pairs cut short."""
    f = golden("f1_random")
    rng = np.random.default_rng(sum(gaps) * 31 + gaps[0])
    for p in range(len(f["gap"])):
        for len1 in (1, int(rng.integers(2, 12)), int(rng.integers(12, 40))):
            a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
            b = rng.integers(0, 4, (2, 128), dtype=np.uint8)
            a[1] = f["seq1"][p, :len1]            # a related pair from the fixture
            b[1] = f["seq2"][p]
            sc, ends, moves, steps = aoracle.align(a, b, f["sm"][p], *gaps)
            for k in range(2):
                score, cells, letters = gotoh_numpy(a[k], b[k], f["sm"][p], *gaps)
                assert sc[k] == score, (gaps, p, len1, k)
                assert tuple(ends[k]) == cells, (gaps, p, len1, k)
                assert moves_as_letters(moves[k], steps[k]) == letters, (gaps, p, len1, k)


@pytest.mark.parametrize("p", range(len(PARAMS)))
def test_open_equal_extend_is_the_linear_aligner(aoracle, loracle, p):
    """open = extend = g: every field equals the linear restatement's, for every F7 input."""
    match, mismatch, g = PARAMS[p]
    sm = match_matrix(match, mismatch)
    for len1, (a, b, _, _) in f7_by_length().items():
        want = loracle.align(a, b, sm, g)
        got = aoracle.align(a, b, sm, g, g)
        for x, y in zip(got[:2] + got[3:], want[:2] + want[3:]):
            assert np.array_equal(x, y), (p, len1)
        for k in range(len(a)):
            words = (int(want[3][k]) + 31) // 32
            assert np.array_equal(got[2][k, :words], want[2][k, :words]), (p, len1, k)


def test_reproduces_f7_at_open_equal_extend_one(aoracle):
    """The reference's own SmithWaterman_111_long answers: score, end cell, start cell and the whole path."""
    for len1, (a, b, scores, paths) in f7_by_length().items():
        sc, ends, moves, steps = aoracle.align(a, b, match_matrix(1, -1), 1, 1)
        for k in range(len(scores)):
            want = paths[k]
            assert sc[k] == scores[k], (len1, k)
            assert tuple(ends[k, :2]) == tuple(want[-1]) and tuple(ends[k, 2:]) == tuple(want[0]), (len1, k)
            assert np.array_equal(moves_to_path(moves[k], steps[k], ends[k, 0], ends[k, 1]), want), (len1, k)


def test_hand_checked_cases(aoracle):
    want_runs = {"deletion10": ("L", 10), "left100": ("L", 100), "up3000": ("U", 3000)}
    for name, a, b, sm, go, ge, score in hand_cases():
        sc, ends, moves, steps = aoracle.align(a, b, sm, go, ge)
        assert sc[0] == score, name
        r = runs(moves_as_letters(moves[0], steps[0]))
        gaps = [x for x in r if x[0] != "D"]
        assert gaps == [want_runs[name]], (name, r)
        if name == "deletion10":
            assert tuple(ends[0]) == (118, 128, 0, 0)
            assert sum(x[1] for x in r if x[0] == "D") == 118
        if name == "left100":
            assert tuple(ends[0]) == (28, 128, 0, 0)


def test_every_new_symbol_is_declared_and_exported():
    import re
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def _per_alignment(len1, traceback):
    per = len1 + 128 + 4 + 16
    if traceback:
        per += 4 * 128 * ((len1 + 15 + 7) // 8) + 8 * move_words(len1) + 4
    return per


@pytest.mark.parametrize("len1", [1, 128, 1000, 16384])
@pytest.mark.parametrize("traceback", [True, False])
def test_slices_cover_every_alignment_within_the_bound(swmi_mod, len1, traceback):
    bound = 4096 * _per_alignment(16384, True) if traceback else 256 << 20
    per = _per_alignment(len1, traceback)
    for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
        sizes = swmi_mod.local_affine_slices_for(n, len1, traceback)
        assert sum(sizes) == n and all(s >= 1 for s in sizes)
        assert all(s * per <= bound and s <= 1 << 20 for s in sizes)
        assert all(s == sizes[0] for s in sizes[:-1]) and (not sizes or sizes[-1] <= sizes[0])
    assert swmi_mod.local_affine_slices_for(10, 0) == [] and swmi_mod.local_affine_slices_for(10, 16385) == []


def test_a_full_length_traceback_slice_gives_every_cu_a_workgroup(swmi_mod):
    sizes = swmi_mod.local_affine_slices_for(10000, 16384, True)
    assert sizes == [4096, 4096, 1808]                       # 256 CUs x 16 alignments per workgroup
    assert 4096 * _per_alignment(16384, True) < 4.2 * (1 << 30)
    per128 = 4096 * _per_alignment(16384, True) // _per_alignment(128, True)
    assert swmi_mod.local_affine_slices_for(1 << 20, 128, True)[0] == per128
    assert swmi_mod.local_affine_slices_for(3 << 20, 1, True)[0] == 1 << 20
    assert len(swmi_mod.local_affine_slices_for(600, 16384, False)) == 1


def test_argument_and_domain_errors_without_a_device(swmi_mod):
    lib = swmi_mod.load()
    sm = match_matrix(1, -1)
    a = np.zeros((2, 128), np.uint8)
    b = np.zeros((2, 128), np.uint8)
    sc = np.zeros(2, np.int32)
    ends = np.zeros((2, 4), np.int32)
    mv = np.zeros((2, move_words(128)), np.uint64)
    st = np.zeros(2, np.uint32)
    P = lambda x: x.ctypes.data  # noqa: E731

    def call(len1=128, s1=P(a), s2=P(b), go=5, ge=2, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_local_align_affine(s1, len1, s2, n, m, go, ge, scores, e, moves, steps)
    INV, DOM = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN
    assert call(len1=0) == INV and call(len1=16385) == INV
    for go, ge in ((-1, 0), (0, -1), (128, 0), (0, 128), (1000, 1)):
        assert call(go=go, ge=ge) == DOM, (go, ge)
    assert b"gap_open" in lib.swmi_last_error()
    for kw in ("s1", "s2", "m", "scores", "e"):
        assert call(**{kw: None}) == INV, kw
    assert call(steps=None) == INV and call(moves=None) == INV          # only one of moves / steps
    assert call(n=0, s1=None, s2=None, scores=None, e=None) == swmi_mod.OK
    assert call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, steps=None) == swmi_mod.OK
    dev = lib.swmi_local_align_affine_device
    assert dev(P(a), 0, P(b), 2, P(sm), 1, 1, P(sc), P(ends), None, None, None) == INV
    assert dev(P(a), 128, P(b), 2, P(sm), 128, 1, P(sc), P(ends), None, None, None) == DOM
    assert dev(P(a), 128, P(b), 2, P(sm), 1, -2, P(sc), P(ends), None, None, None) == DOM
    assert dev(P(a), 128, P(b), 2, P(sm), 1, 1, P(sc), P(ends), P(mv), None, None) == INV
    assert dev(None, 128, None, 0, P(sm), 1, 1, None, None, None, None, None) == swmi_mod.OK
    ms = ctypes.c_float()
    assert lib.swmi_local_affine_time_device(P(a), 128, P(b), 2, P(sm), 1, 1, P(sc), P(ends), None, None, None, 1, None) == INV
    assert lib.swmi_local_affine_time_device(P(a), 128, P(b), 0, P(sm), 1, 1, P(sc), P(ends), None, None, None, 1,
                                             ctypes.byref(ms)) == INV
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_align_affine(a, b, sm, 300, 1)
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_affine.cpp"), "-o", str(tmp_path / "compat_affine"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
