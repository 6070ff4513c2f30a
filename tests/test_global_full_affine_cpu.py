"""The affine global / free-end-gap aligner (swmi_global_full_affine*, include/swmi.h) without a device: the C restatement
tests/native/global_full_affine_oracle.c against an independent numpy/Python three-matrix formulation under all 16 masks,
against the linear restatement (global_full_oracle.c) at open = extend, and against the affine exact semi-global
restatement (sgfull_affine_oracle.c) by the mask-0 prefix identity; properties of the masks and the gap costs; the C ABI
surface, its argument errors and slices; the Python submodule; the C++ header."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from global_full_affine_support import (ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullAffineOracle, check_path,
                                        move_words, moves_of, numpy_global_full_affine, path_from, related_pairs)
from global_full_support import GlobalFullOracle
from local_affine_support import AFFINE_GAPS
from local_support import PARAMS, random_matrix
from sgfull_affine_support import SgAffineOracle

NEW_SYMBOLS = ("swmi_global_full_affine", "swmi_global_full_affine_device", "swmi_global_full_affine_slices_for",
               "swmi_global_full_affine_time_device", "swmi_global_full_affine_release_workspaces")
MATRICES = [match_matrix(1, -1), match_matrix(5, -4), match_matrix(127, -127), random_matrix()]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullAffineOracle(tmp_path_factory.mktemp("global_full_affine_oracle"))


@pytest.fixture(scope="module")
def linear(tmp_path_factory):
    return GlobalFullOracle(tmp_path_factory.mktemp("global_full_oracle"))


@pytest.fixture(scope="module")
def sgaffine(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_affine_oracle"))


def small_pairs(rng, n, len1, len2):
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, len2 - w:] = np.where(rng.random(w) < 0.85, a[0, len1 - w:], b[0, len2 - w:])   # one similar pair
    if n > 2:
        a[1], b[1] = 0, 1                                                                  # one all-mismatch pair
        a[2], b[2] = 2, 2                                                                  # homopolymers: ties everywhere
    return a, b


@pytest.mark.parametrize("len1,len2", [(1, 1), (1, 7), (7, 1), (5, 30), (30, 5), (24, 24), (17, 33)])
def test_restatement_matches_numpy_under_every_mask(oracle, len1, len2):
    rng = np.random.default_rng(11 * len1 + len2)
    for p, (go, ge) in enumerate(AFFINE_GAPS):
        sm = MATRICES[p % len(MATRICES)]
        a, b = small_pairs(rng, 4, len1, len2)
        for mask in ALL_MASKS:
            sc, ends, mv, st = oracle.align(a, b, sm, go, ge, mask)
            sc2, ends2, _, _ = oracle.align(a, b, sm, go, ge, mask, traceback=False)
            assert np.array_equal(sc2, sc) and np.array_equal(ends2[:, :2], ends[:, :2]) and np.all(ends2[:, 2:] == -1)
            for k in range(len(a)):
                want_score, want_end, want_path, H = numpy_global_full_affine(a[k], b[k], sm, go, ge, mask)
                what = (go, ge, mask, k)
                assert sc[k] == want_score and tuple(ends[k, :2]) == want_end, what
                assert tuple(ends[k, 2:]) == tuple(want_path[0]) and st[k] == len(want_path) - 1, what
                assert np.array_equal(check_path(a[k], b[k], sm, go, ge, mask, sc[k], ends[k], mv[k], st[k]), want_path), what
                assert H[ends[k, 0], ends[k, 1]] == sc[k]


@pytest.mark.parametrize("p", range(len(PARAMS)))
def test_open_equal_extend_is_the_linear_aligner(oracle, linear, p):
    """open = extend = g: every field equals the linear restatement's (tests/native/global_full_oracle.c), under every mask."""
    match, mismatch, g = PARAMS[p]
    sm = match_matrix(match, mismatch)
    rng = np.random.default_rng(p)
    for len1, len2 in ((1, 1), (1, 40), (40, 1), (7, 300), (300, 7), (129, 131), (400, 300)):
        a, b = small_pairs(rng, 6, len1, len2)
        for mask in ALL_MASKS:
            want = linear.align(a, b, sm, g, mask)
            got = oracle.align(a, b, sm, g, g, mask)
            for x, y in zip(got[:2] + got[3:], want[:2] + want[3:]):
                assert np.array_equal(x, y), (p, len1, len2, mask)
            for k in range(len(a)):
                assert np.array_equal(moves_of(got[2][k], got[3][k]), moves_of(want[2][k], want[3][k])), (p, len1, len2, mask, k)


def test_mask_zero_is_the_affine_semiglobal_aligner_on_its_prefixes(oracle, sgaffine):
    """The mask-0 table is swmi_semiglobal_full_affine's table: for a pair whose best cell (ei, ej) there lies at (1, 1) or
    beyond, the mask-0 alignment of seq1[:ei], seq2[:ej] has that score, steps == lengths - 1 and the same moves.  Pairs
    whose best cell lies on a border have nothing to align; the seed is chosen so that they are at most a fifth of the draw."""
    drawn = used = 0
    for t, (len1, len2, go, ge) in enumerate(((60, 90, 3, 1), (200, 150, 11, 1), (333, 400, 5, 2), (128, 1030, 2, 5), (500, 500, 0, 0))):
        sm = MATRICES[t % 2]                                # (1, -1) and (5, -4): random pairs still reach positive scores
        a, b = related_pairs(9, len1, len2, 40 + t)
        sc, ends, mv, ln = sgaffine.align(a, b, sm, go, ge)
        for k in range(len(a)):
            drawn += 1
            ei, ej = (int(x) for x in ends[k])
            if ei < 1 or ej < 1:
                assert sc[k] == 0
                continue
            used += 1
            gsc, gends, gmv, gst = oracle.align(a[k:k + 1, :ei], b[k:k + 1, :ej], sm, go, ge, GLOBAL)
            what = (t, k)
            assert gsc[0] == sc[k] and tuple(gends[0]) == (ei, ej, 0, 0), what
            assert gst[0] == ln[k] - 1, what
            assert np.array_equal(moves_of(gmv[0], gst[0]), moves_of(mv[k], ln[k] - 1)), what
    assert used >= 20 and 5 * (drawn - used) <= drawn, (drawn, used)


def swap_mask(mask):
    return ((mask & BEGIN1) << 1) | ((mask & BEGIN2) >> 1) | ((mask & END1) << 1) | ((mask & END2) >> 1)


def test_properties_of_masks_and_gap_costs(oracle):
    """On 200 random pairs: one more free end never lowers the score; a higher open or extend never raises it; swapping the
    sequences with the matrix transposed and the mask's bits swapped (1 <-> 2, 4 <-> 8) keeps it; every path passes
    check_path."""
    assert [swap_mask(m) for m in (0, 1, 2, 4, 8, 15, FIT)] == [0, 2, 1, 8, 4, 15, BEGIN1 | END1]
    rng = np.random.default_rng(17)
    for t in range(200):
        len1, len2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        sm = MATRICES[t % len(MATRICES)]
        go, ge = AFFINE_GAPS[t % len(AFFINE_GAPS)]
        if go < 127 and ge < 127 and t % 3 == 0:
            go, ge = int(rng.integers(0, 20)), int(rng.integers(0, 20))
        a = rng.integers(0, 4, (1, len1), dtype=np.uint8)
        b = rng.integers(0, 4, (1, len2), dtype=np.uint8)
        if t % 4 == 0:
            w = min(len1, len2)
            b[0, :w] = a[0, :w]
        res = {m: oracle.align(a, b, sm, go, ge, m) for m in ALL_MASKS}
        score = {m: int(res[m][0][0]) for m in ALL_MASKS}
        smT = np.asarray(sm).reshape(4, 4).T.reshape(16).copy()
        for m in ALL_MASKS:
            for bit in (BEGIN1, BEGIN2, END1, END2):
                assert score[m | bit] >= score[m], (t, m, bit)
            assert int(oracle.align(b, a, smT, go, ge, swap_mask(m), traceback=False)[0][0]) == score[m], (t, m)
            if go < 127:
                assert int(oracle.align(a, b, sm, go + 1, ge, m, traceback=False)[0][0]) <= score[m], (t, m)
            if ge < 127:
                assert int(oracle.align(a, b, sm, go, ge + 1, m, traceback=False)[0][0]) <= score[m], (t, m)
            sc, ends, mv, st = res[m]
            check_path(a[0], b[0], sm, go, ge, m, sc[0], ends[0], mv[0], st[0])


def test_worked_examples(oracle):
    """Small cases with their answers by hand, at open 3, extend 1."""
    sm = match_matrix(1, -1)
    a, b = np.zeros((1, 3), np.uint8), np.ones((1, 5), np.uint8)
    sc, ends, mv, st = oracle.align(a, b, sm, 3, 1, GLOBAL)      # three mismatches and one gap of two: -3 - (3 + 1)
    assert sc[0] == -7 and tuple(ends[0]) == (3, 5, 0, 0) and st[0] == 5
    sc, ends, mv, st = oracle.align(a, b, sm, 3, 1, OVERLAP)     # nothing aligns: the first free end cell
    assert sc[0] == 0 and tuple(ends[0]) == (0, 5, 0, 5) and st[0] == 0
    a = np.array([[2, 3, 2]], np.uint8)
    b = np.array([[1, 1, 1, 1, 2, 3, 2, 1, 1]], np.uint8)
    sc, ends, mv, st = oracle.align(a, b, sm, 3, 1, FIT)
    assert sc[0] == 3 and tuple(ends[0]) == (3, 7, 0, 4) and st[0] == 3
    sc, ends, mv, st = oracle.align(a, b, sm, 3, 1, GLOBAL)      # a gap of two after it, a gap of four before it
    assert sc[0] == 3 - (3 + 1) - (3 + 3) and tuple(ends[0]) == (3, 9, 0, 0) and st[0] == 9
    assert list(moves_of(mv[0], st[0])) == [1, 1, 3, 3, 3, 1, 1, 1, 1]
    # one long gap beats many: 300 bases against themselves without bases 100..139
    rng = np.random.default_rng(11)
    x = rng.integers(0, 4, 300, dtype=np.uint8)
    y = np.concatenate([x[:100], x[140:]])
    sc, ends, mv, st = oracle.align(x[None], y[None], match_matrix(2, -3), 10, 1, GLOBAL)
    assert sc[0] == 2 * 260 - (10 + 39) and tuple(ends[0]) == (300, 260, 0, 0) and st[0] == 300
    codes = moves_of(mv[0], st[0])
    assert int((codes == 2).sum()) == 40 and int((codes == 1).sum()) == 0
    at = np.flatnonzero(codes == 2)
    assert at[-1] - at[0] == 39                                  # one run


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+SWMI_VERSION\s+300\b", text) and lib.swmi_version() == 300


def test_python_surface(swmi_mod):
    """swmi.global_affine is a submodule; its five functions have docstrings and stay out of the package's namespace."""
    mod = swmi_mod.global_affine
    assert inspect.ismodule(mod) and mod.__name__ == swmi_mod.__name__ + ".global_affine"
    names = ("global_full_affine", "global_full_affine_device", "global_full_affine_time_device", "global_full_affine_slices_for",
             "global_full_affine_release_workspaces")
    assert sorted(n for n, f in vars(mod).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == mod.__name__) \
        == sorted(names)
    for name in names:
        assert (getattr(mod, name).__doc__ or "").strip(), name
        assert not hasattr(swmi_mod, name), name
    assert str(inspect.signature(mod.global_full_affine)) == \
        "(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, traceback=True)"


def test_argument_errors_without_a_device(swmi_mod):
    lib = swmi_mod.load()
    sm = match_matrix(1, -1)
    a = np.zeros((2, 64), np.uint8)
    b = np.zeros((2, 64), np.uint8)
    sc = np.zeros(2, np.int32)
    ends = np.zeros((2, 4), np.int32)
    mv = np.zeros((2, move_words(64, 64)), np.uint64)
    st = np.zeros(2, np.uint32)
    P = lambda x: x.ctypes.data  # noqa: E731

    def call(len1=64, len2=64, s1=P(a), s2=P(b), go=3, ge=1, mask=0, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_global_full_affine(s1, len1, s2, len2, n, m, go, ge, mask, scores, e, moves, steps)
    assert call(len1=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len1=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(mask=16) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(mask=0xFFFFFFFF) == swmi_mod.ERR_INVALID_ARGUMENT
    for bad in (-1, 128):
        assert call(go=bad) == swmi_mod.ERR_DOMAIN and b"gap_open" in lib.swmi_last_error()
        assert call(ge=bad) == swmi_mod.ERR_DOMAIN
    assert call(s1=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(s2=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(m=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(scores=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(e=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(steps=None) == swmi_mod.ERR_INVALID_ARGUMENT            # moves without steps
    assert call(moves=None) == swmi_mod.ERR_INVALID_ARGUMENT            # steps without moves
    dev = lib.swmi_global_full_affine_device
    assert dev(P(a), 0, P(b), 64, 2, P(sm), 3, 1, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 16385, 2, P(sm), 3, 1, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 3, 1, 16, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 3, 128, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 3, 1, 0, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    ms = ctypes.c_float()
    timer = lib.swmi_global_full_affine_time_device
    assert timer(P(a), 64, P(b), 0, 2, P(sm), 3, 1, 0, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 3, 1, 16, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), -1, 1, 0, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_DOMAIN
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 3, 1, 0, P(sc), P(ends), None, None, None, 0, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    ga = swmi_mod.global_affine
    for kwargs in ({"gap_open": 2**31}, {"gap_extend": -2**31 - 1}):
        with pytest.raises(swmi_mod.SwmiError) as err:                 # ctypes would wrap it to a C int
            ga.global_full_affine(a, b, sm, **dict({"gap_open": 3, "gap_extend": 1}, **kwargs))
        assert err.value.code == swmi_mod.ERR_DOMAIN
    for mask in (16, -1):
        with pytest.raises(swmi_mod.SwmiError) as err:
            ga.global_full_affine(a, b, sm, 3, 1, free_ends=mask)
        assert err.value.code == swmi_mod.ERR_INVALID_ARGUMENT
    # n = 0 is a no-op that needs no device
    assert call(n=0) == 0 and call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, steps=None) == 0
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_slices_for(swmi_mod):
    ga = swmi_mod.global_affine
    full = lambda n, tb=True: ga.global_full_affine_slices_for(n, 16384, 16384, tb)  # noqa: E731
    assert full(0) == [] and full(1) == [1] and full(256) == [256] and full(257) == [256, 1]
    assert full(1000) == [256, 256, 256, 232]
    for len1, len2 in ((1, 1), (63, 65), (1000, 1000), (4096, 777), (16384, 1)):
        for tb in (True, False):
            for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
                s = ga.global_full_affine_slices_for(n, len1, len2, tb)
                assert s == swmi_mod.local_full_affine_slices_for(n, len1, len2, tb)   # the same budgets and result layout
                assert sum(s) == n and all(x >= 1 for x in s) and all(x <= 1 << 20 for x in s)
    assert ga.global_full_affine_slices_for(10, 0, 5) == [] and ga.global_full_affine_slices_for(10, 5, 16385) == []


def test_expand_moves_rebuilds_the_path(swmi_mod, oracle):
    """swmi_local_full_expand_moves takes the affine global aligner's (moves, steps, end) unchanged, forced moves included."""
    rng = np.random.default_rng(3)
    a, b = small_pairs(rng, 5, 30, 70)
    for mask in (GLOBAL, FIT, OVERLAP, BEGIN1 | END1):
        sc, ends, mv, st = oracle.align(a, b, match_matrix(1, -1), 3, 1, mask)
        for k in range(len(a)):
            want = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert np.array_equal(swmi_mod.local_full_expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1]), want), (mask, k)


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_full_affine.cpp"), "-o",
                            str(tmp_path / "compat_global_full_affine"), "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
