"""The global / free-end-gap aligner (swmi_global_full*, include/swmi.h) without a device.  Its semantics have no reference
counterpart, so the C restatement tests/native/global_full_oracle.c is their definition; here it is checked against an
independent numpy formulation (all 16 masks), against the semi-global restatement tests/native/sgfull_oracle.c (its score is
the largest mask-0 score over all prefixes), against fixture F8 (the reference's SemiGlobal_111: a mask-0 alignment of the
prefixes that end at F8's best cell is F8's path) and against the properties of the masks; then the C ABI surface, its
argument errors, the slicing rule and the C++ header."""
import ctypes
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from global_full_support import (ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullOracle, check_path, move_words,
                                 numpy_global_full, numpy_table, path_from)
from local_support import PARAMS, random_matrix
from sgfull_support import K111, SgFullOracle, load_f8

NEW_SYMBOLS = ("swmi_global_full", "swmi_global_full_device", "swmi_global_full_slices_for", "swmi_global_full_time_device",
               "swmi_global_full_release_workspaces")
ALL_PARAMS = [(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(), 3)]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullOracle(tmp_path_factory.mktemp("global_full_oracle"))


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


def small_pairs(rng, n, len1, len2):
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, len2 - w:] = np.where(rng.random(w) < 0.85, a[0, len1 - w:], b[0, len2 - w:])   # one similar pair
    if n > 2:
        a[1], b[1] = 0, 1                                                                  # one all-mismatch pair
        a[2], b[2] = 2, 2                                                                  # homopolymers: ties everywhere
    return a, b


@pytest.mark.parametrize("len1,len2", [(1, 1), (1, 7), (7, 1), (5, 40), (40, 5), (40, 40), (17, 33), (33, 16)])
def test_restatement_matches_numpy_under_every_mask(oracle, len1, len2):
    rng = np.random.default_rng(11 * len1 + len2)
    for p, (sm, gap) in enumerate(ALL_PARAMS):
        a, b = small_pairs(rng, 5, len1, len2)
        for mask in ALL_MASKS:
            sc, ends, mv, st = oracle.align(a, b, sm, gap, mask)
            sc2, ends2, _, _ = oracle.align(a, b, sm, gap, mask, traceback=False)
            assert np.array_equal(sc2, sc) and np.array_equal(ends2[:, :2], ends[:, :2]) and np.all(ends2[:, 2:] == -1)
            for k in range(len(a)):
                want_score, want_end, want_path, H = numpy_global_full(a[k], b[k], sm, gap, mask)
                assert sc[k] == want_score and tuple(ends[k, :2]) == want_end, (p, mask, k)
                assert tuple(ends[k, 2:]) == tuple(want_path[0]) and st[k] == len(want_path) - 1, (p, mask, k)
                assert np.array_equal(check_path(a[k], b[k], sm, gap, mask, sc[k], ends[k], mv[k], st[k]), want_path), (p, mask, k)
                assert H[ends[k, 0], ends[k, 1]] == sc[k]


def test_mask_zero_over_all_prefixes_is_the_semiglobal_aligner(oracle, sgoracle):
    """SemiGlobal's best cell is the first cell in row-major order that holds the largest H of the mask-0 table, 0 at (0, 0)
    included; H(i, j) of that table is the mask-0 score of the prefixes (i, j)."""
    rng = np.random.default_rng(5)
    for len1, len2 in ((1, 1), (9, 40), (40, 9), (40, 40), (23, 31)):
        for sm, gap in ALL_PARAMS:
            a, b = small_pairs(rng, 4, len1, len2)
            want_sc, want_ends, _, _ = sgoracle.align(a, b, sm, gap)
            for k in range(len(a)):
                best, at = 0, (0, 0)
                for i in range(1, len1 + 1):
                    for j in range(1, len2 + 1):
                        sc, _, _, _ = oracle.align(a[k:k + 1, :i], b[k:k + 1, :j], sm, gap, GLOBAL, traceback=False)
                        if sc[0] > best:
                            best, at = int(sc[0]), (i, j)
                assert best == want_sc[k] and at == tuple(want_ends[k]), (len1, len2, k)


def f8_vectors():
    """(k, seq1 prefix, seq2 prefix, score, path) of the 25 F8 vectors whose best cell lies at (1, 1) or beyond; the two
    with score 0 (best cell (0, 0)) have no prefixes to align."""
    f8 = load_f8()
    out = []
    for k in range(len(f8["scores"])):
        ei, ej = (int(x) for x in f8["ends"][k])
        if ei >= 1 and ej >= 1:
            out.append((k, f8["seq1"][k:k + 1, :ei], f8["seq2"][k:k + 1, :ej], int(f8["scores"][k]), f8["paths"][k], int(f8["lengths"][k])))
        else:
            assert f8["scores"][k] == 0
    assert len(out) == 25
    return out


def test_f8_the_references_semiglobal_is_a_global_alignment_of_its_prefixes(oracle):
    def one(v):
        k, a, b, score, path, length = v
        sc, ends, mv, st = oracle.align(a, b, K111, 1, GLOBAL)
        assert sc[0] == score, k
        assert tuple(ends[0]) == (a.shape[1], b.shape[1], 0, 0), k
        assert st[0] == length - 1, k
        assert np.array_equal(path_from(mv[0], st[0], ends[0, 0], ends[0, 1]), path), k
        return k
    with ThreadPoolExecutor(8) as pool:
        assert len(list(pool.map(one, f8_vectors()))) == 25


def swap_mask(mask):
    return ((mask & BEGIN1) << 1) | ((mask & BEGIN2) >> 1) | ((mask & END1) << 1) | ((mask & END2) >> 1)


def test_properties_of_the_masks(oracle):
    assert [swap_mask(m) for m in (0, 1, 2, 4, 8, 15, FIT)] == [0, 2, 1, 8, 4, 15, BEGIN1 | END1]
    rng = np.random.default_rng(17)
    for t in range(200):
        len1, len2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        sm, gap = ALL_PARAMS[t % len(ALL_PARAMS)]
        a = rng.integers(0, 4, (1, len1), dtype=np.uint8)
        b = rng.integers(0, 4, (1, len2), dtype=np.uint8)
        score = {m: int(oracle.align(a, b, sm, gap, m, traceback=False)[0][0]) for m in ALL_MASKS}
        smT = np.asarray(sm).reshape(4, 4).T.reshape(16).copy()
        for m in ALL_MASKS:
            for bit in (BEGIN1, BEGIN2, END1, END2):
                assert score[m | bit] >= score[m], (t, m, bit)                   # one more free end never lowers the score
            assert int(oracle.align(b, a, smT, gap, swap_mask(m), traceback=False)[0][0]) == score[m], (t, m)


def test_worked_examples(oracle):
    """Small cases with their answers by hand."""
    sm = match_matrix(1, -1)
    a, b = np.zeros((1, 3), np.uint8), np.ones((1, 5), np.uint8)
    sc, ends, mv, st = oracle.align(a, b, sm, 1, GLOBAL)                          # all mismatch: -max(len1, len2)
    assert sc[0] == -5 and tuple(ends[0]) == (3, 5, 0, 0) and st[0] == 5
    assert [int(mv[0, 0] >> (2 * t)) & 3 for t in range(5)] == [3, 3, 3, 1, 1]    # three diagonals reach row 0, then forced lefts
    sc, ends, mv, st = oracle.align(a, b, sm, 1, OVERLAP)                         # nothing aligns: the first free end cell
    assert sc[0] == 0 and tuple(ends[0]) == (0, 5, 0, 5) and st[0] == 0
    # fit: seq1 = 2 3 2 inside seq2 at offset 4
    a = np.array([[2, 3, 2]], np.uint8)
    b = np.array([[1, 1, 1, 1, 2, 3, 2, 1, 1]], np.uint8)
    sc, ends, mv, st = oracle.align(a, b, sm, 1, FIT)
    assert sc[0] == 3 and tuple(ends[0]) == (3, 7, 0, 4) and st[0] == 3
    sc, ends, mv, st = oracle.align(a, b, sm, 1, GLOBAL)
    assert sc[0] == 3 - 6 and tuple(ends[0]) == (3, 9, 0, 0) and st[0] == 9


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+SWMI_GLOBAL_FULL_MAX_LEN\s+16384\b", text)
    assert "SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2)" in text
    for name in ("SWMI_FREE_BEGIN1 1u", "SWMI_FREE_BEGIN2 2u", "SWMI_FREE_END1 4u", "SWMI_FREE_END2 8u", "SWMI_ENDS_GLOBAL 0u"):
        assert re.search(r"#define\s+" + re.escape(name), text), name
    assert re.search(r"#define\s+SWMI_VERSION\s+300\b", text)


def test_python_surface(swmi_mod):
    for name in ("global_full", "global_full_device", "global_full_time_device", "global_full_slices_for", "global_full_move_words",
                 "global_full_release_workspaces"):
        assert callable(getattr(swmi_mod, name)), name
    assert (swmi_mod.FREE_BEGIN1, swmi_mod.FREE_BEGIN2, swmi_mod.FREE_END1, swmi_mod.FREE_END2) == (BEGIN1, BEGIN2, END1, END2)
    assert (swmi_mod.ENDS_GLOBAL, swmi_mod.ENDS_FIT, swmi_mod.ENDS_OVERLAP) == (GLOBAL, FIT, OVERLAP) == (0, 10, 15)
    for len1, len2 in ((1, 1), (16384, 16384), (100, 3000), (31, 1)):
        assert swmi_mod.global_full_move_words(len1, len2) == move_words(len1, len2) == swmi_mod.local_full_move_words(len1, len2)


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

    def call(len1=64, len2=64, s1=P(a), s2=P(b), gap=1, mask=0, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_global_full(s1, len1, s2, len2, n, m, gap, mask, scores, e, moves, steps)
    assert call(len1=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len1=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(mask=16) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(mask=0xFFFFFFFF) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(gap=-1) == swmi_mod.ERR_DOMAIN
    assert call(s1=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(s2=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(m=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(scores=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(e=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(steps=None) == swmi_mod.ERR_INVALID_ARGUMENT            # moves without steps
    assert call(moves=None) == swmi_mod.ERR_INVALID_ARGUMENT            # steps without moves
    dev = lib.swmi_global_full_device
    assert dev(P(a), 0, P(b), 64, 2, P(sm), 1, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 16385, 2, P(sm), 1, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 1, 16, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), -3, 0, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 1, 0, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    ms = ctypes.c_float()
    timer = lib.swmi_global_full_time_device
    assert timer(P(a), 64, P(b), 0, 2, P(sm), 1, 0, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 1, 16, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 1, 0, P(sc), P(ends), None, None, None, 0, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.global_full(a, b, sm, 300)                            # ctypes would wrap it to an int8
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.global_full(a, b, sm, 1, free_ends=16)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.global_full(a, b, sm, 1, free_ends=-1)
    # n = 0 is a no-op that needs no device
    assert call(n=0) == 0 and call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, steps=None) == 0
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_slices_for(swmi_mod):
    full = lambda n, tb=True: swmi_mod.global_full_slices_for(n, 16384, 16384, tb)  # noqa: E731
    assert full(0) == [] and full(1) == [1] and full(256) == [256] and full(257) == [256, 1]
    assert full(1000) == [256, 256, 256, 232]
    for len1, len2 in ((1, 1), (63, 65), (1000, 1000), (4096, 777), (16384, 1)):
        for tb in (True, False):
            for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
                s = swmi_mod.global_full_slices_for(n, len1, len2, tb)
                assert s == swmi_mod.local_full_slices_for(n, len1, len2, tb)       # the same budgets and result layout
                assert sum(s) == n and all(x >= 1 for x in s) and all(x <= 1 << 20 for x in s)
    assert swmi_mod.global_full_slices_for(10, 0, 5) == [] and swmi_mod.global_full_slices_for(10, 5, 16385) == []


def test_expand_moves_rebuilds_a_path_that_ends_on_a_border(swmi_mod, oracle):
    """swmi_local_full_expand_moves takes the global aligner's (moves, steps, end) unchanged, forced moves included."""
    rng = np.random.default_rng(3)
    a, b = small_pairs(rng, 5, 30, 70)
    for mask in (GLOBAL, FIT, OVERLAP, BEGIN1 | END1):
        sc, ends, mv, st = oracle.align(a, b, match_matrix(1, -1), 1, mask)
        for k in range(len(a)):
            want = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert np.array_equal(swmi_mod.local_full_expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1]), want), (mask, k)


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_full.cpp"), "-o", str(tmp_path / "compat_global_full"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
