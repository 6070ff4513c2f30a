"""The any-length local aligner (swmi_local_full*, include/swmi.h) without a device: the C restatement
tests/native/local_full_oracle.c against the 128-column restatement and fixture F7 (what the reference's
SmithWaterman_111_long returned), against an independent numpy formulation on small shapes, against F7 transposed (len2 up
to 16384) and fixture F1; the properties every path has whatever the tie rules; the C ABI surface, its argument errors, the
slicing rule, the moves expander and the C++ header."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_full_support import LocalFullOracle, check_path, move_words, numpy_local_full, path_from
from local_support import PARAMS, LocalOracle, f7_by_length, path_to_moves, random_matrix

NEW_SYMBOLS = ("swmi_local_full", "swmi_local_full_device", "swmi_local_full_slices_for", "swmi_local_full_time_device",
               "swmi_local_full_release_workspaces", "swmi_local_full_expand_moves")
ALL_PARAMS = [(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(), 3)]


@pytest.fixture(scope="module")
def oracle_full(tmp_path_factory):
    return LocalFullOracle(tmp_path_factory.mktemp("local_full_oracle"))


@pytest.fixture(scope="module")
def oracle_128(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def test_restatement_equals_the_128_column_one_and_f7(oracle_full, oracle_128):
    for len1, (a, b, f7_scores, f7_paths) in f7_by_length().items():
        for p, (sm, gap) in enumerate(ALL_PARAMS):
            sc, ends, mv, st = oracle_full.align(a, b, sm, gap)
            wsc, wends, wmv, wst = oracle_128.align(a, b, sm, gap)
            assert np.array_equal(sc, wsc) and np.array_equal(ends, wends) and np.array_equal(st, wst), (len1, p)
            for k in range(len(sc)):
                assert np.array_equal(path_from(mv[k], st[k], ends[k, 0], ends[k, 1]),
                                      path_from(wmv[k], wst[k], wends[k, 0], wends[k, 1])), (len1, p, k)
                check_path(a[k], b[k], sm, gap, sc[k], ends[k], mv[k], st[k])
            sc2, ends2, _, _ = oracle_full.align(a, b, sm, gap, traceback=False)
            assert np.array_equal(sc2, sc) and np.array_equal(ends2[:, :2], ends[:, :2]) and np.all(ends2[:, 2:] == -1)
        # the real SmithWaterman_111_long at (1, -1, 1)
        sc, ends, mv, st = oracle_full.align(a, b, match_matrix(1, -1), 1)
        assert np.array_equal(sc, f7_scores), len1
        for k, path in enumerate(f7_paths):
            assert np.array_equal(path_from(mv[k], st[k], ends[k, 0], ends[k, 1]), path), (len1, k)


@pytest.mark.parametrize("len1,len2", [(1, 1), (5, 300), (300, 5), (200, 200), (129, 131), (17, 1)])
def test_restatement_matches_numpy_on_small_shapes(oracle_full, len1, len2):
    rng = np.random.default_rng(7 * len1 + len2)
    for p, (sm, gap) in enumerate(ALL_PARAMS):
        a = rng.integers(0, 4, (6, len1), dtype=np.uint8)
        b = rng.integers(0, 4, (6, len2), dtype=np.uint8)
        w = min(len1, len2)
        b[0, :w] = np.where(rng.random(w) < 0.85, a[0, :w], b[0, :w])       # one similar pair
        a[1], b[1] = 0, 1                                                   # one all-mismatch pair (unless the matrix rewards it)
        a[2], b[2] = 2, 2                                                   # homopolymers: ties everywhere
        sc, ends, mv, st = oracle_full.align(a, b, sm, gap)
        for k in range(6):
            want_score, want_end, want_path, H = numpy_local_full(a[k], b[k], sm, gap)
            assert sc[k] == want_score and tuple(ends[k, :2]) == want_end, (p, k)
            assert tuple(ends[k, 2:]) == tuple(want_path[0]) and st[k] == len(want_path) - 1, (p, k)
            assert np.array_equal(check_path(a[k], b[k], sm, gap, sc[k], ends[k], mv[k], st[k], H), want_path), (p, k)


def test_transposed_f7_pins_long_seq2_to_the_reference(oracle_full):
    """F7's long read as seq2 and its 128-mer as seq1 with the transposed matrix: the score is the reference's."""
    sm = match_matrix(1, -1).reshape(4, 4).T.reshape(16).copy()
    for len1, (a, b, f7_scores, _) in f7_by_length().items():
        sc, ends, mv, st = oracle_full.align(b, a, sm, 1)
        assert np.array_equal(sc, f7_scores), len1
        for k in range(len(sc)):
            check_path(b[k], a[k], sm, 1, sc[k], ends[k], mv[k], st[k])
    # and an asymmetric matrix against the 128-column restatement's own scores
    rm = random_matrix()
    a, b, _, _ = f7_by_length()[1000]
    want, _, _, _ = oracle_full.align(a, b, rm, 3)
    got, _, _, _ = oracle_full.align(b, a, rm.reshape(4, 4).T.reshape(16).copy(), 3)
    assert np.array_equal(got, want)


def test_scores_equal_f1_at_128_by_128(oracle_full, golden):
    f1 = golden("f1_random")
    for p in range(len(f1["gap"])):
        sc, _, _, _ = oracle_full.align(f1["seq1"], f1["seq2"], f1["sm"][p], int(f1["gap"][p]), traceback=False)
        assert np.array_equal(sc, f1["scores"][p]), p


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+SWMI_LOCAL_FULL_MAX_LEN\s+16384\b", text)
    assert "SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2)" in text
    assert re.search(r"#define\s+SWMI_VERSION\s+300\b", text)


def test_python_surface(swmi_mod):
    for name in ("local_full", "local_full_device", "local_full_time_device", "local_full_slices_for", "local_full_move_words",
                 "local_full_expand_moves", "local_full_release_workspaces"):
        assert callable(getattr(swmi_mod, name)), name
    for len1, len2 in ((1, 1), (16384, 16384), (100, 3000), (31, 1)):
        assert swmi_mod.local_full_move_words(len1, len2) == move_words(len1, len2) == swmi_mod.semiglobal_full_move_words(len1, len2)


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

    def call(len1=64, len2=64, s1=P(a), s2=P(b), gap=1, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_local_full(s1, len1, s2, len2, n, m, gap, scores, e, moves, steps)
    assert call(len1=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len1=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(gap=-1) == swmi_mod.ERR_DOMAIN
    assert call(s1=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(s2=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(m=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(scores=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(e=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(steps=None) == swmi_mod.ERR_INVALID_ARGUMENT            # moves without steps
    assert call(moves=None) == swmi_mod.ERR_INVALID_ARGUMENT            # steps without moves
    dev = lib.swmi_local_full_device
    assert dev(P(a), 0, P(b), 64, 2, P(sm), 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 16385, 2, P(sm), 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), -3, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 1, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    ms = ctypes.c_float()
    timer = lib.swmi_local_full_time_device
    assert timer(P(a), 64, P(b), 0, 2, P(sm), 1, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 1, P(sc), P(ends), None, None, None, 0, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full(a, b, sm, 300)                             # ctypes would wrap it to an int8
    # n = 0 is a no-op that needs no device, on both entries
    assert call(n=0) == 0 and call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, steps=None) == 0
    assert dev(None, 64, None, 64, 0, P(sm), 1, None, None, None, None, None) == 0
    out = swmi_mod.local_full(np.zeros((0, 5), np.uint8), np.zeros((0, 9), np.uint8), sm, 1)
    assert out[0].shape == (0,) and out[1].shape == (0, 4)
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_slices_for(swmi_mod):
    """Values worked out by hand from the budget: a traceback slice is what 256 alignments of 16384 x 16384 take."""
    full = lambda n, tb=True: swmi_mod.local_full_slices_for(n, 16384, 16384, tb)  # noqa: E731
    assert full(0) == [] and full(1) == [1] and full(256) == [256] and full(257) == [256, 1]
    assert full(1000) == [256, 256, 256, 232]
    # ends-only: 256 MiB over inputs and results, 16384 + 16384 bytes of bases, 4 of score, 16 of ends
    per = 16384 + 16384 + 4 + 16
    sizes = full(100000, False)
    assert sum(sizes) == 100000 and sizes[0] == (256 << 20) // per == 8187 and all(s <= sizes[0] for s in sizes)
    # traceback at 4096 x 4096: 4 waves x 1040 trips (130 chunks of 8) x 256 dwords of codes, 256 move words, against 256
    # full-size alignments of 16 waves x 4112 trips (514 chunks) x 256 dwords and 1024 move words
    one = 4096 + 4096 + 4 + 16 + 4 * 1040 * 256 * 4 + 256 * 8 + 4
    budget = 256 * (16384 + 16384 + 4 + 16 + 16 * 4112 * 256 * 4 + 1024 * 8 + 4)
    assert swmi_mod.local_full_slices_for(10 ** 6, 4096, 4096)[0] == budget // one
    # the cap of 2^20 alignments per slice
    assert swmi_mod.local_full_slices_for(3 * (1 << 20) + 5, 1, 1, False) == [1 << 20] * 3 + [5]
    for len1, len2 in ((1, 1), (63, 65), (1000, 1000), (4096, 777), (16384, 1)):
        for tb in (True, False):
            for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
                s = swmi_mod.local_full_slices_for(n, len1, len2, tb)
                assert sum(s) == n and all(x >= 1 for x in s) and all(x == s[0] for x in s[:-1])
                assert all(x <= 1 << 20 for x in s)
    assert swmi_mod.local_full_slices_for(10, 0, 5) == [] and swmi_mod.local_full_slices_for(10, 5, 16385) == []
    assert swmi_mod.local_full_slices_for(10, 16385, 5) == [] and swmi_mod.local_full_slices_for(10, 5, 0) == []


def test_expand_moves(swmi_mod):
    for len1, (_, _, _, paths) in f7_by_length().items():
        for k, path in enumerate(paths):
            row = path_to_moves(path, move_words(len1, 128))
            got = swmi_mod.local_full_expand_moves(row, len(path) - 1, path[-1][0], path[-1][1])
            assert np.array_equal(got, path), (len1, k)
            assert np.array_equal(swmi_mod.local_full_expand_moves(row, len(path) - 1, path[-1][0], path[-1][1], cap=2), path[:2])
    # an end cell with j > 128, which swmi_local_expand_moves rejects and keeps rejecting
    row = np.zeros(2, np.uint64)
    row[0] = 3 | 1 << 2 | 2 << 4
    assert swmi_mod.local_full_expand_moves(row, 3, 5, 9000).tolist() == [[3, 8998], [4, 8998], [4, 8999], [5, 9000]]
    assert swmi_mod.local_full_expand_moves(row, 0, 16384, 16384).tolist() == [[16384, 16384]]
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_expand_moves(row, 3, 5, 9000)
    for steps, end in ((3, (1, 9)), (3, (9, 1)), (1, (0, 0)), (0, (16385, 1)), (0, (1, 16385)), (0, (-1, 0)), (4, (9, 9))):
        with pytest.raises(swmi_mod.SwmiError):                        # leaves the matrix, starts outside it, or a move of 0
            swmi_mod.local_full_expand_moves(row, steps, end[0], end[1])


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    syntax = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"),
                             os.path.join(ROOT, "tests", "native", "compat_local_full.cpp")],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert syntax.returncode == 0, syntax.stdout
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local_full.cpp"), "-o", str(tmp_path / "compat_local_full"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
