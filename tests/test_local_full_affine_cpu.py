"""The any-length affine local aligner (swmi_local_full_affine*, include/swmi.h) without a device: the C restatement
tests/native/local_full_affine_oracle.c against the 128-column affine restatement (every F7 length, matrix and gap pair),
against the linear any-length restatement at open == extend, against fixture F7 (what the reference's SmithWaterman_111_long
returned) at (1, -1, 1, 1), against an independent numpy formulation -- walk states included -- on small shapes, and under
the transposition that swaps E and F; the properties every path has whatever the tie rules; the C ABI surface, its argument
errors and the slicing rule."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle
from local_full_affine_support import (LocalFullAffineOracle, assert_same, check_path, gotoh_numpy, inputs, move_words,
                                       moves_as_letters, path_from, per_alignment)
from local_full_support import LocalFullOracle
from local_support import PARAMS, f7_by_length, random_matrix

NEW_SYMBOLS = ("swmi_local_full_affine", "swmi_local_full_affine_device", "swmi_local_full_affine_slices_for",
               "swmi_local_full_affine_time_device", "swmi_local_full_affine_release_workspaces")
MATRICES = [match_matrix(m, x) for m, x, _ in PARAMS]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LocalFullAffineOracle(tmp_path_factory.mktemp("local_full_affine_oracle"))


@pytest.fixture(scope="module")
def oracle_128(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


@pytest.fixture(scope="module")
def oracle_linear(tmp_path_factory):
    return LocalFullOracle(tmp_path_factory.mktemp("local_full_oracle"))


def _same_up_to_steps(got, want, what):
    """assert_same for two results whose move rows have different widths"""
    sc, ends, mv, st = got
    wsc, wends, wmv, wst = want
    assert np.array_equal(sc, wsc) and np.array_equal(ends, wends) and np.array_equal(st, wst), what
    for k in range(len(sc)):
        assert np.array_equal(path_from(mv[k], st[k], ends[k, 0], ends[k, 1]), path_from(wmv[k], wst[k], wends[k, 0], wends[k, 1])), (what, k)


def test_restatement_equals_the_128_column_affine_one(oracle, oracle_128):
    for len1, (a, b, _, _) in f7_by_length().items():
        for p, sm in enumerate(MATRICES):
            for go, ge in AFFINE_GAPS:
                got = oracle.align(a, b, sm, go, ge)
                _same_up_to_steps(got, oracle_128.align(a, b, sm, go, ge), (len1, p, go, ge))
                sc, ends, mv, st = got
                for k in range(len(sc)):
                    check_path(a[k], b[k], sm, go, ge, sc[k], ends[k], mv[k], st[k])
                sc2, ends2, _, _ = oracle.align(a, b, sm, go, ge, traceback=False)
                assert np.array_equal(sc2, sc) and np.array_equal(ends2[:, :2], ends[:, :2]) and np.all(ends2[:, 2:] == -1)


@pytest.mark.parametrize("len1,len2", [(100, 300), (129, 1100), (700, 2100), (2100, 700), (1, 129)])
def test_restatement_equals_the_linear_one_at_open_equal_extend(oracle, oracle_linear, len1, len2):
    a, b = inputs(9, len1, len2, len1 + len2)
    for p, (sm, g) in enumerate([(match_matrix(m, x), g) for m, x, g in PARAMS] + [(random_matrix(), 3)]):
        assert_same(oracle.align(a, b, sm, g, g), oracle_linear.align(a, b, sm, g), (len1, len2, p))


def test_restatement_reproduces_f7(oracle):
    """the real SmithWaterman_111_long: (1, -1) with gap 1 is open = extend = 1"""
    for len1, (a, b, f7_scores, f7_paths) in f7_by_length().items():
        sc, ends, mv, st = oracle.align(a, b, match_matrix(1, -1), 1, 1)
        assert np.array_equal(sc, f7_scores), len1
        for k, path in enumerate(f7_paths):
            assert np.array_equal(path_from(mv[k], st[k], ends[k, 0], ends[k, 1]), path), (len1, k)


@pytest.mark.parametrize("len1,len2", [(40, 150), (150, 135), (1, 1), (3, 140)])
def test_restatement_matches_numpy_on_small_shapes(oracle, golden, len1, len2):
    f1 = golden("f1_random")
    rng = np.random.default_rng(13 * len1 + len2)
    for p in range(len(f1["gap"])):
        sm = f1["sm"][p]
        a = rng.integers(0, 4, (4, len1), dtype=np.uint8)
        b = rng.integers(0, 4, (4, len2), dtype=np.uint8)
        w = min(len1, len2)
        b[0, :w] = np.where(rng.random(w) < 0.85, a[0, :w], b[0, :w])       # one similar pair
        if w > 30:
            b[1, :w - 9] = np.concatenate([a[1, :w // 2 - 9], a[1, w // 2:w]])   # one with 9 bases of seq1 missing: an up run
        a[2], b[2] = 2, 2                                                   # homopolymers: ties everywhere
        for go, ge in AFFINE_GAPS:
            sc, ends, mv, st = oracle.align(a, b, sm, go, ge)
            for k in range(4):
                score, want_ends, letters, states, _ = gotoh_numpy(a[k], b[k], sm, go, ge)
                assert sc[k] == score and tuple(ends[k]) == want_ends and st[k] == len(letters), (p, go, ge, k)
                assert moves_as_letters(mv[k], st[k]) == letters, (p, go, ge, k)
                # the states the walk was in: a diagonal only in H, an up only in E, a left only in F
                assert all(s == {"D": "H", "U": "E", "L": "F"}[m] for m, s in zip(letters, states))
                check_path(a[k], b[k], sm, go, ge, sc[k], ends[k], mv[k], st[k])


def _planted(n, len1, len2, seed):
    """seq2 = X + R + Y against seq1 = X + Y and the other way round in turn: one long indel each"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    for k in range(n):
        w = min(len1, len2) - 80
        x = rng.integers(0, 4, w, dtype=np.uint8)
        r = int(rng.integers(5, 70))
        y = np.concatenate([x[:w // 2], rng.integers(0, 4, r, dtype=np.uint8), x[w // 2:]])
        if k % 2:
            a[k, :len(y)], b[k, :w] = y, x
        else:
            a[k, :w], b[k, :len(y)] = x, y
    return a, b


@pytest.mark.parametrize("len1,len2", [(300, 2100), (2100, 300), (1500, 1500)])
def test_scores_survive_the_transposition_that_swaps_E_and_F(oracle, len1, len2):
    """(a, b, sm, o, e) and (b, a, sm^T, o, e) score alike: F of the one is E of the other, also at large len2"""
    for make, seed in ((inputs, 5), (_planted, 6)):
        a, b = make(8, len1, len2, seed + len1)
        for sm in (match_matrix(2, -3), random_matrix(), match_matrix(5, -4)):
            smt = np.asarray(sm, np.int8).reshape(4, 4).T.reshape(16).copy()
            for go, ge in AFFINE_GAPS + [(12, 1), (6, 6), (12, 0), (0, 3)]:
                sc, ends, mv, st = oracle.align(a, b, sm, go, ge)
                tsc, tends, tmv, tst = oracle.align(b, a, smt, go, ge)
                assert np.array_equal(sc, tsc), (len1, len2, go, ge)
                for k in range(0, 8, 3):
                    check_path(a[k], b[k], sm, go, ge, sc[k], ends[k], mv[k], st[k])
                    check_path(b[k], a[k], smt, go, ge, tsc[k], tends[k], tmv[k], tst[k])


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name
    assert re.search(r"#define\s+SWMI_VERSION\s+300\b", text)


def test_python_surface(swmi_mod):
    for name in ("local_full_affine", "local_full_affine_device", "local_full_affine_time_device", "local_full_affine_slices_for",
                 "local_full_affine_release_workspaces"):
        assert callable(getattr(swmi_mod, name)), name


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

    def call(len1=64, len2=64, s1=P(a), s2=P(b), go=3, ge=1, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc), e=P(ends), n=2):
        return lib.swmi_local_full_affine(s1, len1, s2, len2, n, m, go, ge, scores, e, moves, steps)
    for bad in (dict(len1=0), dict(len2=0), dict(len1=16385), dict(len2=16385), dict(s1=None), dict(s2=None), dict(m=None),
                dict(scores=None), dict(e=None), dict(steps=None), dict(moves=None)):
        assert call(**bad) == swmi_mod.ERR_INVALID_ARGUMENT, bad
    for bad in (dict(go=-1), dict(ge=-1), dict(go=128), dict(ge=128)):
        assert call(**bad) == swmi_mod.ERR_DOMAIN, bad
    assert call(len1=0, go=-1) == swmi_mod.ERR_INVALID_ARGUMENT         # lengths are checked before the gaps
    dev = lib.swmi_local_full_affine_device
    assert dev(P(a), 0, P(b), 64, 2, P(sm), 3, 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 16385, 2, P(sm), 3, 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 3, 200, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 3, 1, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    ms = ctypes.c_float()
    timer = lib.swmi_local_full_affine_time_device
    assert timer(P(a), 64, P(b), 0, 2, P(sm), 3, 1, P(sc), P(ends), None, None, None, 3, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    assert timer(P(a), 64, P(b), 64, 2, P(sm), 3, 1, P(sc), P(ends), None, None, None, 0, ctypes.byref(ms)) == swmi_mod.ERR_INVALID_ARGUMENT
    # n = 0 is a no-op that needs no device, on both entries
    assert call(n=0) == 0 and call(n=0, s1=None, s2=None, scores=None, e=None, moves=None, steps=None) == 0
    assert dev(None, 64, None, 64, 0, P(sm), 3, 1, None, None, None, None, None) == 0
    out = swmi_mod.local_full_affine(np.zeros((0, 5), np.uint8), np.zeros((0, 9), np.uint8), sm, 3, 1)
    assert out[0].shape == (0,) and out[1].shape == (0, 4)
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_slices_for(swmi_mod):
    """Values worked out by hand from the budget: a traceback slice is what 256 alignments of 16384 x 16384 take."""
    full = lambda n, tb=True: swmi_mod.local_full_affine_slices_for(n, 16384, 16384, tb)  # noqa: E731
    assert full(0) == [] and full(1) == [1] and full(256) == [256] and full(257) == [256, 1]
    assert full(1000) == [256, 256, 256, 232]
    # ends-only: 256 MiB over inputs and results, 16384 + 16384 bytes of bases, 4 of score, 16 of ends
    per = 16384 + 16384 + 4 + 16
    sizes = full(100000, False)
    assert sum(sizes) == 100000 and sizes[0] == (256 << 20) // per == 8187 and all(s <= sizes[0] for s in sizes)
    # traceback at 4096 x 4096: 4 waves x 1040 trips (130 chunks of 8) x 256 qwords of codes, 256 move words, against 256
    # full-size alignments of 16 waves x 4112 trips (514 chunks) x 256 qwords and 1024 move words
    one = 4096 + 4096 + 4 + 16 + 4 * 1040 * 256 * 8 + 256 * 8 + 4
    assert one == per_alignment(4096, 4096, True)
    budget = 256 * (16384 + 16384 + 4 + 16 + 16 * 4112 * 256 * 8 + 1024 * 8 + 4)
    assert swmi_mod.local_full_affine_slices_for(10 ** 6, 4096, 4096)[0] == budget // one
    assert swmi_mod.local_full_affine_slices_for(3 * (1 << 20) + 5, 1, 1, False) == [1 << 20] * 3 + [5]
    for len1, len2 in ((1, 1), (63, 65), (1000, 1000), (4096, 777), (16384, 1)):
        for tb in (True, False):
            for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
                s = swmi_mod.local_full_affine_slices_for(n, len1, len2, tb)
                assert sum(s) == n and all(x >= 1 for x in s) and all(x == s[0] for x in s[:-1]) and all(x <= 1 << 20 for x in s)
    for len1, len2 in ((0, 5), (5, 16385), (16385, 5), (5, 0)):
        assert swmi_mod.local_full_affine_slices_for(10, len1, len2) == []
