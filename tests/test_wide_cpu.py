"""The wide-alphabet aligners' host-only parts, no device needed (libswmi_wide.so, include/swmi_wide.h, swmi.wide): the C
restatement tests/native/wide_affine_oracle.c against the 4-letter restatements on DNA letters with an embedded matrix (every
field and move, all 16 masks) and against an independent numpy Gotoh on 32-letter inputs with an asymmetric int8 matrix; the
header and the library's symbols; every refusal with code and text in a process with no GPU bound; swmi_wide_slices_for on
hand-checkable offsets; the module swmi.wide.  Every comparison is exact integer equality."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG, ROOT
from global_full_affine_support import GlobalFullAffineOracle
from local_full_affine_support import LocalFullAffineOracle
from local_support import random_matrix
from wide_support import (ALL_MASKS, GLOBAL, LOCAL, WideOracle, assert_same, asymmetric_matrix, embed_dna, inputs, move_offsets, moves_of,
                          numpy_gotoh)

ENTRIES = ["swmi_wide_local", "swmi_wide_global", "swmi_wide_local_device", "swmi_wide_global_device", "swmi_wide_slices_for",
           "swmi_wide_time_device", "swmi_wide_release_workspaces", "swmi_wide_last_error", "swmi_wide_version"]
MAX1, MAX2 = 16384, 4096


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


@pytest.fixture(scope="module")
def woracle(tmp_path_factory):
    return WideOracle(tmp_path_factory.mktemp("wide_oracle"))


@pytest.fixture(scope="module")
def wide(swmi_mod):
    swmi_mod.wide.load()
    return swmi_mod.wide


def _fixed_as_ragged(a, b, r, traceback=True):
    """A fixed-shape restatement's (scores, ends, moves[n, words], steps) in the ragged layout."""
    mo = move_offsets(a, b)
    moves = np.zeros(int(mo[-1]) + 2, np.uint64)
    for k in range(len(a)):
        moves[int(mo[k]):int(mo[k]) + r[2].shape[1]] = r[2][k]
    return r[0], r[1], moves, mo, r[3]


@pytest.mark.parametrize("shape", [(1, 1), (7, 33), (40, 17), (64, 64), (33, 129)])
def test_restatement_equals_the_dna_restatements_on_embedded_matrices(woracle, tmp_path_factory, shape):
    lo = LocalFullAffineOracle(tmp_path_factory.mktemp("wl"))
    go = GlobalFullAffineOracle(tmp_path_factory.mktemp("wg"))
    len1, len2 = shape
    a, b = inputs([shape] * 9, seed=len1 * 131 + len2, letters=4, junk=False)
    A, B = np.stack(a).reshape(9, len1), np.stack(b).reshape(9, len2)
    for sm16, gap_open, gap_extend in [(random_matrix(5), 3, 1), (random_matrix(6), 0, 0), (random_matrix(7), 2, 5),
                                       (np.full(16, -128, np.int8), 127, 127), (np.full(16, 127, np.int8), 1, 0)]:
        sm32 = embed_dna(sm16)
        assert_same(woracle.align(LOCAL, a, b, sm32, gap_open, gap_extend), _fixed_as_ragged(a, b, lo.align(A, B, sm16, gap_open, gap_extend)),
                    ("local", shape, gap_open, gap_extend))
        for mask in ALL_MASKS:
            assert_same(woracle.align(GLOBAL, a, b, sm32, gap_open, gap_extend, mask),
                        _fixed_as_ragged(a, b, go.align(A, B, sm16, gap_open, gap_extend, mask)), ("global", shape, mask, gap_open, gap_extend))
    ends_only = woracle.align(LOCAL, a, b, embed_dna(random_matrix(5)), 3, 1, traceback=False)
    assert ends_only[2] is None and (ends_only[1][:, 2:] == -1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_an_independent_numpy_gotoh_on_32_letters(woracle, seed):
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(1, 41)), int(rng.integers(1, 41))) for _ in range(10)] + [(40, 40), (1, 40), (40, 1), (0, 5), (5, 0), (0, 0)]
    a, b = inputs(shapes, seed=seed + 50)
    for sm, gap_open, gap_extend in [(asymmetric_matrix(seed), 5, 2), (asymmetric_matrix(seed + 10, -6, 9), 3, 1),
                                     (asymmetric_matrix(seed + 20, -3, 4), 0, 0), (asymmetric_matrix(seed + 30, -6, 9), 1, 4)]:
        for kind, masks in ((LOCAL, [0]), (GLOBAL, ALL_MASKS)):
            for mask in masks:
                got = woracle.align(kind, a, b, sm, gap_open, gap_extend, mask)
                for k in range(len(a)):
                    score, ends, moves = numpy_gotoh(kind, a[k], b[k], sm, gap_open, gap_extend, mask)
                    what = (kind, mask, shapes[k], gap_open, gap_extend)
                    assert int(got[0][k]) == score and list(got[1][k]) == ends, (what, int(got[0][k]), score, list(got[1][k]), ends)
                    assert moves_of(got, k) == moves, what


def test_header_declares_and_library_exports_the_entries(wide):
    with open(os.path.join(ROOT, "include", "swmi_wide.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert '#include "swmi.h"' in header
    for absent in ("swmi_wide_move_offsets", "swmi_wide_expand_moves"):       # one layout, one expander: libswmi.so's
        assert absent not in header
    lib = os.path.join(PKG, "lib", "libswmi_wide.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    # what it takes from libswmi.so: the move layout's one function, nothing else
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    taken = {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}
    assert taken <= {"swmi_local_full_ragged_move_offsets", "swmi_last_error", "swmi_local_full_expand_moves"}, taken
    assert wide.version() == 300


def test_every_refusal_works_with_no_device(wide, swmi_mod):
    lib = wide.load()
    sm = np.zeros(1024, np.int8)
    s1, s2 = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    out = np.zeros(64, np.int64)
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    long1 = np.array([0, 3, 3 + MAX1 + 1, 3 + MAX1 + 2, 3 + MAX1 + 3], np.uint64)      # a length of 16385
    long2 = np.array([0, 3, 3 + MAX2 + 1, 3 + MAX2 + 2, 3 + MAX2 + 3], np.uint64)      # a length of 4097
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT

    def local(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_local(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st)

    def glob(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_global(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st)

    def local_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_local_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st, None)

    def glob_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_global_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st, None)

    for f in (local, glob, local_dev, glob_dev):
        assert f(long1, good) == INV and "seq1_offsets: sequence 1 has length 16385 > 16384" in wide.last_error()
        assert f(good, long2) == INV and "seq2_offsets: sequence 1 has length 4097 > 4096" in wide.last_error()
        assert f(bad_dec, good) == INV and "seq1_offsets decrease at 1" in wide.last_error()
        assert f(good, bad_dec) == INV and "seq2_offsets decrease at 1" in wide.last_error()
        assert f(None, good) == INV and "seq1_offsets is NULL" in wide.last_error()
        assert f(good, None) == INV and "seq2_offsets is NULL" in wide.last_error()
        assert f(good, good, mv=None) == INV and "moves and steps" in wide.last_error()
        assert f(good, good, st=None) == INV and "moves and steps" in wide.last_error()
        for name in ("s1p", "s2p", "sc", "en"):
            assert f(good, good, **{name: None}) == INV and "NULL buffer" in wide.last_error(), name
        assert f(good, good, smp=None) == INV and "score_matrix is NULL" in wide.last_error()
        for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
            assert f(good, good, go=go, ge=ge) == DOM and "outside [0,127]" in wide.last_error()
        # n = 0 returns before the buffers and the offsets are looked at, but after the matrix, the gaps and moves / steps
        assert f(bad_dec, None, n=0, s1p=None) == 0
        assert f(good, good, n=0, go=200) == DOM and f(good, good, n=0, mv=None) == INV
        # the order: gaps before the moves / steps pair, that before the buffers, those before the offsets
        assert f(bad_dec, good, go=-1, mv=None) == DOM and f(bad_dec, good, mv=None, sc=None) == INV and "moves and steps" in wide.last_error()
        assert f(bad_dec, good, sc=None) == INV and "NULL buffer" in wide.last_error()
    for f in (glob, glob_dev):
        assert f(good, good, mask=16) == INV and "free_ends 16 above 15" in wide.last_error()
        assert f(good, good, mask=16, go=-1) == INV                       # the mask comes first
    for f in (local_dev, glob_dev):
        assert f(good, good, sc=p(out) + 8) == ALN and "16-byte aligned" in wide.last_error()
    ms = ctypes.c_float()
    t = lambda kind=0, iters=1, n=4, ms=ctypes.byref(ms): lib.swmi_wide_time_device(kind, p(s1), p(good), p(s2), p(good), n, p(sm), 1, 1, 0,   # noqa: E731
                                                                                     p(out), p(out), None, None, None, iters, ms)
    assert t(kind=2) == INV and t(iters=0) == INV and t(n=0) == INV and t(ms=None) == INV
    # the Python layer: what ctypes would wrap raises, as elsewhere
    seqs = [np.zeros(3, np.uint8)]
    with pytest.raises(swmi_mod.SwmiError) as e:
        wide.local(seqs, seqs, sm, 2**32 + 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wide.global_(seqs, seqs, np.full(1024, 300), 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wide.global_(seqs, seqs, sm, 1, 1, free_ends=-1)
    assert e.value.code == INV
    with pytest.raises(swmi_mod.SwmiError) as e:
        wide.local([np.zeros(3, np.uint8)], [np.zeros(MAX2 + 1, np.uint8)], sm, 1, 1)
    assert e.value.code == INV and "4097" in str(e.value)
    with pytest.raises(ValueError):
        wide.local(seqs, seqs, np.zeros(16, np.int8), 1, 1)
    # an empty batch needs no device
    r = wide.local([], [], sm, 1, 1)
    assert len(r[0]) == 0 and r[1].shape == (0, 4)


def test_slices_for_on_hand_checkable_offsets(wide):
    lib = wide.load()
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    long2 = np.array([0, 3, 3 + MAX2 + 1, 3 + MAX2 + 2, 3 + MAX2 + 3], np.uint64)
    ok2 = np.array([0, 3, 3 + MAX2, 3 + MAX2 + 2, 3 + MAX2 + 3], np.uint64)
    for tb in (0, 1):
        for bad in (bad_dec, None):
            assert lib.swmi_wide_slices_for(p(bad), p(good), 4, tb, None, 0) == 0
            assert lib.swmi_wide_slices_for(p(good), p(bad), 4, tb, None, 0) == 0
        assert lib.swmi_wide_slices_for(p(good), p(long2), 4, tb, None, 0) == 0
        assert lib.swmi_wide_slices_for(p(long2), p(good), 4, tb, None, 0) == 1         # 4097 is a fine seq1
        assert lib.swmi_wide_slices_for(p(good), p(ok2), 4, tb, None, 0) == 1
        sizes = (ctypes.c_size_t * 2)(99, 99)
        assert lib.swmi_wide_slices_for(p(good), p(good), 4, tb, sizes, 2) == 1
        assert list(sizes) == [4, 99]
    one = np.zeros(1, np.uint64)
    assert wide.slices_for(one, one) == []
    # the count cap: a slice holds at most 2^20 alignments
    n = (1 << 20) + 5
    rng = np.random.default_rng(2)
    assert wide.slices_for(_off(rng.integers(0, 5, n)), _off(rng.integers(0, 5, n)), traceback=False) == [1 << 20, 5]
    # the traceback budget is what 256 alignments of the largest shape take, slots included: 300 of them are 256 + 44
    assert wide.slices_for(_off([MAX1] * 300), _off([MAX2] * 300)) == [256, 44]
    # ... and smaller ones fill it by bytes: per alignment len1 + len2 + 48 (slot) + 20 (results) + 4 (steps) + 8 x (codes +
    # moves); 16384 x 1024 has a quarter of the codes
    def bytes_tb(len1, len2):
        trips = ((len1 + 63 + 31) // 32) * 8
        codes = ((len2 + 1023) // 1024) * trips * 256
        return len1 + len2 + 48 + 20 + 4 + 8 * (codes + ((((len1 + len2 + 31) // 32) + 1) & ~1))
    per_slice = 256 * bytes_tb(MAX1, MAX2) // bytes_tb(MAX1, 1024)
    assert 1000 < per_slice < 1100
    assert wide.slices_for(_off([MAX1] * 2100), _off([1024] * 2100)) == [per_slice, per_slice, 2100 - 2 * per_slice]
    # ends-only: 256 MiB of inputs, slots and results
    per_slice = (256 << 20) // (MAX1 + MAX2 + 48 + 20)
    assert wide.slices_for(_off([MAX1] * (per_slice + 7)), _off([MAX2] * (per_slice + 7)), traceback=False) == [per_slice, 7]


def test_module_is_a_submodule_with_docstrings(swmi_mod):
    wide = swmi_mod.wide
    assert isinstance(wide, types.ModuleType) and wide.__name__ == "swmi.wide" and wide.__doc__
    public = ["local", "global_", "local_device", "global_device", "slices_for", "time_device", "release_workspaces", "match_matrix",
              "embed_dna", "last_error", "version", "load"]
    for name in public:
        fn = getattr(wide, name)
        assert inspect.isfunction(fn) and fn.__module__ == "swmi.wide" and fn.__doc__, name
    for name in ("global_", "local_device", "global_device", "embed_dna", "time_device"):
        assert not hasattr(swmi_mod, name), name
    top = [n for n, f in vars(swmi_mod).items() if inspect.isfunction(f) and f.__module__ == "swmi" and not n.startswith("_")]
    assert len(top) == 94
    mm = wide.match_matrix(5, -4).reshape(32, 32)
    assert mm.dtype == np.int8 and (np.diag(mm) == 5).all() and (mm[~np.eye(32, dtype=bool)] == -4).all()
    e = wide.embed_dna(np.arange(16)).reshape(32, 32)
    assert e.dtype == np.int8 and np.array_equal(e[:4, :4], np.arange(16).reshape(4, 4)) and (e[4:] == -128).all() and (e[:, 4:] == -128).all()
    with pytest.raises(swmi_mod.SwmiError):
        wide.embed_dna(np.full(16, 200))
