"""The ragged any-length local aligners' host-only parts (swmi_local_full_ragged_move_offsets,
swmi_local_full_ragged_slices_for, argument checks and the Python forms), no device needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_full_affine_support import code_qwords
from local_full_support import move_words

MAX = 16384
ENDS_ONLY_BUDGET = 256 << 20
SLOT = 48                                   # sizeof(TileWork)
ENTRIES = ["swmi_local_full_ragged", "swmi_local_full_affine_ragged", "swmi_local_full_ragged_device",
           "swmi_local_full_affine_ragged_device", "swmi_local_full_ragged_move_offsets", "swmi_local_full_ragged_slices_for"]


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


def _bytes(len1, len2, affine, tb):
    """device bytes one alignment of a ragged slice takes (include/swmi.h: inputs, slot, results, codes, moves, steps)"""
    b = len1 + len2 + SLOT + 20
    if tb:
        words = code_qwords(len1, len2) if len1 and len2 else 0       # one code word per lane and step: a dword, affine a qword
        b += (8 if affine else 4) * words + 8 * move_words(len1, len2) + 4
    return b


def _fixed_budget(affine):
    """what 256 alignments of 16384 x 16384 take in the fixed-length aligner's traceback slice"""
    return 256 * (2 * MAX + 4 + 16 + (8 if affine else 4) * code_qwords(MAX, MAX) + 8 * move_words(MAX, MAX) + 4)


def test_header_declares_and_library_exports_the_entries(swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+\w+\s+%s\(" % name, header), name
        assert getattr(lib, name) is not None
    assert "#define SWMI_VERSION 300" in header


def test_move_offsets_are_prefix_sums_of_the_macro(swmi_mod):
    rng = np.random.default_rng(1)
    pairs = [(0, 0), (0, 7), (7, 0), (1, 1), (31, 1), (1, 32), (MAX, MAX), (MAX, 0)]
    pairs += [(int(x), int(y)) for x, y in rng.integers(0, MAX + 1, (500, 2))]
    off1 = _off([p[0] for p in pairs]) + np.uint64(7)            # offsets need not start at 0
    off2 = _off([p[1] for p in pairs]) + np.uint64(3)
    mo = swmi_mod.local_full_ragged_move_offsets(off1, off2)
    want = np.concatenate([[0], np.cumsum([move_words(x, y) for x, y in pairs])])
    assert np.array_equal(mo, want.astype(np.uint64))
    assert move_words(0, 0) == 0 and move_words(1, 0) == 2 and all(move_words(x, y) % 2 == 0 for x, y in pairs)     # 16-byte rows


def test_a_slice_holds_at_most_2_20_alignments(swmi_mod):
    n = (1 << 20) + 5
    rng = np.random.default_rng(2)
    off1, off2 = _off(rng.integers(0, 5, n)), _off(rng.integers(0, 5, n))
    for affine in (False, True):
        assert swmi_mod.local_full_ragged_slices_for(off1, off2, affine=affine, traceback=False) == [1 << 20, 5]


@pytest.mark.parametrize("affine", [False, True])
def test_ends_only_slices_are_the_longest_runs_within_256_mib(swmi_mod, affine):
    rng = np.random.default_rng(3)
    l1 = [int(x) for x in rng.integers(0, MAX + 1, 40000)]
    l2 = [int(x) for x in rng.integers(0, MAX + 1, 40000)]
    sizes = swmi_mod.local_full_ragged_slices_for(_off(l1), _off(l2), affine=affine, traceback=False)
    assert len(sizes) >= 2 and sum(sizes) == len(l1) and min(sizes) >= 1
    at = 0
    for s in sizes:
        b = sum(_bytes(x, y, affine, False) for x, y in zip(l1[at:at + s], l2[at:at + s]))
        assert b <= ENDS_ONLY_BUDGET
        if at + s < len(l1):                            # the longest run: one more would not fit
            assert b + _bytes(l1[at + s], l2[at + s], affine, False) > ENDS_ONLY_BUDGET
        at += s


@pytest.mark.parametrize("affine", [False, True])
def test_traceback_slices_fit_the_fixed_aligners_budget(swmi_mod, affine):
    """256 alignments of 16384 x 16384 fill the fixed-length aligner's slice; their slots are counted too, so the ragged slice
    holds 255, and a single alignment larger than the remainder of a slice still forms a slice."""
    budget = _fixed_budget(affine)
    assert swmi_mod.local_full_ragged_slices_for(_off([MAX] * 300), _off([MAX] * 300), affine=affine) == [255, 45]
    big = _bytes(MAX, MAX, affine, True)
    small = _bytes(2000, 1000, affine, True)
    n_small = (budget - big // 2) // small                   # leaves less than one big alignment's room
    l1, l2 = [2000] * n_small + [MAX, 5], [1000] * n_small + [MAX, 5]
    sizes = swmi_mod.local_full_ragged_slices_for(_off(l1), _off(l2), affine=affine)
    assert sizes == [n_small, 2]
    assert n_small * small <= budget < n_small * small + big


def test_empty_batch(swmi_mod):
    one = np.zeros(1, np.uint64)
    assert swmi_mod.local_full_ragged_slices_for(one, one) == []
    sc, ends, moves, mo, steps = swmi_mod.local_full_ragged([], [], match_matrix(1, -1), 1)
    assert len(sc) == 0 and ends.shape == (0, 4) and len(moves) == 0 and list(mo) == [0] and len(steps) == 0
    sc, ends, moves, mo, steps = swmi_mod.local_full_affine_ragged([], [], match_matrix(1, -1), 2, 1, traceback=False)
    assert len(sc) == 0 and moves is None and mo is None and steps is None


def test_argument_errors_need_no_device(swmi_mod):
    """Every argument error of the four entries and the two helpers, in a process with no GPU bound."""
    lib = swmi_mod.load()
    sm = np.ascontiguousarray(match_matrix(1, -1), np.int8)
    s1 = np.zeros(64, np.uint8)
    s2 = np.zeros(64, np.uint8)
    out = np.zeros(64, np.int64)
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    bad_long = np.array([0, 3, 3 + MAX + 1, 3 + MAX + 2, 3 + MAX + 3], np.uint64)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN

    def lin(o1, o2, gap=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_local_full_ragged(s1p, p(o1), s2p, p(o2), n, smp, gap, sc, en, mv, st)

    def aff(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_local_full_affine_ragged(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st)

    def lin_dev(o1, o2, gap=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_local_full_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, gap, sc, en, mv, st, None)

    def aff_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_local_full_affine_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st, None)

    for f in (lin, aff, lin_dev, aff_dev):
        for bad in (bad_dec, bad_long, None):
            assert f(bad, good) == INV and f(good, bad) == INV
        assert f(good, good, mv=None) == INV
        assert f(good, good, st=None) == INV
        for name in ("s1p", "s2p", "sc", "en", "smp"):
            assert f(good, good, **{name: None}) == INV, name
        assert f(bad_dec, None, n=0) == 0                       # n = 0: a no-op
        assert f(bad_dec, None, n=0, mv=None, st=None) == 0
    assert lin(good, good, gap=-1) == DOM and lin_dev(good, good, gap=-1) == DOM
    for go, ge in ((-1, 0), (0, 128), (128, 1), (3, -2)):
        assert aff(good, good, go, ge) == DOM and aff_dev(good, good, go, ge) == DOM
    mo = np.zeros(5, np.uint64)
    for bad in (bad_dec, bad_long, None):
        assert lib.swmi_local_full_ragged_move_offsets(p(bad), p(good), 4, p(mo)) == INV
        assert lib.swmi_local_full_ragged_move_offsets(p(good), p(bad), 4, p(mo)) == INV
        assert lib.swmi_local_full_ragged_slices_for(p(bad), p(good), 4, 0, 1, None, 0) == 0
        assert lib.swmi_local_full_ragged_slices_for(p(good), p(bad), 4, 1, 1, None, 0) == 0
    assert lib.swmi_local_full_ragged_move_offsets(p(good), p(good), 4, None) == INV
    assert lib.swmi_local_full_ragged_move_offsets(p(good), p(good), 4, p(mo)) == 0
    assert lib.swmi_local_full_ragged_move_offsets(p(good), p(good), 0, p(mo)) == 0 and mo[0] == 0
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full_ragged((s1, bad_dec), (s2, good), sm, 1)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full_affine_ragged((s1, good), (s2, bad_dec), sm, 1, 1, traceback=False)


def test_the_binding_rejects_what_ctypes_would_wrap(swmi_mod):
    """ctypes converts to int8 / int without an overflow check: gap 256 would align as gap 0, gap_open 2^32 + 1 as 1, a matrix
    entry of 300 as 44."""
    parts = [np.zeros(3, np.uint8)]
    sm = match_matrix(1, -1)
    wide = np.full(16, 300, np.int64)
    with pytest.raises(swmi_mod.SwmiError) as e:
        swmi_mod.local_full_ragged(parts, parts, sm, 256)
    assert e.value.code == swmi_mod.ERR_DOMAIN
    for go, ge in ((2**32 + 1, 1), (1, 2**32 + 1), (-2**32, 1)):
        with pytest.raises(swmi_mod.SwmiError) as e:
            swmi_mod.local_full_affine_ragged(parts, parts, sm, go, ge)
        assert e.value.code == swmi_mod.ERR_DOMAIN
        with pytest.raises(swmi_mod.SwmiError) as e:
            swmi_mod.local_full_affine_ragged_device(16, [0, 3], 16, [0, 3], sm, go, ge, 16, 16)
        assert e.value.code == swmi_mod.ERR_DOMAIN
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full_ragged(parts, parts, wide, 1)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full_ragged_device(16, [0, 3], 16, [0, 3], sm, 300, 16, 16)


def test_list_and_pair_forms_and_mismatched_sides(swmi_mod):
    rng = np.random.default_rng(5)
    parts = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (0, 5, 0, 17, 300)]
    cat1, off1, cat2, off2 = swmi_mod._ragged_pair(parts, (np.concatenate(parts), _off([len(x) for x in parts])))
    assert list(off1) == [0, 0, 5, 5, 22, 322] and np.array_equal(off1, off2) and np.array_equal(cat1, cat2)
    with pytest.raises(ValueError):
        swmi_mod.local_full_ragged(parts, parts[:4], match_matrix(1, -1), 1)
    with pytest.raises(ValueError):
        swmi_mod.local_full_ragged_move_offsets(off1, off2[:-1])
    with pytest.raises(ValueError):
        swmi_mod.local_full_ragged_slices_for(off1[:0], off2[:0])
