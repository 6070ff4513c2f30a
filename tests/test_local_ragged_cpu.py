"""The ragged local aligners' host-only parts (swmi_local_ragged_move_offsets, swmi_local_ragged_slices_for, argument checks
and the Python forms), no device needed."""
import ctypes

import numpy as np
import pytest

from conftest import match_matrix
from local_support import move_words

MAX = 16384
LINEAR_BUDGET = 256 << 20


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


def _code_words(len1, affine):
    trips = (len1 + 15 + 7) // 8
    return trips * (8 if affine else 4) * 16


def _bytes(len1, affine, tb):
    """device bytes one alignment of a ragged slice takes (include/swmi.h: inputs, slot, results, codes, moves, count)"""
    b = len1 + 128 + 20 + 20
    if tb:
        b += 4 * _code_words(len1, affine) + 8 * move_words(len1) + 4
    return b


def _affine_budget():
    return 4096 * (MAX + 128 + 4 + 16 + 4 * _code_words(MAX, True) + 8 * move_words(MAX) + 4)


def test_move_offsets_are_prefix_sums(swmi_mod):
    rng = np.random.default_rng(1)
    lens = [0, 1, 31, 32, 33, 127, 128, 129, MAX] + list(rng.integers(0, MAX + 1, 500))
    off = _off(lens) + np.uint64(7)                   # offsets need not start at 0
    mo = swmi_mod.local_ragged_move_offsets(off)
    want = np.concatenate([[0], np.cumsum([move_words(int(x)) for x in lens])])
    assert np.array_equal(mo, want.astype(np.uint64))
    assert all(move_words(int(x)) % 2 == 0 for x in lens)    # 16-byte rows: every alignment's moves stay 16-byte aligned


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("tb", [True, False])
def test_slices_cover_the_batch_in_order_within_budget(swmi_mod, affine, tb):
    rng = np.random.default_rng(2 + affine + 2 * tb)
    lens = [int(x) for x in rng.integers(0, MAX + 1, 20000)]
    off = _off(lens)
    sizes = swmi_mod.local_ragged_slices_for(off, affine=affine, traceback=tb)
    assert sum(sizes) == len(lens) and min(sizes) >= 1 and max(sizes) <= 1 << 20
    budget = _affine_budget() if (affine and tb) else LINEAR_BUDGET
    at = 0
    for s in sizes:
        b = sum(_bytes(L, affine, tb) for L in lens[at:at + s])
        assert b <= budget
        if at + s < len(lens):                        # the longest prefix: one more would not fit
            assert b + _bytes(lens[at + s], affine, tb) > budget
        at += s


def test_a_slice_holds_at_most_2_20_alignments(swmi_mod):
    off = _off([0] * ((1 << 20) + 5))
    assert swmi_mod.local_ragged_slices_for(off, affine=False, traceback=False) == [1 << 20, 5]


def test_a_longest_alignment_gets_a_slice_of_its_own_when_it_must(swmi_mod):
    """Linear traceback: a slice holds 480 alignments of 16384, so the 481st starts a slice; an alignment after a full slice
    of shorter ones starts one too."""
    per = LINEAR_BUDGET // _bytes(MAX, False, True)
    sizes = swmi_mod.local_ragged_slices_for(_off([MAX] * (per + 1)), affine=False, traceback=True)
    assert sizes == [per, 1]
    short = LINEAR_BUDGET // _bytes(1000, False, True)
    sizes = swmi_mod.local_ragged_slices_for(_off([1000] * short + [MAX]), affine=False, traceback=True)
    assert sizes[-1] == 1 and sum(sizes) == short + 1


def test_empty_batch(swmi_mod):
    assert swmi_mod.local_ragged_slices_for(np.zeros(1, np.uint64)) == []
    sc, ends, moves, mo, steps = swmi_mod.local_align_ragged([], np.zeros((0, 128), np.uint8), match_matrix(1, -1), 1)
    assert len(sc) == 0 and ends.shape == (0, 4) and len(moves) == 0 and list(mo) == [0]


def _raw(swmi_mod):
    return swmi_mod.load()


def test_argument_errors_need_no_device(swmi_mod):
    """Every argument error of the four entries and the two helpers, in a process with no GPU bound."""
    lib = _raw(swmi_mod)
    sm = np.ascontiguousarray(match_matrix(1, -1), np.int8)
    s1 = np.zeros(64, np.uint8)
    s2 = np.zeros((4, 128), np.uint8)
    out = np.zeros(64, np.int64)
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    bad_long = np.array([0, 3, 3 + MAX + 1, 3 + MAX + 2, 3 + MAX + 3], np.uint64)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN

    def lin(off, gap=1, s1p=p(s1), mv=p(out), st=p(out), n=4, smp=p(sm)):
        return lib.swmi_local_align_ragged(s1p, p(off), p(s2), n, smp, gap, p(out), p(out), mv, st)

    def aff(off, go=1, ge=1, s1p=p(s1), mv=p(out), st=p(out), n=4):
        return lib.swmi_local_align_affine_ragged(s1p, p(off), p(s2), n, p(sm), go, ge, p(out), p(out), mv, st)

    def lin_dev(off, gap=1, mv=p(out), st=p(out), n=4):
        return lib.swmi_local_align_ragged_device(p(s1), p(off), p(s2), n, p(sm), gap, p(out), p(out), mv, st, None)

    def aff_dev(off, go=1, ge=1, mv=p(out), st=p(out), n=4):
        return lib.swmi_local_align_affine_ragged_device(p(s1), p(off), p(s2), n, p(sm), go, ge, p(out), p(out), mv, st, None)

    for f in (lin, aff, lin_dev, aff_dev):
        assert f(bad_dec) == INV
        assert f(bad_long) == INV
        assert f(None) == INV
        assert f(good, mv=None) == INV
        assert f(good, st=None) == INV
        assert f(bad_dec, n=0) == 0                     # n = 0: a no-op
    assert lin(good, gap=-1) == DOM and lin_dev(good, gap=-1) == DOM
    assert lin(good, smp=None) == INV
    assert lin(good, s1p=None) == INV and aff(good, s1p=None) == INV
    for go, ge in ((-1, 0), (0, 128), (128, 1), (3, -2)):
        assert aff(good, go, ge) == DOM and aff_dev(good, go, ge) == DOM
    mo = np.zeros(5, np.uint64)
    assert lib.swmi_local_ragged_move_offsets(p(bad_dec), 4, p(mo)) == INV
    assert lib.swmi_local_ragged_move_offsets(p(bad_long), 4, p(mo)) == INV
    assert lib.swmi_local_ragged_move_offsets(p(good), 4, None) == INV
    assert lib.swmi_local_ragged_move_offsets(p(good), 4, p(mo)) == 0
    assert lib.swmi_local_ragged_slices_for(p(bad_dec), 4, 0, 1, None, 0) == 0
    assert lib.swmi_local_ragged_slices_for(p(bad_long), 4, 1, 1, None, 0) == 0
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_align_ragged((s1, bad_dec), s2, sm, 1)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_align_affine_ragged((s1, bad_dec), s2, sm, 1, 1, traceback=False)


def test_list_and_pair_forms_give_the_same_buffers(swmi_mod):
    rng = np.random.default_rng(5)
    parts = [rng.integers(0, 4, int(L), dtype=np.uint8) for L in (0, 5, 0, 17, 300)]
    cat, off = swmi_mod._ragged_seq1s(parts)
    assert list(off) == [0, 0, 5, 5, 22, 322]
    assert np.array_equal(cat, np.concatenate(parts))
    cat2, off2 = swmi_mod._ragged_seq1s((np.concatenate(parts), off))
    assert np.array_equal(cat, cat2) and np.array_equal(off, off2)
    with pytest.raises(ValueError):
        swmi_mod._ragged_seq1s((cat[:10], off))
    with pytest.raises(ValueError):
        swmi_mod.local_align_ragged(parts, np.zeros((4, 128), np.uint8), match_matrix(1, -1), 1)
