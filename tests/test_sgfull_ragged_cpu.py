"""The ragged exact semi-global aligners' host-only parts, no device needed: the header and the library's symbols (every symbol
exported before them, tests/golden/exports_before_semiglobal_ragged.txt, plus exactly the five new ones), every argument error
of the four entries and n = 0 in a process with no GPU bound, swmi_semiglobal_full_ragged_slices_for on hand-checkable offsets,
what swmi/semiglobal_ragged.py hands to the C ABI (two ends per alignment), and the package's pinned top-level API."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from test_python_bindings import DCT, DEN, DMV, DSC, D1, D2, SM, STREAM, Recorder, _api_snapshot, _check_slices, _ptr, _public_functions

MAX = 16384
ENTRIES = ["swmi_semiglobal_full_ragged", "swmi_semiglobal_full_affine_ragged", "swmi_semiglobal_full_ragged_device",
           "swmi_semiglobal_full_affine_ragged_device", "swmi_semiglobal_full_ragged_slices_for"]


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


def test_header_declares_and_library_exports_the_entries(swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+\w+\s+%s\(" % name, header), name
    assert "#define SWMI_VERSION 300" in header
    assert "swmi_semiglobal_full_ragged_move_offsets" not in header     # one layout, one function: the local family's
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libswmi.so")], stdout=subprocess.PIPE, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "tests", "golden", "exports_before_semiglobal_ragged.txt")) as fh:
        before = fh.read().split()
    assert len(before) > 140 and not set(before) & set(ENTRIES)
    assert exported == set(before) | set(ENTRIES), sorted(exported ^ (set(before) | set(ENTRIES)))


def test_slices_for_on_hand_checkable_offsets(swmi_mod):
    lib = swmi_mod.load()
    sr = swmi_mod.semiglobal_ragged
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    bad_long = np.array([0, 3, 3 + MAX + 1, 3 + MAX + 2, 3 + MAX + 3], np.uint64)          # a length of 16385
    ok_long = np.array([0, 3, 3 + MAX, 3 + MAX + 2, 3 + MAX + 3], np.uint64)               # 16384 is taken
    for affine in (0, 1):
        for tb in (0, 1):
            for bad in (bad_dec, bad_long, None):
                assert lib.swmi_semiglobal_full_ragged_slices_for(p(bad), p(good), 4, affine, tb, None, 0) == 0
                assert lib.swmi_semiglobal_full_ragged_slices_for(p(good), p(bad), 4, affine, tb, None, 0) == 0
            assert lib.swmi_semiglobal_full_ragged_slices_for(p(good), p(ok_long), 4, affine, tb, None, 0) == 1
            sizes = (ctypes.c_size_t * 2)(99, 99)
            assert lib.swmi_semiglobal_full_ragged_slices_for(p(good), p(good), 4, affine, tb, sizes, 2) == 1
            assert list(sizes) == [4, 99]
    one = np.zeros(1, np.uint64)
    assert sr.semiglobal_full_ragged_slices_for(one, one) == []
    # the count cap: a slice holds at most 2^20 alignments
    n = (1 << 20) + 5
    rng = np.random.default_rng(2)
    off1, off2 = _off(rng.integers(0, 5, n)), _off(rng.integers(0, 5, n))
    for affine in (False, True):
        assert sr.semiglobal_full_ragged_slices_for(off1, off2, affine=affine, traceback=False) == [1 << 20, 5]
    # the byte budget is the fixed-length aligner's: 256 alignments of 16384 x 16384 fill its traceback slice, and the slots are
    # counted too, so the ragged slice holds 255 (as in the other two ragged families)
    for affine in (False, True):
        assert sr.semiglobal_full_ragged_slices_for(_off([MAX] * 300), _off([MAX] * 300), affine=affine) == [255, 45]
    assert swmi_mod.semiglobal_full_slices_for(300, MAX, MAX) == [256, 44]
    assert swmi_mod.semiglobal_full_affine_slices_for(300, MAX, MAX) == [256, 44]


def test_argument_errors_and_an_empty_batch_need_no_device(swmi_mod):
    """Every argument error of the four entries, and n = 0, in a process with no GPU bound; the checks' order: matrix and gaps,
    moves / lengths, n = 0, buffers, offsets."""
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

    def lin(o1, o2, gap=1, s1p=p(s1), s2p=p(s2), mv=p(out), ln=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_semiglobal_full_ragged(s1p, p(o1), s2p, p(o2), n, smp, gap, sc, en, mv, ln)

    def aff(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), ln=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_semiglobal_full_affine_ragged(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, ln)

    def lin_dev(o1, o2, gap=1, s1p=p(s1), s2p=p(s2), mv=p(out), ln=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_semiglobal_full_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, gap, sc, en, mv, ln, None)

    def aff_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), ln=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_semiglobal_full_affine_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, ln, None)

    for f in (lin, aff, lin_dev, aff_dev):
        for bad in (bad_dec, bad_long, None):
            assert f(bad, good) == INV and f(good, bad) == INV
        assert f(good, good, mv=None) == INV and "lengths" in lib.swmi_last_error().decode()
        assert f(good, good, ln=None) == INV
        for name in ("s1p", "s2p", "sc", "en", "smp"):
            assert f(good, good, **{name: None}) == INV, name
        # n = 0 returns before the buffers and the offsets are looked at, but after the matrix, the gaps and moves / lengths
        assert f(bad_dec, None, n=0) == 0
        assert f(bad_dec, None, n=0, mv=None, ln=None, s1p=None, s2p=None, sc=None, en=None) == 0
        assert f(good, good, n=0, mv=None) == INV and f(good, good, n=0, smp=None) == INV
        # the buffers come before the offsets: the message names the buffer
        assert f(bad_dec, good, sc=None) == INV and "NULL buffer" in lib.swmi_last_error().decode()
    assert lin(good, good, gap=-1) == DOM and lin_dev(good, good, gap=-1) == DOM
    assert lin(good, good, gap=-1, n=0) == DOM
    for go, ge in ((-1, 0), (0, 128), (128, 1), (3, -2)):
        assert aff(good, good, go, ge) == DOM and aff_dev(good, good, go, ge) == DOM and aff(good, good, go, ge, n=0) == DOM
    assert lin(good, good, gap=0, n=0) == 0 and aff(good, good, 0, 0, n=0) == 0
    sr = swmi_mod.semiglobal_ragged
    sc, ends, moves, mo, lengths = sr.semiglobal_full_ragged([], [], sm, 1)
    assert len(sc) == 0 and ends.shape == (0, 2) and len(moves) == 0 and list(mo) == [0] and len(lengths) == 0
    sc, ends, moves, mo, lengths = sr.semiglobal_full_affine_ragged([], [], sm, 2, 1, traceback=False)
    assert len(sc) == 0 and ends.shape == (0, 2) and moves is None and mo is None and lengths is None
    with pytest.raises(swmi_mod.SwmiError) as e:
        sr.semiglobal_full_ragged((s1, bad_dec), (s2, good), sm, 1)
    assert e.value.code == INV
    with pytest.raises(ValueError):
        sr.semiglobal_full_ragged([s1[:3]], [s2[:3], s2[:2]], sm, 1)


# ---- what the Python wrappers hand to the C ABI ---------------------------------------------------------------------------------
LENS1, LENS2 = [5, 0, 9, 2], [7, 3, 0, 2]


@pytest.fixture
def rec(swmi_mod, monkeypatch):
    r = Recorder()
    monkeypatch.setattr(swmi_mod, "_lib", r)
    assert swmi_mod.load() is r
    return r


def _pairs():
    rng = np.random.default_rng(1)
    off1, off2 = _off(LENS1), _off(LENS2)
    return (rng.integers(0, 4, int(off1[-1]), dtype=np.uint8), off1), (rng.integers(0, 4, int(off2[-1]), dtype=np.uint8), off2)


@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("affine", [False, True])
def test_host_wrappers(swmi_mod, rec, affine, traceback):
    """The symbol and every argument by value and position; ends is (n, 2); traceback=False passes NULL for moves and lengths."""
    sr = swmi_mod.semiglobal_ragged
    (cat1, off1), (cat2, off2) = _pairs()
    fn, symbol, gaps = (sr.semiglobal_full_affine_ragged, "swmi_semiglobal_full_affine_ragged", (4, 2)) if affine else \
        (sr.semiglobal_full_ragged, "swmi_semiglobal_full_ragged", (3,))
    n = len(LENS1)
    scores, ends, moves, mo, lengths = fn((cat1, off1), (cat2, off2), SM, *gaps, traceback=traceback)
    calls = list(rec.calls)
    if traceback:                                       # the layout of the moves comes from the local family's function
        name, args = calls.pop(0)
        assert name == "swmi_local_full_ragged_move_offsets" and args[:3] == (off1.ctypes.data, off2.ctypes.data, n)
    assert calls == [(symbol, (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, SM.ctypes.data) + gaps
                      + (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(lengths)))]
    assert (scores.shape, scores.dtype) == ((n,), np.int32) and (ends.shape, ends.dtype) == ((n, 2), np.int32)
    if traceback:
        assert moves.dtype == np.uint64 and moves.ndim == 1 and (mo.shape, mo.dtype) == ((n + 1,), np.uint64)
        assert (lengths.shape, lengths.dtype) == ((n,), np.uint32)
    else:
        assert moves is None and mo is None and lengths is None and calls[0][1][-2:] == (None, None)


def test_device_wrappers(swmi_mod, rec):
    sr = swmi_mod.semiglobal_ragged
    off1, off2 = _off(LENS1), _off(LENS2)
    n = len(LENS1)
    for fn, symbol, gaps in ((sr.semiglobal_full_ragged_device, "swmi_semiglobal_full_ragged_device", (3,)),
                             (sr.semiglobal_full_affine_ragged_device, "swmi_semiglobal_full_affine_ragged_device", (4, 2))):
        for d_moves, d_lengths in ((DMV, DCT), (None, None)):
            tail = () if d_moves is None else (d_moves, d_lengths)
            del rec.calls[:]
            assert fn(D1, off1, D2, off2, SM, *gaps, DSC, DEN, *tail, stream=STREAM) is None
            assert rec.calls == [(symbol, (D1, off1.ctypes.data, D2, off2.ctypes.data, n, SM.ctypes.data) + gaps
                                  + (DSC, DEN, d_moves, d_lengths, STREAM))]
        del rec.calls[:]
        fn(D1, off1, D2, off2, SM, *gaps, DSC, DEN)
        assert rec.calls[0][1][-3:] == (None, None, 0)                    # ends-only, stream 0
        with pytest.raises(ValueError):
            fn(D1, off1, D2, off2[:-1], SM, *gaps, DSC, DEN)


def test_slices_for_wrapper(swmi_mod, rec):
    off1, off2 = _off(LENS1), _off(LENS2)
    for kwargs, flags in (({}, (0, 1)), ({"traceback": False}, (0, 0)), ({"affine": True}, (1, 1)), ({"affine": True, "traceback": False}, (1, 0))):
        del rec.calls[:]
        assert swmi_mod.semiglobal_ragged.semiglobal_full_ragged_slices_for(off1, off2, **kwargs) == []
        _check_slices(rec, "swmi_semiglobal_full_ragged_slices_for", (off1.ctypes.data, off2.ctypes.data, len(LENS1)) + flags)


def test_the_package_namespace_is_unchanged(swmi_mod):
    """The submodule is imported as a module: none of its functions is a top-level function of swmi, whose list is still the
    pinned one; each of the five has a docstring of its own."""
    want = _api_snapshot()
    assert len(want) == 94
    assert ["%s%s" % (n, inspect.signature(f)) for n, f in _public_functions(swmi_mod)] == want
    sr = swmi_mod.semiglobal_ragged
    assert inspect.ismodule(sr)
    names = [n for n, f in vars(sr).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == sr.__name__]
    assert sorted(names) == ["semiglobal_full_affine_ragged", "semiglobal_full_affine_ragged_device", "semiglobal_full_ragged",
                             "semiglobal_full_ragged_device", "semiglobal_full_ragged_slices_for"]
    docs = set()
    for name in names:
        assert not hasattr(swmi_mod, name), name
        doc = (getattr(sr, name).__doc__ or "").strip()
        assert doc and doc not in docs, name
        docs.add(doc)
