"""The ragged global / fit / overlap aligners' host-only parts, no device needed: the header and the library's symbols, every
argument error of the four entries, n = 0, swmi_global_full_ragged_slices_for (count cap, byte budgets, a single 16384 x 16384
affine traceback alignment that splits a batch), what swmi/global_ragged.py hands to the C ABI (the stand-in of
test_python_bindings.py records symbol and arguments), and the package's pinned top-level API."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_full_affine_support import code_qwords
from local_full_support import move_words
from test_python_bindings import DCT, DEN, DMV, DSC, D1, D2, SM, STREAM, Recorder, _api_snapshot, _check_slices, _ptr, _public_functions

MAX = 16384
ENDS_ONLY_BUDGET = 256 << 20
SLOT = 48                                   # sizeof(TileWork)
ENTRIES = ["swmi_global_full_ragged", "swmi_global_full_affine_ragged", "swmi_global_full_ragged_device",
           "swmi_global_full_affine_ragged_device", "swmi_global_full_ragged_slices_for"]


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


def _bytes(len1, len2, affine, tb):
    """device bytes one alignment of a ragged slice takes (include/swmi.h: inputs, slot, results, codes, moves, steps); an
    alignment with a zero length takes no codes, but its move words"""
    b = len1 + len2 + SLOT + 20
    if tb:
        words = code_qwords(len1, len2) if len1 and len2 else 0       # one code word per lane and step: a dword, affine a qword
        b += (8 if affine else 4) * words + 8 * move_words(len1, len2) + 4
    return b


def _fixed_budget(affine):
    """what 256 alignments of 16384 x 16384 take in the fixed-length global aligner's traceback slice"""
    return 256 * (2 * MAX + 4 + 16 + (8 if affine else 4) * code_qwords(MAX, MAX) + 8 * move_words(MAX, MAX) + 4)


def test_header_declares_and_library_exports_the_entries(swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+\w+\s+%s\(" % name, header), name
        assert getattr(lib, name) is not None
    assert "#define SWMI_VERSION 300" in header
    assert "swmi_global_full_ragged_move_offsets" not in header         # one layout, one function: the local family's
    assert not hasattr(lib, "swmi_global_full_ragged_move_offsets")
    # the zero-length table is stated where the entries are declared
    assert all(word in header for word in ("ZERO LENGTHS", "-cost(L)", "0xAAAA", "0x5555"))


def test_a_slice_holds_at_most_2_20_alignments(swmi_mod):
    n = (1 << 20) + 5
    rng = np.random.default_rng(2)
    off1, off2 = _off(rng.integers(0, 5, n)), _off(rng.integers(0, 5, n))
    for affine in (False, True):
        assert swmi_mod.global_ragged.global_full_ragged_slices_for(off1, off2, affine=affine, traceback=False) == [1 << 20, 5]


@pytest.mark.parametrize("affine", [False, True])
def test_ends_only_slices_are_the_longest_runs_within_256_mib(swmi_mod, affine):
    rng = np.random.default_rng(3)
    l1 = [int(x) for x in rng.integers(0, MAX + 1, 40000)]
    l2 = [int(x) for x in rng.integers(0, MAX + 1, 40000)]
    sizes = swmi_mod.global_ragged.global_full_ragged_slices_for(_off(l1), _off(l2), affine=affine, traceback=False)
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
    holds 255.  A single 16384 x 16384 alignment larger than the remainder of a slice splits the batch and still forms a slice
    with what follows it.  Alignments with a zero length take no codes: 2^20 of them fit one traceback slice by bytes."""
    slices_for = swmi_mod.global_ragged.global_full_ragged_slices_for
    budget = _fixed_budget(affine)
    assert slices_for(_off([MAX] * 300), _off([MAX] * 300), affine=affine) == [255, 45]
    big = _bytes(MAX, MAX, affine, True)
    small = _bytes(2000, 1000, affine, True)
    n_small = (budget - big // 2) // small                   # leaves less than one big alignment's room
    l1, l2 = [2000] * n_small + [MAX, 5], [1000] * n_small + [MAX, 5]
    assert slices_for(_off(l1), _off(l2), affine=affine) == [n_small, 2]
    assert n_small * small <= budget < n_small * small + big
    n_zero = 1 << 20
    assert n_zero * _bytes(1000, 0, affine, True) <= budget < n_zero * _bytes(1000, 1000, affine, True)
    assert slices_for(_off([1000] * n_zero), _off([0] * n_zero), affine=affine) == [n_zero]


def test_argument_errors_and_an_empty_batch_need_no_device(swmi_mod):
    """Every argument error of the four entries and the helper, and n = 0, in a process with no GPU bound."""
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

    def lin(o1, o2, gap=1, mask=0, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_global_full_ragged(s1p, p(o1), s2p, p(o2), n, smp, gap, mask, sc, en, mv, st)

    def aff(o1, o2, go=1, ge=1, mask=0, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_global_full_affine_ragged(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st)

    def lin_dev(o1, o2, gap=1, mask=0, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_global_full_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, gap, mask, sc, en, mv, st, None)

    def aff_dev(o1, o2, go=1, ge=1, mask=0, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out)):
        return lib.swmi_global_full_affine_ragged_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st, None)

    for f in (lin, aff, lin_dev, aff_dev):
        for bad in (bad_dec, bad_long, None):
            assert f(bad, good) == INV and f(good, bad) == INV
        assert f(good, good, mv=None) == INV
        assert f(good, good, st=None) == INV
        for name in ("s1p", "s2p", "sc", "en", "smp"):
            assert f(good, good, **{name: None}) == INV, name
        for mask in (16, 255, 0xFFFFFFFF):
            assert f(good, good, mask=mask) == INV and f(good, good, mask=mask, n=0) == INV
        for mask in range(16):
            assert f(bad_dec, None, n=0, mask=mask) == 0            # n = 0: a no-op under every mask
        assert f(bad_dec, None, n=0, mv=None, st=None) == 0
    assert lin(good, good, gap=-1) == DOM and lin_dev(good, good, gap=-1) == DOM
    for go, ge in ((-1, 0), (0, 128), (128, 1), (3, -2)):
        assert aff(good, good, go, ge) == DOM and aff_dev(good, good, go, ge) == DOM
    for bad in (bad_dec, bad_long, None):
        assert lib.swmi_global_full_ragged_slices_for(p(bad), p(good), 4, 0, 1, None, 0) == 0
        assert lib.swmi_global_full_ragged_slices_for(p(good), p(bad), 4, 1, 1, None, 0) == 0
    assert lib.swmi_global_full_ragged_slices_for(p(good), p(good), 4, 0, 1, None, 0) == 1
    one = np.zeros(1, np.uint64)
    gr = swmi_mod.global_ragged
    assert gr.global_full_ragged_slices_for(one, one) == []
    sc, ends, moves, mo, steps = gr.global_full_ragged([], [], sm, 1, swmi_mod.ENDS_FIT)
    assert len(sc) == 0 and ends.shape == (0, 4) and len(moves) == 0 and list(mo) == [0] and len(steps) == 0
    sc, ends, moves, mo, steps = gr.global_full_affine_ragged([], [], sm, 2, 1, traceback=False)
    assert len(sc) == 0 and moves is None and mo is None and steps is None
    with pytest.raises(swmi_mod.SwmiError) as e:
        gr.global_full_ragged((s1, bad_dec), (s2, good), sm, 1)
    assert e.value.code == INV
    with pytest.raises(swmi_mod.SwmiError) as e:
        gr.global_full_affine_ragged((s1, good), (s2, good), sm, 1, 1, 16, traceback=False)
    assert e.value.code == INV
    with pytest.raises(ValueError):
        gr.global_full_ragged([s1[:3]], [s2[:3], s2[:2]], sm, 1)


# ---- what the Python wrappers hand to the C ABI ---------------------------------------------------------------------------------
LENS1, LENS2 = [5, 0, 9, 2], [7, 3, 0, 2]
MASKS = ((None, 0), (10, 10), (15, 15), (-3, (-3) & 0xFFFFFFFF))     # (given, what the C entry must get); None: the default


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
    """The symbol and every argument by value and position: the (concatenated, offsets) form is passed where it lies; the mask
    defaults to ENDS_GLOBAL and goes after the gap or gaps; traceback=False passes NULL for moves and steps."""
    gr = swmi_mod.global_ragged
    (cat1, off1), (cat2, off2) = _pairs()
    fn, symbol, gaps = (gr.global_full_affine_ragged, "swmi_global_full_affine_ragged", (4, 2)) if affine else \
        (gr.global_full_ragged, "swmi_global_full_ragged", (3,))
    n = len(LENS1)
    for given, passed in MASKS:
        del rec.calls[:]
        extra = () if given is None else (given,)
        scores, ends, moves, mo, steps = fn((cat1, off1), (cat2, off2), SM, *gaps, *extra, traceback=traceback)
        calls = list(rec.calls)
        if traceback:                                   # the layout of the moves comes from the local family's function
            name, args = calls.pop(0)
            assert name == "swmi_local_full_ragged_move_offsets" and args[:3] == (off1.ctypes.data, off2.ctypes.data, n)
        assert calls == [(symbol, (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, SM.ctypes.data) + gaps
                          + (passed, scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))]
        assert (scores.shape, scores.dtype) == ((n,), np.int32) and (ends.shape, ends.dtype) == ((n, 4), np.int32)
        if traceback:
            assert moves.dtype == np.uint64 and (mo.shape, mo.dtype) == ((n + 1,), np.uint64)
            assert (steps.shape, steps.dtype) == ((n,), np.uint32)
        else:
            assert moves is None and mo is None and steps is None and calls[0][1][-2:] == (None, None)
    del rec.calls[:]
    if affine:
        fn((cat1, off1), (cat2, off2), SM, gap_extend=2, gap_open=4, free_ends=swmi_mod.ENDS_FIT, traceback=False)   # by keyword
        assert rec.calls[0][1][6:9] == (4, 2, 10)
    else:
        fn((cat1, off1), (cat2, off2), SM, gap_penalty=3, free_ends=swmi_mod.ENDS_FIT, traceback=False)
        assert rec.calls[0][1][6:8] == (3, 10)


def test_host_wrapper_list_form(swmi_mod, monkeypatch):
    """A list of arrays reaches the entry concatenated, with the prefix sums of the lengths as offsets."""
    seen = []

    def on_call(name, args):
        if name == "swmi_global_full_ragged":
            n = args[4]
            off1 = np.frombuffer(ctypes.string_at(args[1], 8 * (n + 1)), np.uint64)
            off2 = np.frombuffer(ctypes.string_at(args[3], 8 * (n + 1)), np.uint64)
            seen.append((off1, off2, ctypes.string_at(args[0], int(off1[-1])), ctypes.string_at(args[2], int(off2[-1])), args[6:8]))

    monkeypatch.setattr(swmi_mod, "_lib", Recorder(on_call))
    (cat1, off1), (cat2, off2) = _pairs()
    a = [cat1[int(off1[k]):int(off1[k + 1])] for k in range(len(LENS1))]
    b = [cat2[int(off2[k]):int(off2[k + 1])] for k in range(len(LENS2))]
    swmi_mod.global_ragged.global_full_ragged(a, b, SM, 3, swmi_mod.ENDS_OVERLAP, traceback=False)
    (g1, g2, bytes1, bytes2, tail), = seen
    assert np.array_equal(g1, off1) and np.array_equal(g2, off2) and bytes1 == cat1.tobytes() and bytes2 == cat2.tobytes()
    assert tail == (3, 15)


def test_device_wrappers(swmi_mod, rec):
    gr = swmi_mod.global_ragged
    off1, off2 = _off(LENS1), _off(LENS2)
    n = len(LENS1)
    for fn, symbol, gaps in ((gr.global_full_ragged_device, "swmi_global_full_ragged_device", (3,)),
                             (gr.global_full_affine_ragged_device, "swmi_global_full_affine_ragged_device", (4, 2))):
        for given, passed in MASKS:
            mask = swmi_mod.ENDS_GLOBAL if given is None else given       # (free_ends has no default in the device wrappers)
            for d_moves, d_steps in ((DMV, DCT), (None, None)):
                tail = () if d_moves is None else (d_moves, d_steps)
                del rec.calls[:]
                assert fn(D1, off1, D2, off2, SM, *gaps, mask, DSC, DEN, *tail, stream=STREAM) is None
                assert rec.calls == [(symbol, (D1, off1.ctypes.data, D2, off2.ctypes.data, n, SM.ctypes.data) + gaps
                                      + (passed, DSC, DEN, d_moves, d_steps, STREAM))]
        del rec.calls[:]
        fn(D1, off1, D2, off2, SM, *gaps, 10, DSC, DEN)
        assert rec.calls[0][1][-3:] == (None, None, 0)                    # ends-only, stream 0
        with pytest.raises(ValueError):
            fn(D1, off1, D2, off2[:-1], SM, *gaps, 0, DSC, DEN)


def test_slices_for_wrapper(swmi_mod, rec):
    off1, off2 = _off(LENS1), _off(LENS2)
    for kwargs, flags in (({}, (0, 1)), ({"traceback": False}, (0, 0)), ({"affine": True}, (1, 1)), ({"affine": True, "traceback": False}, (1, 0))):
        del rec.calls[:]
        assert swmi_mod.global_ragged.global_full_ragged_slices_for(off1, off2, **kwargs) == []
        _check_slices(rec, "swmi_global_full_ragged_slices_for", (off1.ctypes.data, off2.ctypes.data, len(LENS1)) + flags)


def test_gaps_that_ctypes_would_wrap_are_refused(swmi_mod, rec):
    gr = swmi_mod.global_ragged
    pairs = _pairs()
    off1, off2 = _off(LENS1), _off(LENS2)
    with pytest.raises(swmi_mod.SwmiError) as e:
        gr.global_full_ragged(*pairs, SM, 256)
    assert e.value.code == swmi_mod.ERR_DOMAIN
    for go, ge in ((2**32 + 1, 1), (1, 2**32 + 1), (-2**32, 1)):
        with pytest.raises(swmi_mod.SwmiError) as e:
            gr.global_full_affine_ragged(*pairs, SM, go, ge)
        assert e.value.code == swmi_mod.ERR_DOMAIN
        with pytest.raises(swmi_mod.SwmiError) as e:
            gr.global_full_affine_ragged_device(D1, off1, D2, off2, SM, go, ge, 0, DSC, DEN)
        assert e.value.code == swmi_mod.ERR_DOMAIN
    with pytest.raises(swmi_mod.SwmiError):
        gr.global_full_ragged(*pairs, np.full(16, 300, np.int64), 1)
    assert rec.calls == []


def test_the_package_namespace_is_unchanged(swmi_mod):
    """The submodule is imported as a module: none of its functions is a top-level function of swmi, whose list is still the
    pinned one."""
    want = _api_snapshot()
    assert len(want) == 94
    assert ["%s%s" % (n, inspect.signature(f)) for n, f in _public_functions(swmi_mod)] == want
    gr = swmi_mod.global_ragged
    assert inspect.ismodule(gr)
    names = [n for n, f in vars(gr).items() if inspect.isfunction(f) and not n.startswith("_") and f.__module__ == gr.__name__]
    assert sorted(names) == ["global_full_affine_ragged", "global_full_affine_ragged_device", "global_full_ragged",
                             "global_full_ragged_device", "global_full_ragged_slices_for"]
    for name in names:
        assert not hasattr(swmi_mod, name), name
        assert (getattr(gr, name).__doc__ or "").strip(), name
