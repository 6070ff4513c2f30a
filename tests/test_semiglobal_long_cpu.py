"""The long semi-global aligners (swmi_semiglobal_long*, swmi_semiglobal_long_affine*) without a GPU: the new symbols declared and
exported beside every symbol the library exported before them (tests/golden/exports_before_semiglobal_long.txt), what the entries
refuse before any device is touched -- through the host entry, the device entry and the timer, with code and text -- the domain
rule's edge at 65536 x 65536, the slices' arithmetic with the carry counted, both expanders' limits, the Python submodule, and the
fixed-length entries' unchanged limit."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix

STRIPE, MAX_LEN = 16384, 65536
NAMES = [base + suffix for base in ("swmi_semiglobal_long", "swmi_semiglobal_long_affine")
         for suffix in ("", "_device", "_time_device", "_slices_for", "_release_workspaces")] + ["swmi_semiglobal_long_expand_moves"]
NOT_INIT = "swmi_init() has not been called (or failed)"


@pytest.fixture(scope="module")
def sl(swmi_mod):
    return swmi_mod.semiglobal_long


def test_symbols_declared_and_exported(swmi_mod, sl):
    header = open(os.path.join(ROOT, "include", "swmi.h")).read()
    assert len(set(NAMES)) == 11                  # five entries per family and the expander; with them the three macros below
    for name in NAMES:
        assert "SWMI_API" in header and (" " + name + "(") in header, name
    assert "#define SWMI_SEMIGLOBAL_LONG_MAX_LEN 65536" in header and "#define SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(len1, len2)" in header
    assert "#define SWMI_SEMIGLOBAL_LONG_MAX_TRACEBACK 131073" in header
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libswmi.so")], stdout=subprocess.PIPE, text=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    before = open(os.path.join(ROOT, "tests", "golden", "exports_before_semiglobal_long.txt")).read().split()
    assert len(before) > 130 and not set(before) & set(NAMES)
    assert set(before) <= exported, sorted(set(before) - exported)
    # the move-word formula is the fixed-length entry's
    for len1, len2 in ((1, 1), (129, 17409), (MAX_LEN, MAX_LEN)):
        assert sl.move_words(len1, len2) == (((len1 + len2 + 31) // 32) + 1) & ~1
    for len1, len2 in ((1, 1), (300, 16384), (STRIPE, STRIPE)):
        assert sl.move_words(len1, len2) == swmi_mod.semiglobal_full_move_words(len1, len2)


# ---- refusals through the three kinds of entry ------------------------------------------------------------------------------

def _aligned(nbytes):
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]


def _entries(swmi_mod, affine, len1, len2, sm, gaps, n=1, moves=None, lengths=None):
    """The status and swmi_last_error() text of the host entry, the device entry and the timer on one call (ends-only unless
    `moves` / `lengths` are given)."""
    lib = swmi_mod.load()
    lib.swmi_last_error.restype = ctypes.c_char_p
    base = "swmi_semiglobal_long_affine" if affine else "swmi_semiglobal_long"
    a, b = _aligned(max(1, min(len1, MAX_LEN))), _aligned(max(1, min(len2, MAX_LEN)))
    sc, ends = _aligned(16), _aligned(16)
    ms = ctypes.c_float()
    smp = sm.ctypes.data if sm is not None else None
    head = (a.ctypes.data, len1, b.ctypes.data, len2, n, smp) + tuple(gaps)
    out = []
    for name, tail in ((base, (sc.ctypes.data, ends.ctypes.data, moves, lengths)),
                       (base + "_device", (sc.ctypes.data, ends.ctypes.data, moves, lengths, None)),
                       (base + "_time_device", (sc.ctypes.data, ends.ctypes.data, moves, lengths, None, 2, ctypes.byref(ms)))):
        rc = getattr(lib, name)(*head, *tail)
        out.append((rc, lib.swmi_last_error().decode()))
    return out


@pytest.mark.parametrize("affine", [False, True])
def test_refusals_need_no_device(swmi_mod, affine):
    k = match_matrix(1, -1)
    gaps = (3, 1) if affine else (1,)
    inv, dom = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN
    for len1, len2 in ((0, 5), (5, 0), (MAX_LEN + 1, 5), (5, MAX_LEN + 1)):
        for rc, text in _entries(swmi_mod, affine, len1, len2, k, gaps):
            assert rc == inv and text == "lengths (%d, %d) outside [1, 65536]" % (len1, len2)
    for rc, text in _entries(swmi_mod, affine, 5, 5, None, gaps):
        assert rc == inv and text == "score_matrix is NULL"
    if affine:
        for rc, text in _entries(swmi_mod, affine, 5, 5, k, (128, 1)):
            assert rc == dom and text == "gap_open 128 / gap_extend 1 outside [0,127]"
        for rc, text in _entries(swmi_mod, affine, 5, 5, k, (1, 128)):
            assert rc == dom and text == "gap_open 1 / gap_extend 128 outside [0,127]"
        for rc, text in _entries(swmi_mod, affine, 5, 5, k, (-1, 1)):
            assert rc == dom and text == "gap_open -1 / gap_extend 1 outside [0,127]"
    else:
        # the fixed entry's gap check, code and text
        lib = swmi_mod.load()
        a, sc, ends = np.zeros(8, np.uint8), np.zeros(1, np.int32), np.zeros(2, np.int32)
        rc = lib.swmi_semiglobal_full(a.ctypes.data, 5, a.ctypes.data, 5, 1, k.ctypes.data, -1, sc.ctypes.data, ends.ctypes.data, None, None)
        fixed_text = lib.swmi_last_error().decode()
        assert rc == dom
        for got, text in _entries(swmi_mod, affine, 5, 5, k, (-1,)):
            assert got == dom and text == fixed_text


@pytest.mark.parametrize("affine", [False, True])
def test_only_one_of_moves_and_lengths_is_refused(swmi_mod, affine):
    """moves without lengths, and lengths without moves: refused, with the fixed entry's code and text, by all three kinds of
    entry and before any device is looked for."""
    k = match_matrix(1, -1)
    gaps = (3, 1) if affine else (1,)
    lib = swmi_mod.load()
    lib.swmi_last_error.restype = ctypes.c_char_p
    buf = _aligned(64)
    a, sc, ends = np.zeros(8, np.uint8), np.zeros(1, np.int32), np.zeros(2, np.int32)
    fixed = lib.swmi_semiglobal_full_affine if affine else lib.swmi_semiglobal_full
    for moves, lengths in ((buf.ctypes.data, None), (None, buf.ctypes.data)):
        rc = fixed(a.ctypes.data, 5, a.ctypes.data, 5, 1, k.ctypes.data, *gaps, sc.ctypes.data, ends.ctypes.data, moves, lengths)
        want = lib.swmi_last_error().decode()
        assert rc == swmi_mod.ERR_INVALID_ARGUMENT and want != NOT_INIT
        host, device, timer = _entries(swmi_mod, affine, 5, 5, k, gaps, moves=moves, lengths=lengths)
        assert host == (rc, want), host
        for got in (device, timer):
            assert got[0] == swmi_mod.ERR_INVALID_ARGUMENT and got[1] != NOT_INIT, got


@pytest.mark.parametrize("affine", [False, True])
def test_domain_rule(swmi_mod, sl, affine):
    """Accepted iff max(1, max |sm|, gaps) * (len1 + len2) <= 2^23.  A call inside the rule goes on to look for a device, which
    this process has not bound."""
    inv = swmi_mod.ERR_INVALID_ARGUMENT
    text = ("max(1, |score|, gap_open, gap_extend) * (len1 + len2) = P * 131072 above 2^23" if affine
            else "max(1, |score|, gap) * (len1 + len2) = P * 131072 above 2^23")
    for rc, got in _entries(swmi_mod, affine, MAX_LEN, MAX_LEN, match_matrix(127, -127), (127, 127) if affine else (127,)):
        assert rc == inv and got == text
    # (64, -64, 65) is refused, gap 64 is the edge: 64 * 131072 = 2^23
    for gaps in (((65, 64), (64, 65)) if affine else ((65,),)):
        for rc, got in _entries(swmi_mod, affine, MAX_LEN, MAX_LEN, match_matrix(64, -64), gaps):
            assert rc == inv and got == text
    for rc, got in _entries(swmi_mod, affine, MAX_LEN, MAX_LEN, match_matrix(65, -64), (64, 64) if affine else (64,)):
        assert rc == inv and got == text
    assert 64 * 2 * MAX_LEN == 1 << 23
    for rc, got in _entries(swmi_mod, affine, MAX_LEN, MAX_LEN, match_matrix(64, -64), (64, 64) if affine else (64,)):
        assert rc == swmi_mod.ERR_NOT_INITIALIZED and got == NOT_INIT, (rc, got)
    # every shape up to 32768 x 32768 passes with any int8 parameters; one base more does not
    for rc, got in _entries(swmi_mod, affine, 32768, 32768, match_matrix(127, -128), (127, 127) if affine else (127,)):
        assert rc == swmi_mod.ERR_NOT_INITIALIZED and got == NOT_INIT, (rc, got)
    for rc, got in _entries(swmi_mod, affine, 32768, 32769, match_matrix(127, -128), (127, 127) if affine else (127,)):
        assert rc == inv and got.endswith("P * 65537 above 2^23")
    # the stripe-edge grid's extreme set is inside the rule, and the key range the rule buys (the kernels' headers, (a) - (c))
    assert 127 * (257 + MAX_LEN) < 1 << 23
    assert ((1 << 23) + 1023 * 127) < (1 << 23) + (1 << 17) and (MAX_LEN + 95) * 127 < 1 << 23
    assert (((1 << 23) + (1 << 17)) << 6) + (128 << 6) + 63 < 1 << 30 and -(1 << 30) - (127 << 6) > -(1 << 31)
    # _slices_for knows no parameters and takes the shape
    slices_for = sl.semiglobal_long_affine_slices_for if affine else sl.semiglobal_long_slices_for
    assert slices_for(40, MAX_LEN, MAX_LEN) == [16, 16, 8]


# ---- slices ------------------------------------------------------------------------------------------------------------------

def _trips(len1):
    return ((len1 + 63 + 31) // 32) * 8


def _alignment_bytes(len1, len2, affine, tb):
    """Device bytes of one alignment of a slice: inputs, score, the best cell, the carry where len2 > 16384, and with a traceback
    the codes (one dword -- affine: one qword -- per lane and step of the padded sweep), the moves and the length."""
    code_bytes = ((len2 + 1023) // 1024) * _trips(len1) * 256 * (8 if affine else 4)
    move_words = (((len1 + len2 + 31) // 32) + 1) & ~1
    carry = (len1 * (8 if affine else 4)) if len2 > STRIPE else 0
    return len1 + len2 + 4 + 8 + carry + (code_bytes + 8 * move_words + 4 if tb else 0)


@pytest.mark.parametrize("affine", [False, True])
def test_slices_for(swmi_mod, sl, affine):
    slices_for = sl.semiglobal_long_affine_slices_for if affine else sl.semiglobal_long_slices_for
    fixed = swmi_mod.semiglobal_full_affine_slices_for if affine else swmi_mod.semiglobal_full_slices_for
    budget = 256 * _alignment_bytes(STRIPE, STRIPE, affine, True)          # the fixed-length semi-global entry's traceback budget
    assert slices_for(40, MAX_LEN, MAX_LEN) == [16, 16, 8]                  # the known limit
    assert budget // _alignment_bytes(MAX_LEN, MAX_LEN, affine, True) == 16
    # (257, 65536): 64 waves x 80 trips of codes, 2057 -> 2058 move words, a carry of 257 dwords (affine: 514)
    unit = 8 if affine else 4
    wide = 257 + 65536 + 4 + 8 + 257 * unit + 64 * 80 * 256 * unit + 8 * 2058 + 4
    assert wide == _alignment_bytes(257, MAX_LEN, affine, True)
    # (65536, 257): 1 wave x 16400 trips, no carry
    tall = 65536 + 257 + 4 + 8 + 1 * 16400 * 256 * unit + 8 * 2058 + 4
    assert tall == _alignment_bytes(MAX_LEN, 257, affine, True)
    for shape, per in (((257, MAX_LEN), wide), ((MAX_LEN, 257), tall)):
        s = min(budget // per, 1 << 20)
        assert slices_for(2 * s + 1, *shape) == [s, s, 1] and slices_for(s, *shape) == [s], shape
        e = min((256 << 20) // _alignment_bytes(*shape, affine, False), 1 << 20)
        assert slices_for(e + 2, *shape, traceback=False) == [e, 2], shape
    # the carry decides an ends-only slice's size at (65536, 65536), and is absent at (65536, 16384)
    assert slices_for(1 << 20, MAX_LEN, MAX_LEN, traceback=False)[0] == (256 << 20) // (2 * MAX_LEN + 12 + MAX_LEN * unit)
    assert slices_for(1 << 20, MAX_LEN, STRIPE, traceback=False)[0] == (256 << 20) // (MAX_LEN + STRIPE + 12)
    assert slices_for(5, 0, 5) == [] and slices_for(5, 5, MAX_LEN + 1) == [] and slices_for(5, MAX_LEN + 1, 5) == [] and slices_for(5, 5, 0) == []
    # where both lengths fit the fixed-length entry the slices are that entry's
    for n in (1, 255, 256, 257, 4097):
        for len1 in (1, 63, 64, 65, 1024, 16383, 16384):
            for len2 in (1, 63, 64, 65, 1024, 16383, 16384):
                for tb in (True, False):
                    assert slices_for(n, len1, len2, traceback=tb) == fixed(n, len1, len2, traceback=tb), (n, len1, len2, tb)


# ---- the expanders -----------------------------------------------------------------------------------------------------------

def test_expand_moves_limits(swmi_mod, sl):
    """swmi_semiglobal_long_expand_moves takes a length of 131073 (65536 up moves behind 65536 left moves); 131074 and 0 are
    refused; swmi_semiglobal_expand_moves still refuses 32770 and still takes 32769."""
    assert sl.MAX_TRACEBACK == 2 * MAX_LEN + 1 == 131073
    moves = np.zeros(sl.move_words(MAX_LEN, MAX_LEN), np.uint64)
    moves[:2048] = 0x5555555555555555                                     # walking order: 65536 left moves, then
    moves[2048:4096] = 0xAAAAAAAAAAAAAAAA                                 # 65536 up moves
    pos = sl.expand_moves(moves, 131073)
    assert pos.shape == (131073, 2) and pos[0].tolist() == [0, 0] and pos[-1].tolist() == [MAX_LEN, MAX_LEN]
    assert pos[MAX_LEN].tolist() == [MAX_LEN, 0] and pos[MAX_LEN + 1].tolist() == [MAX_LEN, 1]
    assert sl.expand_moves(moves, 131073, cap=3).tolist() == [[0, 0], [1, 0], [2, 0]]
    assert sl.expand_moves(moves, 1).tolist() == [[0, 0]]
    assert np.array_equal(sl.expand_moves(moves, 32769), swmi_mod.semiglobal_expand_moves(moves, 32769))
    for bad in (131074, 0):
        with pytest.raises(swmi_mod.SwmiError) as e:
            sl.expand_moves(moves, bad)
        assert "outside [1, 131073]" in str(e.value)
    with pytest.raises(swmi_mod.SwmiError) as e:
        swmi_mod.semiglobal_expand_moves(moves, 32770)
    assert "length 32770 outside [1, 32769]" in str(e.value)


# ---- the Python submodule, and what stays as it was -----------------------------------------------------------------------------

def test_python_module(swmi_mod, sl):
    import swmi
    assert swmi.semiglobal_long is sl and sl.MAX_LEN == MAX_LEN and sl.move_words(MAX_LEN, MAX_LEN) == 4096 and sl.move_words(1, 1) == 2
    names = ["move_words", "expand_moves"] + [base + suffix for base in ("semiglobal_long", "semiglobal_long_affine")
                                              for suffix in ("", "_device", "_time_device", "_slices_for", "_release_workspaces")]
    for name in names:
        f = getattr(sl, name)
        assert inspect.isfunction(f) and f.__doc__ and len(f.__doc__) > 20, name
        assert not inspect.isfunction(getattr(swmi, name, None)), name      # (swmi.semiglobal_long is the module)
    assert sl.__doc__
    # the package's own top level still defines exactly the pinned functions
    pinned = open(os.path.join(ROOT, "tests", "python_api.txt")).read().splitlines()
    top = sorted(n for n, f in vars(swmi).items() if inspect.isfunction(f) and not n.startswith("_"))
    assert len(pinned) == 94 and top == sorted(line.split("(")[0] for line in pinned)
    # argtypes of every new entry are set by load()
    lib = swmi.load()
    for name in NAMES:
        assert name.endswith("_release_workspaces") or getattr(lib, name).argtypes is not None, name      # (void)
    # the module's own argument checks
    k = match_matrix(1, -1)
    a = np.zeros((2, 40), np.uint8)
    with pytest.raises(ValueError):
        sl.semiglobal_long(a, np.zeros((3, 40), np.uint8), k, 1)
    with pytest.raises(ValueError):
        sl.semiglobal_long_affine(a, a, np.zeros(15, np.int8), 3, 1)
    for bad in (lambda: sl.semiglobal_long(a, a, k, 128), lambda: sl.semiglobal_long_affine(a, a, k, 2**32 + 1, 1),
                lambda: sl.semiglobal_long_affine(a, a, k, 3, 128),
                lambda: sl.semiglobal_long(np.zeros((1, MAX_LEN + 1), np.uint8), a[:1], k, 1)):
        with pytest.raises(swmi_mod.SwmiError):
            bad()


def test_fixed_entries_still_refuse_16385(swmi_mod):
    k = match_matrix(1, -1)
    lib = swmi_mod.load()
    lib.swmi_last_error.restype = ctypes.c_char_p
    a, sc, ends = np.zeros(STRIPE + 1, np.uint8), np.zeros(1, np.int32), np.zeros(2, np.int32)
    for len1, len2 in ((STRIPE + 1, 5), (5, STRIPE + 1)):
        rc = lib.swmi_semiglobal_full(a.ctypes.data, len1, a.ctypes.data, len2, 1, k.ctypes.data, 1, sc.ctypes.data, ends.ctypes.data, None,
                                      None)
        assert rc == swmi_mod.ERR_INVALID_ARGUMENT and lib.swmi_last_error().decode() == "lengths (%d, %d) outside [1, 16384]" % (len1, len2)
        rc = lib.swmi_semiglobal_full_affine(a.ctypes.data, len1, a.ctypes.data, len2, 1, k.ctypes.data, 3, 1, sc.ctypes.data,
                                             ends.ctypes.data, None, None)
        assert rc == swmi_mod.ERR_INVALID_ARGUMENT and lib.swmi_last_error().decode() == "lengths (%d, %d) outside [1, 16384]" % (len1, len2)
    assert swmi_mod.semiglobal_full_slices_for(3, STRIPE + 1, 5) == [] and swmi_mod.semiglobal_full_affine_slices_for(3, 5, STRIPE + 1) == []


def test_cpp_header_compiles(tmp_path):
    """include/swmi_compat.hpp's SemiGlobal_long_mi355x, SemiGlobal_long_affine_mi355x and their batch forms compile and link
    against the library (the GPU tests run the program)."""
    import shutil
    assert shutil.which("g++") is not None, "g++ not available"
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_semiglobal_long.cpp"), "-o",
                            str(tmp_path / "compat_semiglobal_long"), "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
