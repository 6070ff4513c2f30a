"""The long global / fit / overlap aligners (swmi_global_long*, swmi_global_long_affine*) without a GPU: what they refuse before
any device is touched (lengths, mask, NULLs, the domain rule P (len1 + len2) <= 2^23 on both sides of its edge), the slices'
arithmetic with the carry counted, the expander's bounds, the key-range arithmetic that the kernels' files derive, and the
Python module's own argument checks."""
import ctypes

import numpy as np
import pytest

from conftest import match_matrix

INVALID, DOMAIN = -2, None        # DOMAIN is read from the module below
STRIPE, MAX_LEN = 16384, 65536
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def gl(swmi_mod):
    return swmi_mod.global_long


def _rc(swmi_mod, fn, *args):
    """The status of a raw C call (no exception)."""
    return getattr(swmi_mod.load(), fn)(*args)


def _linear(swmi_mod, len1, len2, sm, gap, mask=0, n=1, bufs=True, moves=False, steps=False):
    a = np.zeros(max(1, n * len1), np.uint8)
    b = np.zeros(max(1, n * len2), np.uint8)
    sc, ends = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 4), np.int32)
    mv, st = np.zeros(8200, np.uint64), np.zeros(max(n, 1), np.uint32)
    return _rc(swmi_mod, "swmi_global_long", a.ctypes.data if bufs else None, len1, b.ctypes.data if bufs else None, len2, n,
               sm.ctypes.data if sm is not None else None, gap, mask, sc.ctypes.data if bufs else None, ends.ctypes.data,
               mv.ctypes.data if moves else None, st.ctypes.data if steps else None)


def _affine(swmi_mod, len1, len2, sm, go, ge, mask=0):
    a, b = np.zeros(len1 or 1, np.uint8), np.zeros(len2 or 1, np.uint8)
    sc, ends = np.zeros(1, np.int32), np.zeros((1, 4), np.int32)
    return _rc(swmi_mod, "swmi_global_long_affine", a.ctypes.data, len1, b.ctypes.data, len2, 1, sm.ctypes.data, go, ge, mask,
               sc.ctypes.data, ends.ctypes.data, None, None)


def test_refusals_need_no_device(swmi_mod):
    """Every refusal comes back as a status before any device is looked for (this process has bound none)."""
    k = match_matrix(1, -1)
    inv, dom = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN
    for len1, len2 in ((0, 5), (5, 0), (MAX_LEN + 1, 5), (5, MAX_LEN + 1)):
        assert _linear(swmi_mod, len1, len2, k, 1) == inv
        assert _affine(swmi_mod, len1, len2, k, 3, 1) == inv
    assert _linear(swmi_mod, 5, 5, k, 1, mask=16) == inv and _affine(swmi_mod, 5, 5, k, 3, 1, mask=16) == inv
    assert _linear(swmi_mod, 5, 5, None, 1) == inv
    assert _linear(swmi_mod, 5, 5, k, 1, bufs=False) == inv                    # NULL sequences and scores
    assert _linear(swmi_mod, 5, 5, k, 1, moves=True) == inv and _linear(swmi_mod, 5, 5, k, 1, steps=True) == inv
    assert _linear(swmi_mod, 5, 5, k, -1) == dom
    assert _affine(swmi_mod, 5, 5, k, 128, 1) == dom and _affine(swmi_mod, 5, 5, k, 1, -1) == dom
    assert _linear(swmi_mod, 5, 5, k, 1, n=0, bufs=False) == 0                 # n = 0: a no-op


def test_domain_rule_at_its_edge(swmi_mod):
    """P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gaps): a refusal is INVALID_ARGUMENT; an accepted call goes on to look
    for a device, which this process has not bound, so it comes back with another status."""
    inv = swmi_mod.ERR_INVALID_ARGUMENT
    k128 = match_matrix(1, -128)
    k64, k65, k1 = match_matrix(64, -64), match_matrix(64, -65), match_matrix(1, -1)
    assert 128 * (32768 + 32768) == 1 << 23 and 64 * (65536 + 65536) == 1 << 23
    accepted = lambda rc: rc != inv and rc != swmi_mod.ERR_DOMAIN  # noqa: E731
    assert accepted(_linear(swmi_mod, 32768, 32768, k128, 127))
    assert _linear(swmi_mod, 32769, 32768, k128, 127) == inv
    assert _linear(swmi_mod, 32768, 32769, k128, 1) == inv
    assert accepted(_linear(swmi_mod, MAX_LEN, MAX_LEN, k64, 64))
    assert _linear(swmi_mod, MAX_LEN, MAX_LEN, k65, 1) == inv
    assert _linear(swmi_mod, MAX_LEN, MAX_LEN, k64, 65) == inv
    assert accepted(_linear(swmi_mod, MAX_LEN, MAX_LEN, k1, 0))                # P = max(1, ..): never 0
    assert accepted(_affine(swmi_mod, MAX_LEN, MAX_LEN, k64, 64, 64))
    assert _affine(swmi_mod, MAX_LEN, MAX_LEN, k64, 65, 1) == inv and _affine(swmi_mod, MAX_LEN, MAX_LEN, k64, 1, 65) == inv
    assert accepted(_affine(swmi_mod, 32768, 32768, k128, 127, 127)) and _affine(swmi_mod, 32768, 32769, k128, 0, 0) == inv
    # every shape up to 32768 x 32768 takes any int8 parameters: 128 is the largest magnitude there is
    assert 128 * (32768 + 32768) <= 1 << 23


def _trips(len1):
    return ((len1 + 63 + 31) // 32) * 8


def _alignment_bytes(len1, len2, affine, tb):
    """Device bytes of one alignment of a slice: inputs, score, ends, the carry where len2 > 16384, and with a traceback the
    codes (one dword -- affine: one qword -- per lane and step of the padded sweep), the moves and the count."""
    code_bytes = ((len2 + 1023) // 1024) * _trips(len1) * 256 * (8 if affine else 4)
    move_words = (((len1 + len2 + 31) // 32) + 1) & ~1
    carry = (len1 * (8 if affine else 4)) if len2 > STRIPE else 0
    return len1 + len2 + 4 + 16 + carry + (code_bytes + 8 * move_words + 4 if tb else 0)


@pytest.mark.parametrize("affine", [False, True])
def test_slices_for_counts_the_carry(gl, affine):
    slices_for = gl.global_long_affine_slices_for if affine else gl.global_long_slices_for
    budget = 256 * _alignment_bytes(STRIPE, STRIPE, affine, True)          # the fixed-length entry's traceback budget
    for len1, len2 in ((MAX_LEN, MAX_LEN), (MAX_LEN, STRIPE), (129, 32769), (STRIPE, STRIPE + 1), (STRIPE, STRIPE)):
        s = min(max(budget // _alignment_bytes(len1, len2, affine, True), 1), 1 << 20)
        assert slices_for(2 * s + 1, len1, len2) == [s, s, 1], (len1, len2)
        assert slices_for(s, len1, len2) == [s] and slices_for(s + 1, len1, len2) == [s, 1]
        e = min(max((256 << 20) // _alignment_bytes(len1, len2, affine, False), 1), 1 << 20)
        assert slices_for(e + 2, len1, len2, traceback=False) == [e, 2], (len1, len2)
    # the known limit: 16 alignments of 65536 x 65536 per traceback slice, and the carry decides an ends-only slice's size
    assert slices_for(40, MAX_LEN, MAX_LEN) == [16, 16, 8]
    assert slices_for(1, MAX_LEN, MAX_LEN, traceback=False) == [1]
    with_carry = (256 << 20) // _alignment_bytes(MAX_LEN, MAX_LEN, affine, False)
    without = (256 << 20) // (2 * MAX_LEN + 20)
    assert slices_for(1 << 20, MAX_LEN, MAX_LEN, traceback=False)[0] == with_carry < without
    assert slices_for(5, 0, 5) == [] and slices_for(5, 5, MAX_LEN + 1) == []
    # where both lengths fit the fixed-length entry the slices are that entry's
    assert gl.global_long_slices_for(1000, STRIPE, STRIPE) == [256, 256, 256, 232]


def test_expand_moves_bounds(swmi_mod, gl):
    """End cells up to (65536, 65536), where swmi.local_full_expand_moves still stops at 16384."""
    moves = np.full(2, 0xFFFFFFFFFFFFFFFF, np.uint64)                      # 64 diagonal steps
    pos = gl.expand_moves(moves, 40, MAX_LEN, MAX_LEN)
    assert pos.shape == (41, 2) and tuple(pos[0]) == (MAX_LEN - 40, MAX_LEN - 40) and tuple(pos[-1]) == (MAX_LEN, MAX_LEN)
    assert gl.expand_moves(moves, 0, 0, 0).tolist() == [[0, 0]]
    assert gl.expand_moves(moves, 40, MAX_LEN, MAX_LEN, cap=3).tolist() == [[MAX_LEN - 40 + k] * 2 for k in range(3)]
    for end in ((MAX_LEN + 1, 5), (5, MAX_LEN + 1), (-1, 5)):
        with pytest.raises(swmi_mod.SwmiError):
            gl.expand_moves(moves, 1, *end)
    with pytest.raises(swmi_mod.SwmiError):
        gl.expand_moves(moves, 11, 5, 5)                                   # more steps than i + j
    with pytest.raises(swmi_mod.SwmiError):
        gl.expand_moves(np.zeros(2, np.uint64), 3, 5, 5)                   # a move of 0
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_full_expand_moves(moves, 1, STRIPE + 1, 5)
    assert gl.move_words(MAX_LEN, MAX_LEN) == 4096 and gl.move_words(1, 1) == 2 and gl.MAX_LEN == MAX_LEN


def test_key_range_under_the_domain_rule():
    """The arithmetic of global_long_kernels.hip's and global_long_affine_kernels.hip's key-range derivations: under
    P (len1 + len2) <= 2^23 every key H << 6 and every candidate fits 32 bits with room for the affine body's -inf."""
    bound = 1 << 23                                                        # |H| of a valid cell
    for p, total in ((128, 65536), (127, 66052), (64, 131072), (1, 131072)):
        assert p * total <= bound
    padded = bound + 1023 * 127                                            # a padded column loses at most a gap per column
    assert padded < bound + (1 << 17)
    assert (65536 + 95) * 127 < bound                                      # the left border's closed form past row len1
    key = padded << 6
    assert key < (1 << 29) + (1 << 23)
    assert key + (128 << 6) + (127 << 6) < 1 << 30                         # a candidate: a key plus a score, or less a gap
    minus_inf = -(1 << 30)
    assert -key - (127 << 6) > minus_inf                                   # every reachable E / F candidate beats -inf
    assert minus_inf - (127 << 6) > -(1 << 31)                             # -inf less one extend does not wrap
    # the reduction: H + bias is positive and fits the 30 bits above end_pack's two 17-bit fields, which hold 65536
    bias = 1 << 24
    assert bias - bound > 0 and bound + bias < 1 << 30 and 0x1FFFF - 65536 >= 0 and 30 + 17 + 17 == 64
    assert not (1 << 22) > bound                                           # the fixed-length kernels' bias would not do
    # indices at 65536 x 65536: code words per alignment exceed 2^28, bytes 2^30, so the kernels sum them as size_t
    words = 64 * _trips(65536) * 256
    assert _trips(65536) == 16400 and words == 268697600 and words * 4 > 1 << 30 and 16 * words * 8 < 1 << 36


def test_python_argument_checks(swmi_mod, gl):
    k = match_matrix(1, -1)
    a = np.zeros((2, 40), np.uint8)
    with pytest.raises(ValueError):
        gl.global_long(a, np.zeros((3, 40), np.uint8), k, 1)
    with pytest.raises(ValueError):
        gl.global_long(a[0], a, k, 1)
    with pytest.raises(ValueError):
        gl.global_long_affine(a, a, np.zeros(15, np.int8), 3, 1)
    for bad in (lambda: gl.global_long(a, a, k, 128), lambda: gl.global_long(a, a, k, 1, free_ends=16),
                lambda: gl.global_long(a, a, k, 1, free_ends=-1), lambda: gl.global_long_affine(a, a, k, 2**32 + 1, 1),
                lambda: gl.global_long_affine(a, a, k, 3, 128), lambda: gl.global_long(np.zeros((1, MAX_LEN + 1), np.uint8), a[:1], k, 1),
                lambda: gl.global_long(np.zeros((1, MAX_LEN), np.uint8), np.zeros((1, MAX_LEN), np.uint8), match_matrix(65, -1), 1)):
        with pytest.raises(swmi_mod.SwmiError):
            bad()
    # the package's own namespace holds the module, not its functions
    assert not hasattr(swmi_mod, "global_long_affine") and swmi_mod.global_long is gl


def test_cpp_header_compiles(tmp_path):
    """include/swmi_compat.hpp's NeedlemanWunsch_long_mi355x, NeedlemanWunsch_long_affine_mi355x and their batch forms compile
    and link against the library (tests/test_global_long_gpu.py runs the program)."""
    import os
    import shutil
    import subprocess

    from conftest import PKG, ROOT
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_long.cpp"), "-o", str(tmp_path / "compat_global_long"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
