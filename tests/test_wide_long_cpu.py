"""The long wide-alphabet aligners' host-only parts, no device needed (libswmi_wide_long.so, include/swmi_wide_long.h,
swmi.wide_long): the header and the library's symbols; every refusal with code and text, in swmi_wide.h's order, in a process
with no GPU bound -- a length of 65537 in either place, the global kind's domain rule on both sides of its edge, no such rule
for the local kind, a stripe width that is not shipped; swmi_wide_long_move_offsets and swmi_wide_long_slices_for on
hand-checkable offsets, a slot's carry bytes included; the module; the arithmetic of the kernel file's key-range derivation."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG, ROOT

ENTRIES = ["swmi_wide_long_local", "swmi_wide_long_global", "swmi_wide_long_local_device", "swmi_wide_long_global_device",
           "swmi_wide_long_slices_for", "swmi_wide_long_move_offsets", "swmi_wide_long_time_device", "swmi_wide_long_release_workspaces",
           "swmi_wide_long_set_stripe_waves", "swmi_wide_long_last_error", "swmi_wide_long_version"]
MAX = 65536


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


@pytest.fixture(scope="module")
def wl(swmi_mod):
    swmi_mod.wide_long.load()
    return swmi_mod.wide_long


def test_header_declares_and_library_exports_the_entries(wl):
    with open(os.path.join(ROOT, "include", "swmi_wide_long.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert '#include "swmi_wide.h"' in header and "swmi_wide_long_expand_moves" not in header     # one expander: libswmi.so's
    lib = os.path.join(PKG, "lib", "libswmi_wide_long.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    taken = {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}
    assert taken <= {"swmi_local_long_expand_moves", "swmi_last_error"}, taken
    assert wl.version() == 300
    # the two older libraries keep their entries: the nine of libswmi_wide.so are pinned by test_wide_cpu.py


def test_every_refusal_works_with_no_device(wl, swmi_mod):
    lib = wl.load()
    sm = np.zeros(1024, np.int8)
    s1, s2 = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    out = np.zeros(64, np.int64)
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    too_long = np.array([0, 3, 3 + MAX + 1, 3 + MAX + 2, 3 + MAX + 3], np.uint64)      # a length of 65537
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT

    def local(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_long_local(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st)

    def glob(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_long_global(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st)

    def local_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_long_local_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, sc, en, mv, st, None)

    def glob_dev(o1, o2, go=1, ge=1, s1p=p(s1), s2p=p(s2), mv=p(out), st=p(out), n=4, smp=p(sm), sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_long_global_device(s1p, p(o1), s2p, p(o2), n, smp, go, ge, mask, sc, en, mv, st, None)

    for f in (local, glob, local_dev, glob_dev):
        assert f(too_long, good) == INV and "seq1_offsets: sequence 1 has length 65537 > 65536" in wl.last_error()
        assert f(good, too_long) == INV and "seq2_offsets: sequence 1 has length 65537 > 65536" in wl.last_error()
        assert f(bad_dec, good) == INV and "seq1_offsets decrease at 1" in wl.last_error()
        assert f(good, bad_dec) == INV and "seq2_offsets decrease at 1" in wl.last_error()
        assert f(None, good) == INV and "seq1_offsets is NULL" in wl.last_error()
        assert f(good, None) == INV and "seq2_offsets is NULL" in wl.last_error()
        assert f(good, good, mv=None) == INV and "moves and steps" in wl.last_error()
        assert f(good, good, st=None) == INV and "moves and steps" in wl.last_error()
        for name in ("s1p", "s2p", "sc", "en"):
            assert f(good, good, **{name: None}) == INV and "NULL buffer" in wl.last_error(), name
        assert f(good, good, smp=None) == INV and "score_matrix is NULL" in wl.last_error()
        for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
            assert f(good, good, go=go, ge=ge) == DOM and "outside [0,127]" in wl.last_error()
        # n = 0 returns before the buffers and the offsets are looked at, but after the matrix, the gaps and moves / steps
        assert f(bad_dec, None, n=0, s1p=None) == 0
        assert f(good, good, n=0, go=200) == DOM and f(good, good, n=0, mv=None) == INV
        # the order: gaps before the moves / steps pair, that before the buffers, those before the offsets
        assert f(bad_dec, good, go=-1, mv=None) == DOM and f(bad_dec, good, mv=None, sc=None) == INV and "moves and steps" in wl.last_error()
        assert f(bad_dec, good, sc=None) == INV and "NULL buffer" in wl.last_error()
    for f in (glob, glob_dev):
        assert f(good, good, mask=16) == INV and "free_ends 16 above 15" in wl.last_error()
        assert f(good, good, mask=16, go=-1) == INV                       # the mask comes first
    for f in (local_dev, glob_dev):
        assert f(good, good, sc=p(out) + 8) == ALN and "16-byte aligned" in wl.last_error()
    ms = ctypes.c_float()
    t = lambda kind=0, iters=1, n=4, ms=ctypes.byref(ms): lib.swmi_wide_long_time_device(kind, p(s1), p(good), p(s2), p(good), n, p(sm), 1, 1, 0,   # noqa: E731
                                                                                          p(out), p(out), None, None, None, iters, ms)
    assert t(kind=2) == INV and t(iters=0) == INV and t(n=0) == INV and t(ms=None) == INV
    # the stripe width: 0, 1 and 4 are shipped (2 won no row of the measurement and is not built)
    for w in (2, 3, 5, 8, 16, -1):
        assert lib.swmi_wide_long_set_stripe_waves(w) == INV and "stripe width %d is not shipped" % w in wl.last_error()
        with pytest.raises(swmi_mod.SwmiError) as e:
            wl.set_stripe_waves(w)
        assert e.value.code == INV
    for w in (1, 4, 0):
        assert lib.swmi_wide_long_set_stripe_waves(w) == 0
    # the Python layer: what ctypes would wrap raises, as elsewhere
    seqs = [np.zeros(3, np.uint8)]
    with pytest.raises(swmi_mod.SwmiError) as e:
        wl.local(seqs, seqs, sm, 2**32 + 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wl.global_(seqs, seqs, np.full(1024, 300), 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wl.global_(seqs, seqs, sm, 1, 1, free_ends=-1)
    assert e.value.code == INV
    with pytest.raises(swmi_mod.SwmiError) as e:
        wl.local([np.zeros(3, np.uint8)], [np.zeros(MAX + 1, np.uint8)], sm, 1, 1)
    assert e.value.code == INV and "65537" in str(e.value)
    with pytest.raises(ValueError):
        wl.local(seqs, seqs, np.zeros(16, np.int8), 1, 1)
    r = wl.local([], [], sm, 1, 1)          # an empty batch needs no device
    assert len(r[0]) == 0 and r[1].shape == (0, 4)


def test_domain_rule_at_its_edge(wl, swmi_mod):
    """Global kind: P (len1 + len2) <= 2^23 with P = max(1, max |matrix|, gaps), checked last, the text naming the first
    offending alignment.  An accepted call goes on to look for a device; in a process without one it comes back with another
    status (with one, it runs: the buffers are real).  Local kind: no rule."""
    lib = wl.load()
    INV, DOM = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN
    s1, s2 = np.zeros(MAX, np.uint8), np.zeros(2 * MAX, np.uint8)
    sc, en = np.zeros(4, np.int32), np.zeros(16, np.int32)
    accepted = lambda rc: rc not in (INV, DOM)   # noqa: E731

    def glob(lens, sm, go=0, ge=0):
        o1, o2 = _off([x for x, _ in lens]), _off([y for _, y in lens])
        return lib.swmi_wide_long_global(s1.ctypes.data, o1.ctypes.data, s2.ctypes.data, o2.ctypes.data, len(lens), sm.ctypes.data, go, ge, 0,
                                         sc.ctypes.data, en.ctypes.data, None, None)

    def local(lens, sm, go=0, ge=0):
        o1, o2 = _off([x for x, _ in lens]), _off([y for _, y in lens])
        return lib.swmi_wide_long_local(s1.ctypes.data, o1.ctypes.data, s2.ctypes.data, o2.ctypes.data, len(lens), sm.ctypes.data, go, ge,
                                        sc.ctypes.data, en.ctypes.data, None, None)

    m128, m127, m1 = np.full(1024, -128, np.int8), np.full(1024, 127, np.int8), np.full(1024, 1, np.int8)
    assert 128 * (3 + 65533) == 1 << 23
    assert accepted(glob([(3, 65533)], m128))
    assert glob([(3, 65534)], m128) == INV
    assert "alignment 0 is outside the domain" in wl.last_error() and "128 x 65537 > 2^23" in wl.last_error()
    assert glob([(5, 5), (3, 65533), (3, 65534), (4, 65534)], m128) == INV and "alignment 2 is outside" in wl.last_error()
    # every shape that swmi_wide_global takes passes: 128 * 20480 < 2^23
    assert 128 * (16384 + 4096) < 1 << 23 and accepted(glob([(16384, 4096)], m128, 127, 127))
    # the all 127 matrix with gaps (0, 0) takes 65536 + 3; a gap of 128 would not exist, one of 127 changes nothing, P stays 127
    assert 127 * 65539 <= 1 << 23 and accepted(glob([(3, 65536)], m127)) and accepted(glob([(3, 65536)], m127, 127, 127))
    assert 127 * 66053 > 1 << 23 and glob([(517, 65536)], m127) == INV and accepted(glob([(516, 65536)], m127))
    # the gaps count: P = 65 at a matrix of 1
    assert 64 * 131072 == 1 << 23 and glob([(65536, 65536)], m1, 65, 0) == INV and glob([(65536, 65536)], m1, 0, 65) == INV
    assert accepted(glob([(65536, 1)], m1, 127, 0))
    assert accepted(glob([(65536, 65536)], np.zeros(1024, np.int8)))           # P = max(1, ..): never 0
    # the rule comes after the offsets: a length above the limit is reported as that
    assert glob([(3, 65537)], m128) == INV and "length 65537 > 65536" in wl.last_error()
    # no rule for the local kind
    assert accepted(local([(3, 65534)], m128, 127, 127))


def test_move_offsets_on_hand_checkable_offsets(wl, swmi_mod):
    # SWMI_LOCAL_LONG_MOVE_WORDS: ((len1 + len2 + 31) / 32 + 1) & ~1
    lens = [(3, 5), (0, 0), (65536, 65536), (100, 28), (16384, 4096)]
    off1, off2 = _off([x for x, _ in lens]), _off([y for _, y in lens])
    assert wl.move_offsets(off1, off2).tolist() == [0, 2, 2, 4098, 4102, 4102 + 640]
    # on the shapes of swmi.wide the layout is the package's
    small = [(3, 5), (0, 0), (16384, 4096), (100, 28)]
    o1, o2 = _off([x for x, _ in small]), _off([y for _, y in small])
    assert np.array_equal(wl.move_offsets(o1, o2), swmi_mod.local_full_ragged_move_offsets(o1, o2))
    assert wl.move_offsets(np.zeros(1, np.uint64), np.zeros(1, np.uint64)).tolist() == [0]
    too_long = _off([3, MAX + 1])
    with pytest.raises(swmi_mod.SwmiError) as e:
        wl.move_offsets(too_long, _off([3, 3]))
    assert e.value.code == swmi_mod.ERR_INVALID_ARGUMENT and "65537 > 65536" in str(e.value)
    with pytest.raises(swmi_mod.SwmiError):
        wl.move_offsets(np.array([0, 5, 3], np.uint64), _off([3, 3]))
    lib = wl.load()
    assert lib.swmi_wide_long_move_offsets(o1.ctypes.data, o2.ctypes.data, 4, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert lib.swmi_wide_long_move_offsets(None, o2.ctypes.data, 4, o1.ctypes.data) == swmi_mod.ERR_INVALID_ARGUMENT


def _striped(len1, len2):
    return len1 > 0 and len2 > 0 and (len1 > 16384 or len2 > 4096)


def _bytes(len1, len2, tb):
    """Device bytes of one alignment of a slice: inputs, 48 of slot, 20 of results, the carry (8 len1) of a striped slot of more
    than 1024 columns, and with a traceback codes (a qword per lane and row of the padded sweep), moves and steps."""
    b = len1 + len2 + 48 + 20
    if _striped(len1, len2) and len2 > 1024:
        b += 8 * len1
    if tb:
        trips = ((len1 + 63 + 31) // 32) * 8
        codes = ((len2 + 1023) // 1024) * trips * 256 if len1 and len2 else 0
        b += 4 + 8 * (codes + ((((len1 + len2 + 31) // 32) + 1) & ~1))
    return b


def test_slices_for_on_hand_checkable_offsets(wl):
    lib = wl.load()
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    too_long = np.array([0, 3, 3 + MAX + 1, 3 + MAX + 2, 3 + MAX + 3], np.uint64)
    ok = np.array([0, 3, 3 + MAX, 3 + MAX + 2, 3 + MAX + 3], np.uint64)
    for tb in (0, 1):
        for bad in (bad_dec, None, too_long):
            assert lib.swmi_wide_long_slices_for(p(bad), p(good), 4, tb, None, 0) == 0
            assert lib.swmi_wide_long_slices_for(p(good), p(bad), 4, tb, None, 0) == 0
        assert lib.swmi_wide_long_slices_for(p(good), p(ok), 4, tb, None, 0) == 1 and lib.swmi_wide_long_slices_for(p(ok), p(ok), 4, tb, None, 0) == 1
        sizes = (ctypes.c_size_t * 2)(99, 99)
        assert lib.swmi_wide_long_slices_for(p(good), p(good), 4, tb, sizes, 2) == 1
        assert list(sizes) == [4, 99]
    one = np.zeros(1, np.uint64)
    assert wl.slices_for(one, one) == []
    # the count cap: a slice holds at most 2^20 alignments
    n = (1 << 20) + 5
    rng = np.random.default_rng(2)
    assert wl.slices_for(_off(rng.integers(0, 5, n)), _off(rng.integers(0, 5, n)), traceback=False) == [1 << 20, 5]
    # the known limit: the traceback budget is what 16 alignments of 65536 x 65536 take, carry included
    assert wl.slices_for(_off([MAX] * 40), _off([MAX] * 40)) == [16, 16, 8]
    assert _bytes(MAX, MAX, True) == 2 * MAX + 68 + 8 * MAX + 4 + 8 * (64 * 16400 * 256 + 4096)
    budget = 16 * _bytes(MAX, MAX, True)
    # ... and smaller shapes fill it by bytes; a slot's carry counts where it is striped over more than 1024 columns
    for len1, len2 in ((16384, 16384), (20000, 1025), (20000, 1024), (16384, 4096), (300, 4097), (16385, 1)):
        s = budget // _bytes(len1, len2, True)
        assert 16 < s < 1 << 20
        assert wl.slices_for(_off([len1] * (2 * s + 1)), _off([len2] * (2 * s + 1))) == [s, s, 1], (len1, len2)
    assert _bytes(20000, 1025, False) - _bytes(20000, 1024, False) == 1 + 8 * 20000        # one column more: a carry block
    assert _bytes(16384, 4096, False) == 16384 + 4096 + 68 and _bytes(16385, 4096, False) == 16385 + 4096 + 68 + 8 * 16385
    assert _bytes(0, 65536, False) == 65536 + 68                                          # a zero length is not striped
    # ends-only: 256 MiB of inputs, slots, results and carry
    for len1, len2 in ((MAX, MAX), (20000, 1025), (20000, 1024), (16384, 4096)):
        per = (256 << 20) // _bytes(len1, len2, False)
        assert wl.slices_for(_off([len1] * (per + 7)), _off([len2] * (per + 7)), traceback=False) == [per, 7], (len1, len2)
    # a mixed batch: the running sum in caller order decides
    lens = [(MAX, MAX)] * 10 + [(16384, 4096)] * 100 + [(MAX, MAX)] * 10
    first, total = [], 0
    for x, (len1, len2) in enumerate(lens):
        b = _bytes(len1, len2, True)
        if total and total + b > budget:
            first.append(x)
            total = 0
        total += b
    want = [b - a for a, b in zip([0] + first, first + [len(lens)])]
    assert len(want) == 2 and wl.slices_for(_off([x for x, _ in lens]), _off([y for _, y in lens])) == want


def test_module_is_a_submodule_with_docstrings(swmi_mod):
    wl = swmi_mod.wide_long
    assert isinstance(wl, types.ModuleType) and wl.__name__ == "swmi.wide_long" and wl.__doc__
    public = ["local", "global_", "local_device", "global_device", "slices_for", "move_offsets", "time_device", "release_workspaces",
              "set_stripe_waves", "last_error", "version", "load"]
    for name in public:
        fn = getattr(wl, name)
        assert inspect.isfunction(fn) and fn.__module__ == "swmi.wide_long" and fn.__doc__, name
    # the matrices are swmi.wide's, not copies
    assert wl.match_matrix is swmi_mod.wide.match_matrix and wl.embed_dna is swmi_mod.wide.embed_dna
    # the call shapes are swmi.wide's
    for name in ("local", "global_", "local_device", "global_device", "slices_for", "time_device", "release_workspaces"):
        assert inspect.signature(getattr(wl, name)) == inspect.signature(getattr(swmi_mod.wide, name)), name
    for name in ("set_stripe_waves", "wide_long_local", "move_offsets"):
        assert not hasattr(swmi_mod, name), name
    top = [n for n, f in vars(swmi_mod).items() if inspect.isfunction(f) and f.__module__ == "swmi" and not n.startswith("_")]
    assert len(top) == 94
    assert wl.MAX_LEN == MAX and wl.STRIPE_WAVES == (1, 4)


def test_key_range_of_the_striped_wide_kernels():
    """The arithmetic of wide_long_affine_kernels.hip's key-range derivation, for matrices that may hold -128."""
    bound = 1 << 23
    # global kind, under P (len1 + len2) <= 2^23: |H| of a valid cell is at most P per move of a path of at most len1 + len2 moves
    for p, total in ((128, 65536), (127, 66052), (64, 131072), (1, 131072)):
        assert p * total <= bound
    assert 128 * 65537 > bound and 128 * (16384 + 4096) < bound             # -128 in the matrix: len1 + len2 <= 65536; the old domain fits
    padded = bound + 1023 * 127                                            # a padded column lies at most 1023 columns and one gap run away
    key = padded << 6
    assert key < (1 << 29) + (1 << 23)
    assert key + (128 << 6) + (127 << 6) < 1 << 30                         # a candidate: a key plus a score, or less a gap
    minus_inf = -(1 << 30)
    assert -key - (127 << 6) > minus_inf                                   # every reachable E / F candidate beats -inf
    assert minus_inf - (127 << 6) > -(1 << 31)                             # -inf less one extend does not wrap
    # the reduction: H + bias is positive and fits the 30 bits above end_pack's two 17-bit fields, which hold 65536
    bias = 1 << 24
    assert bias - bound > 0 and bound + bias < 1 << 30 and 0x1FFFF - 65536 >= 0 and 30 + 17 + 17 == 64
    # the unstriped kernels' bias of 2^22 covers 128 (16384 + 4096) and not 128 (16385 + 1): len1 > 16384 is striped whatever len2
    assert 128 * (16384 + 4096) < 1 << 22 < 128 * (32768 + 1) and 128 * (65536 + 3) > 1 << 22
    # local kind: no rule.  0 <= H <= 127 * 65536 < 2^23, and the pack holds it above the same two fields
    assert 127 * 65536 < bound and (127 * 65536) << 6 < 1 << 30 and (127 * 65536) < 1 << 30
    # indices at 65536 x 65536: code words per alignment exceed 2^28, so the kernels sum them as size_t; a slot's lanes
    trips = ((65536 + 63 + 31) // 32) * 8
    assert trips == 16400 and 64 * trips * 256 == 268697600 and 16 * 64 * trips * 256 * 8 < 1 << 36
    for w in (1, 4):
        assert (1024 * w) // 16 == 64 * w                                  # lanes per stripe: kStripeCols / kCols, not 64 max(w, 2)
    assert 64 * max(1, 2) != 1024 // 16
    # LDS: 32 KiB of profile a wavefront, the ring, the reduction's words: at most 160 KiB at 4 wavefronts
    assert 4 * 32768 + 3 * 256 * 8 + 4 * 8 + 3 * 4 <= 137264 <= 160 * 1024
    # carry blocks: TileWork::pad counts units of 2 int2; a slice's carry bytes lie within the traceback budget, below 2^35
    assert 16 * (2 * 65536 + 72 + 8 * 65536 + 8 * (268697600 + 4096)) < 1 << 36
