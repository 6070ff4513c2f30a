"""libswmi_banded_ragged.so (include/swmi_banded_ragged.h) without a device: its nine exports and what it
links, its version, every refusal in the header's order (none of them touches a device: this machine has none), slices_for
recomputed from the header's arithmetic, the kernels' resources from the compiler's remarks, the support module's oracle
against the two restatements' batch functions, and the two fixed headers left as they were."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from banded_align_support import BandedOracle
from banded_global_support import BandedGlobalOracle
from banded_ragged_support import (ALL_MASKS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_SLICE, NO_ALIGNMENT, TB_BUDGET, Batch, RaggedOracle,
                                   per_alignment, slices_by_hand)
from conftest import PKG, ROOT, match_matrix

ENTRIES = ["swmi_banded_ragged_last_error", "swmi_banded_ragged_version", "swmi_banded_ragged_release_workspaces", "swmi_banded_ragged_local",
           "swmi_banded_ragged_global", "swmi_banded_ragged_local_device", "swmi_banded_ragged_global_device", "swmi_banded_ragged_slices_for",
           "swmi_banded_ragged_time_device"]
LIB = os.path.join(PKG, "lib", "libswmi_banded_ragged.so")


@pytest.fixture(scope="module")
def br(swmi_mod):
    swmi_mod.banded_ragged.load()
    return swmi_mod.banded_ragged


def test_header_declares_and_library_exports_exactly_the_nine_entries(br, swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi_banded_ragged.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 9
    assert "expand_moves(" not in header.replace("swmi_local_full_expand_moves", "")          # one expander: libswmi.so's
    assert "move_offsets(" not in header.replace("swmi_local_full_ragged_move_offsets", "")   # ... and one layout function
    for text in ("SWMI_BANDED_RAGGED_LOCAL 0", "SWMI_BANDED_RAGGED_GLOBAL 1", "SWMI_BANDED_RAGGED_SLOT_BYTES 48", "swmi_banded.h", "swmi_banded_global.h"):
        assert text in header, text
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}     # it calls nothing of libswmi.so
    dyn = subprocess.run(["readelf", "-d", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn)
    assert "libswmi.so" in needed and "$ORIGIN" in dyn
    allowed = re.compile(r"^(libswmi\.so|libamdhip64\.so(\.\d+)*|libstdc\+\+\.so\.6|libm\.so\.6|libgcc_s\.so\.1|libc\.so\.6|ld-linux-x86-64\.so\.2|"
                         r"libdl\.so\.2|libpthread\.so\.0)$")
    assert all(allowed.match(x) for x in needed), needed
    assert br.version() == swmi_mod.load().swmi_version() == 300


def test_the_two_fixed_libraries_and_modules_are_as_they_were(swmi_mod):
    for lib, count in (("libswmi_banded.so", 7), ("libswmi_banded_global.so", 7)):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", lib)], stdout=subprocess.PIPE, text=True, check=True).stdout
        names = [line.split()[-1] for line in syms.splitlines() if " T " in line]
        assert len(names) == count and not any("ragged" in x for x in names), names
    for name in ("swmi_banded.h", "swmi_banded_global.h"):
        with open(os.path.join(ROOT, "include", name)) as fh:
            text = fh.read()
        assert "KNOWN LIMITS: one (len1, len2) per call" in text and "ragged" not in text, name
    assert set(dir(swmi_mod.banded_ragged)) >= {"local", "global_", "local_device", "global_device", "time_device", "slices_for", "move_offsets",
                                                "paths", "release_workspaces", "version", "last_error"}


def test_every_refusal_in_the_stated_order_with_no_device(br, swmi_mod):
    """Each call below breaks several rules at once; the one that is reported is the first in the header's order: the mask, the
    matrix, the gaps, the moves / steps pair, n = 0, the buffers, the offsets, the alignment of device pointers."""
    lib = br.load()
    buf = np.zeros(4096, np.int64)
    sm = np.zeros(16, np.int8)
    good = np.array([0, 8, 16], np.uint64)
    decreasing = np.array([0, 8, 7], np.uint64)
    too_long = np.array([0, 8, 8 + 16385], np.uint64)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT
    ms = ctypes.c_float()

    def args(o1=good, o2=good, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return (s1, p(o1), s2, p(o2), n, dg, m, go, ge), (sc, en, mv, st)

    def calls(fe=0, **kw):
        head, tail = args(**kw)
        yield "global", lambda: lib.swmi_banded_ragged_global(*head, fe, *tail)
        yield "global_device", lambda: lib.swmi_banded_ragged_global_device(*head, fe, *tail, None)
        yield "time global", lambda: lib.swmi_banded_ragged_time_device(1, *head, fe, *tail, None, 1, ctypes.byref(ms))
        if fe <= 19:
            yield "local", lambda: lib.swmi_banded_ragged_local(*head, *tail)
            yield "local_device", lambda: lib.swmi_banded_ragged_local_device(*head, *tail, None)
            yield "time local", lambda: lib.swmi_banded_ragged_time_device(0, *head, fe, *tail, None, 1, ctypes.byref(ms))

    def refused(code, text, **kw):
        for name, call in calls(**kw):
            assert call() == code, (name, kw, br.last_error())
            assert text in br.last_error(), (name, br.last_error())

    # 1. the mask (global kind) before everything else; the local kind takes none, and its timer ignores it
    for bad in (20, 24, 32, 0xFFFFFFFF):
        refused(INV, "free_ends", fe=bad, m=None, go=200, mv=None, s1=None, o1=decreasing)
    head, tail = args()
    assert lib.swmi_banded_ragged_time_device(0, *head, 77, *(p(buf), p(buf), None, p(buf)), None, 1, ctypes.byref(ms)) == INV
    assert "moves and steps" in br.last_error()
    # 2. the matrix before the gaps
    refused(INV, "score_matrix is NULL", m=None, go=200, mv=None, s1=None, o1=decreasing)
    # 3. the gaps before the pair
    for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
        refused(DOM, "outside [0,127]", go=go, ge=ge, mv=None, s1=None, o1=decreasing)
    # 4. the pair before n = 0 and the buffers
    refused(INV, "moves and steps", mv=None, n=0, s1=None)
    refused(INV, "moves and steps", st=None, s1=None, o1=decreasing)
    # 5. n = 0 is SWMI_OK whatever the buffers and offsets are (the timer alone wants n > 0)
    for name, call in calls(n=0, s1=None, s2=None, sc=None, en=None, o1=None, o2=None):
        assert call() == (INV if name.startswith("time") else 0), name
    # 6. the buffers before the offsets; diagonals may be NULL
    for missing in ("s1", "s2", "sc", "en"):
        refused(INV, "NULL buffer", o1=decreasing, **{missing: None})
    # 7. the offsets: NULL, decreasing, a length above 16384 -- before the alignment of device pointers
    odd = p(buf) + 8
    refused(INV, "offsets is NULL", o1=None, s1=odd)
    refused(INV, "offsets is NULL", o2=None, s1=odd)
    refused(INV, "offsets decrease at alignment 1", o1=decreasing, s1=odd)
    refused(INV, "offsets decrease at alignment 1", o2=decreasing, s1=odd)
    refused(INV, "a length above 16384", o1=too_long, s1=odd)
    refused(INV, "a length above 16384", o2=too_long, sc=odd)
    # 8. 16-byte alignment of every device pointer (the host entries take any)
    for which in ("s1", "s2", "sc", "en", "mv", "st"):
        head, tail = args(**{which: odd})
        assert lib.swmi_banded_ragged_local_device(*head, *tail, None) == ALN, which
        assert lib.swmi_banded_ragged_global_device(*head, 19, *tail, None) == ALN, which
        assert lib.swmi_banded_ragged_time_device(1, *head, 19, *tail, None, 1, ctypes.byref(ms)) == ALN, which
        assert "16-byte aligned" in br.last_error()
    # the timer's own: kind, avg_ms, iters
    head, tail = args()
    assert lib.swmi_banded_ragged_time_device(2, *head, 0, *tail, None, 1, ctypes.byref(ms)) == INV and "kind 2" in br.last_error()
    assert lib.swmi_banded_ragged_time_device(0, *head, 0, *tail, None, 0, ctypes.byref(ms)) == INV
    assert lib.swmi_banded_ragged_time_device(0, *head, 0, *tail, None, 1, None) == INV
    # the module: one of the two sides of a different size, diagonals of the wrong size or outside int32
    with pytest.raises(ValueError):
        br.local([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)] * 2, sm, 1, 1)
    with pytest.raises(ValueError):
        br.local([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)], sm, 1, 1, diagonals=[0, 0])
    with pytest.raises(ValueError):
        br.global_([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)], sm, 1, 1, diagonals=np.array([2**31]))
    with pytest.raises(swmi_mod.SwmiError) as err:
        br.global_([np.zeros(3, np.uint8)], [np.zeros(3, np.uint8)], sm, 1, 1, free_ends=-1)
    assert err.value.code == INV and "free_ends" in str(err.value)
    with pytest.raises(swmi_mod.SwmiError) as err:
        br.local([np.zeros(16385, np.uint8)], [np.zeros(3, np.uint8)], sm, 1, 1, traceback=False)
    assert err.value.code == INV and "a length above 16384" in str(err.value)
    with pytest.raises(swmi_mod.SwmiError):                     # (with a traceback the layout function of libswmi.so refuses it first)
        br.local([np.zeros(16385, np.uint8)], [np.zeros(3, np.uint8)], sm, 1, 1)
    assert br.local([], [], sm, 1, 1)[0].shape == (0,)            # n = 0 needs no device


def test_slices_for_is_the_headers_arithmetic(br):
    # the count cap on a tiny shape, ends-only
    n = 2 * MAX_SLICE + 7
    off1, off2 = 3 * np.arange(n + 1, dtype=np.uint64), 2 * np.arange(n + 1, dtype=np.uint64)
    for kind in (LOCAL, GLOBAL):
        assert br.slices_for(kind, off1, off2, traceback=False) == [MAX_SLICE, MAX_SLICE, 7]
    assert per_alignment(LOCAL, 3, 2, False) * MAX_SLICE < 256 << 20
    # a mixed traceback batch whose byte budget binds in the middle: every fourth alignment is (16384, 700), the rest small
    rng = np.random.default_rng(1)
    shapes = [(16384, 700) if k % 4 == 0 else (int(rng.integers(0, 900)), int(rng.integers(0, 900))) for k in range(20000)]
    off1 = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.uint64)
    off2 = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.uint64)
    for kind in (LOCAL, GLOBAL):
        want = slices_by_hand(kind, shapes, True)
        assert br.slices_for(kind, off1, off2, traceback=True) == want
        assert len(want) >= 2 and 0 < want[0] < MAX_SLICE and sum(want) == len(shapes)
        at = want[0]
        used = sum(per_alignment(kind, *s, True) for s in shapes[:at])
        assert used <= TB_BUDGET < used + per_alignment(kind, *shapes[at], True)          # the longest run that fits
        assert br.slices_for(kind, off1, off2, traceback=False) == slices_by_hand(kind, shapes, False) == [len(shapes)]
    # the two kinds differ where len1 + 63 is a multiple of 4: the global kind sweeps row 0
    assert per_alignment(GLOBAL, 1, 1, True) == per_alignment(LOCAL, 1, 1, True) + 256
    assert per_alignment(GLOBAL, 2, 1, True) == per_alignment(LOCAL, 2, 1, True)
    # one alignment always fits; n = 0, an unknown kind and refused offsets give 0
    one = np.array([0, 16384], np.uint64)
    assert br.slices_for(LOCAL, one, one) == [1]
    assert br.slices_for(LOCAL, np.array([0], np.uint64), np.array([0], np.uint64)) == []
    assert br.slices_for(2, one, one) == [] and "kind 2" in br.last_error()
    assert br.slices_for(GLOBAL, np.array([0, 8, 7], np.uint64), np.array([0, 8, 9], np.uint64)) == [] and "decrease" in br.last_error()
    assert br.slices_for(GLOBAL, np.array([0, 16385], np.uint64), one) == [] and "16384" in br.last_error()
    lib = br.load()
    assert lib.swmi_banded_ragged_slices_for(0, None, one.ctypes.data, 1, 1, None, 0) == 0 and "NULL" in br.last_error()
    # sizes beyond cap are counted and not written
    buf = (ctypes.c_size_t * 2)(0, 99)
    assert lib.swmi_banded_ragged_slices_for(0, off1.ctypes.data, off2.ctypes.data, len(shapes), 1, buf, 1) == len(want) and buf[1] == 99


def test_kernel_resources_no_scratch_no_spill_and_the_fixed_kernels_lds(tmp_path):
    """The compiler's own remarks for csrc/banded_ragged_kernels.hip with the Makefile's flags: eight kernels, none with
    scratch or a spilled register, 16 KiB of LDS with a traceback and none without."""
    src = os.path.join(PKG, "csrc", "banded_ragged_kernels.hip")
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall",
                          "-Wno-unused-function", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                          str(tmp_path / "k.o"), src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-3000:]
    kernels = {}
    name = None
    for line in run.stdout.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    assert len(kernels) == 8, sorted(kernels)
    assert sum("banded_ragged_local_kernel" in k for k in kernels) == 4 and sum("banded_ragged_global_kernel" in k for k in kernels) == 4
    for k, r in kernels.items():
        traceback = re.search(r"kernelILb[01]ELb1E", k) is not None
        assert r["ScratchSize"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == (16384 if traceback else 0), (k, r)
        assert r["VGPRs"] <= 128, (k, r)


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return RaggedOracle(tmp_path_factory.mktemp("banded_ragged_oracle"))


def test_the_support_oracle_is_the_two_restatements_alignment_by_alignment(orc, tmp_path):
    """The mixed-batch oracle against the restatements' own batch functions on batches of one shape, and its zero lengths
    against the header's closed forms."""
    rng = np.random.default_rng(3)
    fixed_local, fixed_global = BandedOracle(tmp_path), BandedGlobalOracle(tmp_path)
    a, b = rng.integers(0, 4, (5, 90), dtype=np.uint8), rng.integers(0, 4, (5, 70), dtype=np.uint8)
    b[:3, :60] = a[:3, 10:70]
    d = np.array([0, -10, 30, 100, INT32_MIN], np.int32)
    batch = Batch(list(a), list(b), d)
    sm = match_matrix(2, -3)
    for tb in (True, False):
        sc, ends, mv, st = orc.align(LOCAL, batch, sm, 5, 1, traceback=tb)
        wsc, wends, wmv, wst = fixed_local.align(a, b, sm, 5, 1, d, traceback=tb)
        assert np.array_equal(sc, wsc) and np.array_equal(ends, wends) and sc.max() > 50
        if tb:
            assert np.array_equal(st, wst) and np.array_equal(mv.reshape(5, -1), wmv)
        for mask in ALL_MASKS:
            sc, ends, mv, st = orc.align(GLOBAL, batch, sm, 5, 1, mask, traceback=tb)
            wsc, wends, wmv, wst = fixed_global.align(a, b, sm, 5, 1, mask, d, traceback=tb)
            assert np.array_equal(sc, wsc) and np.array_equal(ends, wends), mask
            if tb:
                assert np.array_equal(st, wst), mask
    # zero lengths: the local kind's closed form whatever the diagonal; the global kind's border
    e = np.zeros(0, np.uint8)
    five = np.array([0, 1, 2, 3, 0], np.uint8)
    zero = Batch([e, five, e, e, five], [five, e, e, five, e], np.array([0, 0, 0, 70, INT32_MAX], np.int32))
    sc, ends, mv, st = orc.align(LOCAL, zero, sm, 5, 1)
    assert not sc.any() and not ends.any() and not st.any()
    assert np.array_equal(orc.align(LOCAL, zero, sm, 5, 1, traceback=False)[1], np.tile([0, 0, -1, -1], (5, 1)))
    sc, ends, mv, st = orc.align(GLOBAL, zero, sm, 5, 1, 0)
    assert list(sc) == [-9, -9, 0, NO_ALIGNMENT, NO_ALIGNMENT]        # open + 4 extend; (0, 0) alone; the band misses (0, 5) and (5, 0)
    assert list(map(tuple, ends)) == [(0, 5, 0, 0), (5, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)] and list(st) == [5, 5, 0, 0, 0]
    sc, ends, mv, st = orc.align(GLOBAL, zero, sm, 5, 1, 3)           # both begins free: no cost, no forced step
    assert list(sc[:3]) == [0, 0, 0] and list(st[:3]) == [0, 0, 0] and tuple(ends[0]) == (0, 5, 0, 5)
    sc, ends, mv, st = orc.align(GLOBAL, zero, sm, 5, 1, 16)          # the end anywhere: (0, 0) holds the best, 0
    assert list(sc[:3]) == [0, 0, 0] and not ends[:3].any()
