"""libswmi_banded_long.so (include/swmi_banded_long.h) without a device: its ten exports and the unchanged
sets of its siblings, every refusal with the band first and the length bound of 65536, slices_for against values worked out by
hand for 65536-long alignments at every width and both budgets, the tenth export against swmi.wide_long.move_offsets, the 32
kernels' resources from the compiler's remarks beside the width kernels', the compat header (compiled against the real
libraries, and run over the host source on the fake GPU as a stand-alone ASan + UBSan program), and the module's signatures.
The host source's own driver runs from tests/test_banded_long_host_fake.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from banded_long_support import (EO_BUDGET, GLOBAL, LOCAL, MAX_LEN, TB_BUDGET, WIDTHS, code_bytes, move_words, per_alignment, slices_by_hand)
from conftest import PKG, ROOT

NAMES = ["last_error", "version", "release_workspaces", "local", "global", "local_device", "global_device", "slices_for", "time_device"]
ENTRIES = ["swmi_banded_long_" + x for x in NAMES + ["move_offsets"]]
LIB_DIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIB_DIR, "libswmi_banded_long.so")
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def bl(swmi_mod):
    swmi_mod.banded_long.load()
    return swmi_mod.banded_long


def exported(lib):
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {line.split()[-1] for line in syms.splitlines() if " T " in line}


def test_header_declares_and_library_exports_exactly_the_ten_entries(bl, swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi_banded_long.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 10
    assert "expand_moves(" not in header                                            # one expander: libswmi.so's
    for text in ("SWMI_BANDED_LONG_MAX_LEN 65536", "NO DOMAIN RULE", "[-127 * 131072 - 254, 127 * 65536]", "KNOWN LIMITS: one band width per call",
                 "4 letters", "131072 dependent steps", "a length above 65536"):
        assert text in header, text
    for m in re.finditer(r"swmi_banded_long_(?:local|global)(?:_device)?\(([^;]*?)\);", header, re.S):
        assert re.search(r"diagonals,\s+int band,\s+const int8_t score_matrix\[16\]", m.group(1)), m.group(0)
    assert exported(LIB) == set(ENTRIES), sorted(exported(LIB) ^ set(ENTRIES))
    # the siblings' sets are what they were
    assert exported(os.path.join(LIB_DIR, "libswmi_banded_width.so")) == {"swmi_banded_width_" + x for x in NAMES}
    assert exported(os.path.join(LIB_DIR, "libswmi_banded_ragged.so")) == {"swmi_banded_ragged_" + x for x in NAMES}
    undefined = subprocess.run(["nm", "-D", "--undefined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}     # it calls nothing of libswmi.so
    dyn = subprocess.run(["readelf", "-d", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn)
    assert "libswmi.so" in needed and "$ORIGIN" in dyn and not [x for x in needed if "wide" in x or "banded" in x]
    assert bl.version() == swmi_mod.load().swmi_version()


def test_every_refusal_with_the_band_first_and_the_length_bound(bl, swmi_mod):
    """The width header's order: a bad band before every other broken rule, then the mask, the matrix, the gaps, the moves /
    steps pair, n = 0, the buffers, the offsets -- where a length of 65537 is refused and 65536 and 16385 are not -- and the
    alignment of device pointers.  None touches a device."""
    lib = bl.load()
    buf = np.zeros(4096, np.int64)
    sm = np.zeros(16, np.int8)
    good = np.array([0, 8, 16], np.uint64)
    decreasing = np.array([0, 8, 7], np.uint64)
    too_long = np.array([0, 8, 8 + 65537], np.uint64)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT
    ms = ctypes.c_float()

    def args(band=256, o1=good, o2=good, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return (s1, p(o1), s2, p(o2), n, dg, band, m, go, ge), (sc, en, mv, st)

    def calls(fe=0, **kw):
        head, tail = args(**kw)
        yield "global", lambda: lib.swmi_banded_long_global(*head, fe, *tail)
        yield "global_device", lambda: lib.swmi_banded_long_global_device(*head, fe, *tail, None)
        yield "time global", lambda: lib.swmi_banded_long_time_device(1, *head, fe, *tail, None, 1, ctypes.byref(ms))
        if fe <= 19:
            yield "local", lambda: lib.swmi_banded_long_local(*head, *tail)
            yield "local_device", lambda: lib.swmi_banded_long_local_device(*head, *tail, None)
            yield "time local", lambda: lib.swmi_banded_long_time_device(0, *head, fe, *tail, None, 1, ctypes.byref(ms))

    def refused(code, text, **kw):
        for name, call in calls(**kw):
            assert call() == code, (name, kw, bl.last_error())
            assert text in bl.last_error(), (name, bl.last_error())

    for bad in (0, 64, 127, 192, 2048, -128, 2**31 - 1, -2**31):
        refused(INV, "band %d is not one of 128, 256, 512, 1024" % bad, band=bad, fe=20, m=None, go=200, mv=None, s1=None, o1=too_long)
        refused(INV, "band", band=bad, n=0)
    odd = p(buf) + 8
    for band in WIDTHS:
        for bad in (20, 0xFFFFFFFF):
            refused(INV, "free_ends", band=band, fe=bad, m=None, go=200, mv=None, s1=None, o1=too_long)
        refused(INV, "score_matrix is NULL", band=band, m=None, go=200, mv=None, s1=None, o1=too_long)
        refused(DOM, "outside [0,127]", band=band, go=128, mv=None, s1=None, o1=too_long)
        refused(INV, "moves and steps", band=band, mv=None, n=0, s1=None)
        for name, call in calls(band=band, n=0, s1=None, s2=None, sc=None, en=None, o1=None, o2=None):
            assert call() == (INV if name.startswith("time") else 0), name
        refused(INV, "NULL buffer", band=band, o1=too_long, s2=None)
        refused(INV, "offsets is NULL", band=band, o1=None, s1=odd)
        refused(INV, "offsets decrease at alignment 1", band=band, o2=decreasing, s1=odd)
        refused(INV, "alignment 1: a length above 65536", band=band, o1=too_long, s1=odd)
        refused(INV, "alignment 1: a length above 65536", band=band, o2=too_long, s1=odd)
        for which in ("s1", "sc", "mv"):
            head, tail = args(band=band, **{which: odd})
            assert lib.swmi_banded_long_local_device(*head, *tail, None) == ALN, which
            assert lib.swmi_banded_long_global_device(*head, 19, *tail, None) == ALN, which
        # the bound itself: 65537 no, 65536 and 16385 yes
        for kind in (LOCAL, GLOBAL):
            assert bl.slices_for(kind, band, too_long, good) == [] and "a length above 65536" in bl.last_error()
            assert bl.slices_for(kind, band, np.array([0, 65536, 131072], np.uint64), np.array([0, 65536, 65536 + 16385], np.uint64)) == [2]
            assert bl.slices_for(kind, band, np.array([0, 16385], np.uint64), np.array([0, 0], np.uint64), traceback=False) == [1]
    head, tail = args()
    assert lib.swmi_banded_long_time_device(2, *head, 0, *tail, None, 1, ctypes.byref(ms)) == INV and "kind 2" in bl.last_error()
    assert bl.slices_for(2, 128, good, good) == [] and "kind 2" in bl.last_error()
    assert bl.slices_for(LOCAL, 192, good, good) == [] and "band 192" in bl.last_error()
    # the module
    one = [np.zeros(3, np.uint8)]
    with pytest.raises(swmi_mod.SwmiError) as err:
        bl.local(one, one, 100, sm, 1, 1)
    assert err.value.code == INV and "band 100" in str(err.value)
    with pytest.raises(swmi_mod.SwmiError) as err:
        bl.local([np.zeros(65537, np.uint8)], one, 128, sm, 1, 1)
    assert err.value.code == INV and "a length above 65536" in str(err.value)
    assert bl.local([], [], 1024, sm, 1, 1)[0].shape == (0,)            # n = 0 needs no device


def test_slices_for_by_hand_for_65536_long_alignments(bl):
    """65536 x 65536, by hand.  Ends-only an alignment takes 65536 + 65536 + 48 + 20 = 131 140 bytes at every width: 256 MiB =
    268 435 456 hold 2046 (2046 * 131 140 = 268 312 440; one more is 268 443 580).  With a traceback it takes its codes, 256 K
    bytes for each of ceil((65536 + 63 or 64) / 4) = 16400 trips, 8 * 4096 of moves and 4 of steps: 163 912 + 4 198 400 K, and
    4 383 801 344 bytes hold 1004, 512, 258 and 129 of them at K = 1, 2, 4, 8:
        1004 * 4 362 312 = 4 379 761 248     1005 * 4 362 312 = 4 384 123 560
         512 * 8 560 712 = 4 383 084 544      513 * 8 560 712 = 4 391 645 256
         258 * 16 957 512 = 4 375 038 096     259 * 16 957 512 = 4 391 995 608
         129 * 33 751 112 = 4 353 893 448     130 * 33 751 112 = 4 387 644 560
    and of (65536, 600) at band 1024 -- 66 204 + 33 587 200 + 8 * 2068 + 4 = 33 669 952 -- 130."""
    assert EO_BUDGET == 268435456 and TB_BUDGET == 4383801344 and move_words(65536, 65536) == 4096 and move_words(65536, 600) == 2068
    m = 2100
    off = MAX_LEN * np.arange(m + 1, dtype=np.uint64)
    short = 600 * np.arange(m + 1, dtype=np.uint64)
    by_hand = {128: 1004, 256: 512, 512: 258, 1024: 129}
    for band in WIDTHS:
        k = band // 128
        for kind in (LOCAL, GLOBAL):
            assert code_bytes(kind, 65536, band) == 4198400 * k
            assert per_alignment(kind, 65536, 65536, band, True) == 163912 + 4198400 * k
            assert bl.slices_for(kind, band, off, off, traceback=False) == [2046, m - 2046]
            fit = by_hand[band]
            want = [fit] * (m // fit) + ([m % fit] if m % fit else [])
            assert bl.slices_for(kind, band, off, off, traceback=True) == want == slices_by_hand(kind, [(65536, 65536)] * m, band, True), band
    assert bl.slices_for(LOCAL, 1024, off[:132], short[:132], traceback=True) == [130, 1]
    assert bl.slices_for(GLOBAL, 1024, off[:132], short[:132], traceback=True) == [130, 1]
    # a mixed batch on both sides of 16384, against the arithmetic recomputed
    rng = np.random.default_rng(3)
    shapes = [(65536, 65536) if k % 5 == 0 else (int(rng.integers(0, 40000)), int(rng.integers(0, 40000))) for k in range(900)]
    off1 = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.uint64)
    off2 = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.uint64)
    for band in WIDTHS:
        for kind in (LOCAL, GLOBAL):
            want = slices_by_hand(kind, shapes, band, True)
            assert bl.slices_for(kind, band, off1, off2, traceback=True) == want and len(want) >= (2 if band >= 512 else 1)


def test_move_offsets_is_the_wide_long_layout_without_that_library(bl, swmi_mod):
    rng = np.random.default_rng(4)
    len1 = np.concatenate([[0, 16384, 16385, 65536, 1, 65536], rng.integers(0, 65537, 60)])
    len2 = np.concatenate([[0, 16385, 16384, 65536, 65536, 0], rng.integers(0, 65537, 60)])
    off1, off2 = np.concatenate([[0], np.cumsum(len1)]).astype(np.uint64), np.concatenate([[0], np.cumsum(len2)]).astype(np.uint64)
    got = bl.move_offsets(off1, off2)
    assert got.dtype == np.uint64 and np.array_equal(got, swmi_mod.wide_long.move_offsets(off1, off2))
    assert np.array_equal(np.diff(got.astype(np.int64)), [move_words(int(x), int(y)) for x, y in zip(len1, len2)])
    short = np.minimum(len1, 16384), np.minimum(len2, 16384)
    s1, s2 = np.concatenate([[0], np.cumsum(short[0])]).astype(np.uint64), np.concatenate([[0], np.cumsum(short[1])]).astype(np.uint64)
    assert np.array_equal(bl.move_offsets(s1, s2), swmi_mod.banded_width.move_offsets(s1, s2))         # one layout up to 16384
    with pytest.raises(swmi_mod.SwmiError, match="a length above 65536"):
        bl.move_offsets([0, 65537], [0, 1])
    with pytest.raises(swmi_mod.SwmiError, match="decrease"):
        bl.move_offsets([0, 5, 4], [0, 1, 2])


def resources(tmp_path, source):
    """{(K, global, open >= extend, traceback): the compiler's remarks} of one kernel file with the Makefile's flags"""
    run = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall",
                          "-Wno-unused-function", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                          str(tmp_path / (source + ".o")), os.path.join(PKG, "csrc", source)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    assert run.returncode == 0, run.stdout[-3000:]
    kernels, name = {}, None
    for line in run.stdout.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            v = re.search(r"banded_(?:width|long)_kernelILi(\d)ELb([01])ELb([01])ELb([01])E", m.group(1))
            assert v, m.group(1)
            name = tuple(int(x) for x in v.groups())
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels


def test_kernel_resources_no_scratch_no_spill_and_the_width_kernels_waves(tmp_path):
    """The compiler's own remarks for csrc/banded_long_kernels.hip and, on the same tree, csrc/banded_width_kernels.hip: 32
    kernels each, none of the long ones with scratch or a spilled register, 16 KiB of LDS with a traceback and none without,
    and the waves per SIMD of every long kernel not below the width kernel's of the same (K, kind, gap order, traceback)."""
    long_, width = resources(tmp_path, "banded_long_kernels.hip"), resources(tmp_path, "banded_width_kernels.hip")
    variants = {(K, g, o, t) for K in (1, 2, 4, 8) for g in (0, 1) for o in (0, 1) for t in (0, 1)}
    assert set(long_) == set(width) == variants
    for v in sorted(variants):
        r, w = long_[v], width[v]
        print(v, "long", r["VGPRs"], r["TotalSGPRs"], r["Occupancy"], "width", w["VGPRs"], w["TotalSGPRs"], w["Occupancy"])
        assert r["ScratchSize"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (v, r)
        assert r["LDS Size"] == (16384 if v[3] else 0), (v, r)
        assert r["Occupancy"] >= w["Occupancy"] >= 3, (v, r, w)


def test_the_compat_header_compiles_and_links_against_this_library_and_libswmi_alone(tmp_path):
    assert shutil.which("g++") is not None
    exe = str(tmp_path / "compat_banded_long")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(NATIVE, "compat_banded_long.cpp"),
                            "-o", exe, "-L", LIB_DIR, "-lswmi_banded_long", "-lswmi", "-lpthread", "-Wl,-rpath," + LIB_DIR],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    dyn = subprocess.run(["readelf", "-d", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = [x for x in re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn) if "swmi" in x]
    assert sorted(needed) == ["libswmi.so", "libswmi_banded_long.so"]


def test_the_compat_header_runs_on_the_fake_gpu(tmp_path):
    """include/swmi_banded_long_compat.hpp's two overloads over the real host source on the fake GPU, as a stand-alone g++ ASan +
    UBSan program (tests/native/compat_banded_long_fake.cpp): pieces, results and paths at caller positions across them, lengths on
    both sides of 16384 and of 65536, empty sides, no diagonals, an empty batch, and the refusals as exceptions."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path / "compat_banded_long_fake")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-DSWMI_BANDED_LONG_LIBRARY", "-o", exe, os.path.join(NATIVE, "compat_banded_long_fake.cpp"),
                                          os.path.join(NATIVE, "fake_hip.cpp"), os.path.join(PKG, "csrc", "banded_ragged_api.cpp"), "-ldl",
                                          "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "banded long compat fake ok\n" in r.stdout
    assert r.stdout.count(": ok") == 5, r.stdout


def test_the_module_has_the_width_modules_functions_and_its_own_layout(swmi_mod):
    bl, bw = swmi_mod.banded_long, swmi_mod.banded_width
    assert inspect.ismodule(bl) and bl.WIDTHS == WIDTHS and bl.MAX_LEN == 65536 and bw.MAX_LEN == 16384
    assert (bl.LOCAL, bl.GLOBAL, bl.SLOT_BYTES, bl.END_ANYWHERE, bl.NO_ALIGNMENT) == (0, 1, 48, 16, -2**31)
    for name in ("local", "global_", "local_device", "global_device", "time_device", "slices_for", "move_offsets", "paths",
                 "release_workspaces", "version", "last_error", "load"):
        f = getattr(bl, name)
        assert inspect.isfunction(f) and f.__module__ == "swmi.banded_long" and f.__doc__, name
        assert inspect.signature(f) == inspect.signature(getattr(bw, name)), name
    assert bl.LIB_PATH == os.environ.get("SWMI_BANDED_LONG_LIB", bl.LIB_PATH)
    assert "SWMI_BANDED_LONG_LIB" in os.environ or bl.LIB_PATH.endswith("/lib/libswmi_banded_long.so")
    assert bl.expand_moves is swmi_mod.local_long.expand_moves and bl.SwmiError is swmi_mod.SwmiError
    # the binding body is given the layout function; it imports none
    from swmi import _banded_ragged_binding as body
    assert not hasattr(body, "local_full_ragged_move_offsets")
    assert bl._binding.move_offsets is bl.move_offsets
    assert bw._binding.move_offsets is swmi_mod.local_full_ragged_move_offsets is swmi_mod.banded_ragged._binding.move_offsets
    assert not hasattr(swmi_mod, "banded_long_local")            # the package's top-level functions stay the pinned set
