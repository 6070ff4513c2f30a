"""libswmi_banded_width.so (include/swmi_banded_width.h) without a device: the restatements' identities
at a width (a band that holds the table equals the full-table affine restatements; local scores never fall as the band doubles;
the drift family binds at 128 and 256 and is free at 512 and 1024), its nine exports, every refusal with the band first,
slices_for at every width, the 32 kernels' resources from the compiler's remarks, the compat header (over the host source on the
fake GPU as a stand-alone ASan + UBSan program; the host source's own driver runs from tests/test_banded_ragged_host_fake.py),
and the module's signatures."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from banded_width_support import (ALL_MASKS, EO_BUDGET, GLOBAL, LOCAL, MAX_SLICE, TB_BUDGET, WIDTHS, Batch, WidthOracle, assert_same,
                                  code_bytes, differs, drift_batch, move_words, per_alignment, related_batch, slices_by_hand, unbounded_for)
from conftest import PKG, ROOT, match_matrix

ENTRIES = ["swmi_banded_width_last_error", "swmi_banded_width_version", "swmi_banded_width_release_workspaces", "swmi_banded_width_local",
           "swmi_banded_width_global", "swmi_banded_width_local_device", "swmi_banded_width_global_device", "swmi_banded_width_slices_for",
           "swmi_banded_width_time_device"]
LIB = os.path.join(PKG, "lib", "libswmi_banded_width.so")
NATIVE = os.path.join(ROOT, "tests", "native")
SM = match_matrix(2, -3)


@pytest.fixture(scope="module")
def bw(swmi_mod):
    swmi_mod.banded_width.load()
    return swmi_mod.banded_width


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return WidthOracle(tmp_path_factory.mktemp("banded_width_oracle"))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    """the two full-table affine restatements, single-alignment functions"""
    so = os.path.join(str(tmp_path_factory.mktemp("full_affine_oracle")), "libfull_affine_oracle.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(NATIVE, "local_full_affine_oracle.c"),
                           os.path.join(NATIVE, "global_full_affine_oracle.c")])
    lib = ctypes.CDLL(so)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.local_full_affine_oracle.argtypes = [vp, sz, vp, sz, vp, ci, ci, vp, vp, vp, vp]
    lib.global_full_affine_oracle.argtypes = [vp, sz, vp, sz, vp, ci, ci, ctypes.c_uint, vp, vp, vp, vp]

    def align(kind, batch, sm, go, ge, mask=0):
        m = np.ascontiguousarray(sm, np.int8)
        scores, ends = np.zeros(batch.n, np.int32), np.zeros((batch.n, 4), np.int32)
        moves, steps = np.zeros(int(batch.move_offsets[-1]) + 1, np.uint64), np.zeros(batch.n, np.uint32)
        for k in range(batch.n):
            a, b = batch.seq1s[k], batch.seq2s[k]
            head = (a.ctypes.data, len(a), b.ctypes.data, len(b), m.ctypes.data, go, ge)
            tail = (scores[k:].ctypes.data, ends[k:].ctypes.data, moves[int(batch.move_offsets[k]):].ctypes.data, steps[k:].ctypes.data)
            rc = lib.global_full_affine_oracle(*head, mask, *tail) if kind == GLOBAL else lib.local_full_affine_oracle(*head, *tail)
            assert rc == 0
        return scores, ends, moves[:-1], steps
    return align


def test_a_band_that_holds_the_table_is_the_full_table_restatement(orc, full):
    """band / 2 > max(len1, len2) + |d0|: every cell of the table is in the band, and the banded restatements equal the
    full-table affine ones field for field and move for move (masks 0 .. 15: the full one has no END_ANYWHERE)."""
    rng = np.random.default_rng(1)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 200, 12), rng.integers(1, 200, 12))]
    diags = [int(x) for x in rng.integers(-50, 51, 12)]
    batch = related_batch(rng, shapes, diags)
    for band in (512, 1024):                                                     # 256 > 199 + 50
        for go, ge in ((5, 1), (1, 3)):
            assert_same(orc.align(LOCAL, batch, band, SM, go, ge), full(LOCAL, batch, SM, go, ge), batch, ("local", band, go, ge))
            for mask in range(16):
                assert_same(orc.align(GLOBAL, batch, band, SM, go, ge, mask), full(GLOBAL, batch, SM, go, ge, mask), batch, (band, mask, go, ge))


def test_drift_binds_at_128_and_256_and_is_free_at_512_and_1024(orc):
    """The issue's family: 20 pairs of 700 bases, 8 % substitutions, four runs of 40 bases inserted or deleted, diagonals 0,
    matrix 2 / -3, gaps (4, 1).  The path ends 160 diagonals from where it starts: outside 128 and 256, inside 512 and 1024.
    Local scores never fall as the band doubles."""
    rng = np.random.default_rng(2)
    batch = drift_batch(rng, 20, 700, 4, 40)
    unbounded = unbounded_for(batch)
    free_l, free_g = orc.align(LOCAL, batch, unbounded, SM, 4, 1), orc.align(GLOBAL, batch, unbounded, SM, 4, 1, 0)
    last = None
    for band in WIDTHS:
        loc, glo = orc.align(LOCAL, batch, band, SM, 4, 1), orc.align(GLOBAL, batch, band, SM, 4, 1, 0)
        if band <= 256:
            assert int(differs(loc, free_l).sum()) >= 15, band
            assert differs(glo, free_g).all(), band
        else:
            assert_same(loc, free_l, batch, ("local", band))
            assert_same(glo, free_g, batch, ("global", band))
        if last is not None:
            assert (loc[0] >= last).all(), band
        last = loc[0]
    assert (free_l[0] >= last).all()


def test_header_declares_and_library_exports_exactly_the_nine_entries(bw, swmi_mod):
    with open(os.path.join(ROOT, "include", "swmi_banded_width.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 9
    assert "expand_moves(" not in header.replace("swmi_local_full_expand_moves", "")          # one expander: libswmi.so's
    assert "move_offsets(" not in header.replace("swmi_local_full_ragged_move_offsets", "")   # ... and one layout function
    for text in ("KNOWN LIMITS: one band width per call", "4 letters", "lengths up to 16384", "SWMI_BANDED_WIDTH_MIN 128", "SWMI_BANDED_WIDTH_MAX 1024"):
        assert text in header, text
    for m in re.finditer(r"swmi_banded_width_(?:local|global)(?:_device)?\(([^;]*?)\);", header, re.S):
        assert re.search(r"diagonals,\s+int band,\s+const int8_t score_matrix\[16\]", m.group(1)), m.group(0)     # band directly before the matrix
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}     # it calls nothing of libswmi.so
    dyn = subprocess.run(["readelf", "-d", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", dyn)
    assert "libswmi.so" in needed and "$ORIGIN" in dyn
    assert bw.version() == swmi_mod.load().swmi_version()


def test_every_refusal_with_the_band_first_and_no_device(bw, swmi_mod):
    """A bad band is reported before every other broken rule; then the ragged header's order: the mask, the matrix, the gaps,
    the moves / steps pair, n = 0, the buffers, the offsets, the alignment of device pointers.  None touches a device."""
    lib = bw.load()
    buf = np.zeros(4096, np.int64)
    sm = np.zeros(16, np.int8)
    good = np.array([0, 8, 16], np.uint64)
    decreasing = np.array([0, 8, 7], np.uint64)
    too_long = np.array([0, 8, 8 + 16385], np.uint64)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT
    ms = ctypes.c_float()

    def args(band=256, o1=good, o2=good, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return (s1, p(o1), s2, p(o2), n, dg, band, m, go, ge), (sc, en, mv, st)

    def calls(fe=0, **kw):
        head, tail = args(**kw)
        yield "global", lambda: lib.swmi_banded_width_global(*head, fe, *tail)
        yield "global_device", lambda: lib.swmi_banded_width_global_device(*head, fe, *tail, None)
        yield "time global", lambda: lib.swmi_banded_width_time_device(1, *head, fe, *tail, None, 1, ctypes.byref(ms))
        if fe <= 19:
            yield "local", lambda: lib.swmi_banded_width_local(*head, *tail)
            yield "local_device", lambda: lib.swmi_banded_width_local_device(*head, *tail, None)
            yield "time local", lambda: lib.swmi_banded_width_time_device(0, *head, fe, *tail, None, 1, ctypes.byref(ms))

    def refused(code, text, **kw):
        for name, call in calls(**kw):
            assert call() == code, (name, kw, bw.last_error())
            assert text in bw.last_error(), (name, bw.last_error())

    # 0. the band before everything else, the mask included
    for bad in (0, 1, 64, 127, 129, 192, 384, 640, 2048, -128, 2**31 - 1, -2**31):
        refused(INV, "band %d is not one of 128, 256, 512, 1024" % bad, band=bad, fe=20, m=None, go=200, mv=None, s1=None, o1=decreasing)
        refused(INV, "band", band=bad, n=0)
    for band in WIDTHS:
        # 1. the mask (global kind)
        for bad in (20, 32, 0xFFFFFFFF):
            refused(INV, "free_ends", band=band, fe=bad, m=None, go=200, mv=None, s1=None, o1=decreasing)
        # 2. the matrix before the gaps, 3. the gaps before the pair, 4. the pair before n = 0 and the buffers
        refused(INV, "score_matrix is NULL", band=band, m=None, go=200, mv=None, s1=None, o1=decreasing)
        refused(DOM, "outside [0,127]", band=band, go=128, mv=None, s1=None, o1=decreasing)
        refused(INV, "moves and steps", band=band, mv=None, n=0, s1=None)
        # 5. n = 0 is SWMI_OK whatever the buffers and offsets are and needs no device (the timer alone wants n > 0)
        for name, call in calls(band=band, n=0, s1=None, s2=None, sc=None, en=None, o1=None, o2=None):
            assert call() == (INV if name.startswith("time") else 0), name
        # 6. the buffers before the offsets, 7. the offsets before the alignment of device pointers
        refused(INV, "NULL buffer", band=band, o1=decreasing, s2=None)
        odd = p(buf) + 8
        refused(INV, "offsets is NULL", band=band, o1=None, s1=odd)
        refused(INV, "offsets decrease at alignment 1", band=band, o2=decreasing, s1=odd)
        refused(INV, "a length above 16384", band=band, o1=too_long, s1=odd)
        # 8. 16-byte alignment of every device pointer
        for which in ("s1", "sc", "mv"):
            head, tail = args(band=band, **{which: odd})
            assert lib.swmi_banded_width_local_device(*head, *tail, None) == ALN, which
            assert lib.swmi_banded_width_global_device(*head, 19, *tail, None) == ALN, which
    head, tail = args()
    assert lib.swmi_banded_width_time_device(2, *head, 0, *tail, None, 1, ctypes.byref(ms)) == INV and "kind 2" in bw.last_error()
    assert lib.swmi_banded_width_time_device(0, *head, 0, *tail, None, 0, ctypes.byref(ms)) == INV
    # the module
    one = [np.zeros(3, np.uint8)]
    with pytest.raises(swmi_mod.SwmiError) as err:
        bw.local(one, one, 100, sm, 1, 1)
    assert err.value.code == INV and "band 100" in str(err.value)
    with pytest.raises(swmi_mod.SwmiError) as err:
        bw.global_(one, one, 512, sm, 1, 1, free_ends=-1)
    assert err.value.code == INV and "free_ends" in str(err.value)
    with pytest.raises(ValueError):
        bw.local(one, one, 512, sm, 1, 1, diagonals=[0, 0])
    assert bw.local([], [], 1024, sm, 1, 1)[0].shape == (0,)            # n = 0 needs no device


def test_slices_for_is_the_headers_arithmetic_at_every_width(bw):
    # by hand: one alignment of (16384, 700) with a traceback at band 1024, global kind:
    #   16384 + 700 + 48 + 20 = 17152; codes 8 * 256 * ceil(16448 / 4) = 8 * 256 * 4112 = 8421376; moves 8 * words; steps 4
    assert code_bytes(GLOBAL, 16384, 1024) == 8421376 and code_bytes(LOCAL, 16384, 128) == 256 * 4112 and code_bytes(LOCAL, 1, 256) == 2 * 256 * 16
    assert per_alignment(GLOBAL, 16384, 700, 1024, True) == 17152 + 8421376 + 8 * move_words(16384, 700) + 4
    assert per_alignment(GLOBAL, 16384, 700, 1024, False) == 17152
    # the count cap on a tiny shape, ends-only: the width does not enter
    n = 2 * MAX_SLICE + 7
    off1, off2 = 3 * np.arange(n + 1, dtype=np.uint64), 2 * np.arange(n + 1, dtype=np.uint64)
    for band in WIDTHS:
        assert bw.slices_for(LOCAL, band, off1, off2, traceback=False) == bw.slices_for(GLOBAL, band, off1, off2, traceback=False) == [MAX_SLICE, MAX_SLICE, 7]
    # the ends-only budget: 256 MiB of (16384, 16384) alignments, 32836 bytes each, at every width
    m = 9000
    long_ = 16384 * np.arange(m + 1, dtype=np.uint64)
    fit = EO_BUDGET // 32836
    for band in WIDTHS:
        assert bw.slices_for(LOCAL, band, long_, long_, traceback=False) == [fit, m - fit] == slices_by_hand(LOCAL, [(16384, 16384)] * m, band, False)
    # the traceback budget binds by the width's codes: every fourth alignment is (16384, 700), the rest small
    rng = np.random.default_rng(1)
    shapes = [(16384, 700) if k % 4 == 0 else (int(rng.integers(0, 900)), int(rng.integers(0, 900))) for k in range(20000)]
    off1 = np.concatenate([[0], np.cumsum([s[0] for s in shapes])]).astype(np.uint64)
    off2 = np.concatenate([[0], np.cumsum([s[1] for s in shapes])]).astype(np.uint64)
    counts = {}
    for band in WIDTHS:
        for kind in (LOCAL, GLOBAL):
            want = slices_by_hand(kind, shapes, band, True)
            assert bw.slices_for(kind, band, off1, off2, traceback=True) == want
            assert len(want) >= 2 and sum(want) == len(shapes)
            used = sum(per_alignment(kind, *s, band, True) for s in shapes[:want[0]])
            assert used <= TB_BUDGET < used + per_alignment(kind, *shapes[want[0]], band, True)          # the longest run that fits
            assert bw.slices_for(kind, band, off1, off2, traceback=False) == [len(shapes)]
            counts[band, kind] = len(want)
    assert counts[1024, LOCAL] > counts[512, LOCAL] > counts[256, LOCAL] > counts[128, LOCAL]
    # one alignment always fits; n = 0, an unknown kind, an illegal band and refused offsets give 0
    one = np.array([0, 16384], np.uint64)
    assert bw.slices_for(LOCAL, 1024, one, one) == [1]
    assert bw.slices_for(LOCAL, 1024, np.array([0], np.uint64), np.array([0], np.uint64)) == []
    assert bw.slices_for(2, 128, one, one) == [] and "kind 2" in bw.last_error()
    assert bw.slices_for(LOCAL, 192, one, one) == [] and "band 192" in bw.last_error()
    assert bw.slices_for(GLOBAL, 256, np.array([0, 8, 7], np.uint64), np.array([0, 8, 9], np.uint64)) == [] and "decrease" in bw.last_error()


def test_kernel_resources_no_scratch_no_spill_at_any_width(tmp_path):
    """The compiler's own remarks for csrc/banded_width_kernels.hip with the Makefile's flags: 32 kernels -- K = 1, 2, 4, 8, two
    kinds, open >= extend or not, traceback or not -- none with scratch or a spilled register, 16 KiB of LDS with a traceback at
    every width (two workgroups a CU need at most 80 KiB each) and none without."""
    src = os.path.join(PKG, "csrc", "banded_width_kernels.hip")
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
    assert len(kernels) == 32, sorted(kernels)
    variants = set()
    for k, r in kernels.items():
        m = re.search(r"banded_width_kernelILi(\d)ELb([01])ELb([01])ELb([01])E", k)
        assert m, k
        variants.add(m.groups())
        assert r["ScratchSize"] == 0 and r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == (16384 if m.group(4) == "1" else 0), (k, r)
        assert r["Occupancy"] >= 3, (k, r)
    assert variants == {(str(K), g, o, t) for K in (1, 2, 4, 8) for g in "01" for o in "01" for t in "01"}


def test_the_compat_header_compiles_and_links(tmp_path):
    """include/swmi_banded_width_compat.hpp's two overloads compile and link against libswmi_banded_width.so and libswmi.so
    alone (the GPU tests run the program)."""
    assert shutil.which("g++") is not None
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(NATIVE, "compat_banded_width.cpp"),
                            "-o", str(tmp_path / "compat_banded_width"), "-L", lib, "-lswmi_banded_width", "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout


def test_the_compat_header_runs_on_the_fake_gpu(tmp_path):
    """include/swmi_banded_width_compat.hpp's two overloads run over the real host source on the fake GPU, as a stand-alone
    g++ ASan + UBSan program (tests/native/compat_banded_width_fake.cpp, with plain stand-ins for the launcher and for the three
    libswmi.so functions the header calls): several pieces, results and paths at caller positions across them, empty sides, no
    diagonals, an empty batch, and the refusals as exceptions with the library's text, the band first."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path / "compat_banded_width_fake")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-DSWMI_BANDED_WIDTH_LIBRARY", "-o", exe, os.path.join(NATIVE, "compat_banded_width_fake.cpp"),
                                          os.path.join(NATIVE, "fake_hip.cpp"), os.path.join(PKG, "csrc", "banded_ragged_api.cpp"), "-ldl",
                                          "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "banded width compat fake ok\n" in r.stdout
    assert r.stdout.count(": ok") == 6, r.stdout


def test_the_module_has_the_ragged_modules_functions_with_band_before_the_matrix(swmi_mod):
    bw, br = swmi_mod.banded_width, swmi_mod.banded_ragged
    assert inspect.ismodule(bw) and bw.WIDTHS == WIDTHS
    for name in ("local", "global_", "local_device", "global_device", "time_device", "slices_for"):
        mine, theirs = list(inspect.signature(getattr(bw, name)).parameters), list(inspect.signature(getattr(br, name)).parameters)
        at = mine.index("band")
        assert mine[:at] + mine[at + 1:] == theirs, name
        assert mine[at + 1] == ("seq1_offsets" if name == "slices_for" else "score_matrix"), name
    assert list(inspect.signature(bw.slices_for).parameters)[:2] == ["kind", "band"]
    for name in ("move_offsets", "paths", "release_workspaces", "version", "last_error", "load"):
        assert inspect.signature(getattr(bw, name)) == inspect.signature(getattr(br, name)), name
    assert not hasattr(swmi_mod, "banded_width_local")           # the package's top-level functions stay the pinned set
