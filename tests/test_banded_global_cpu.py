"""The banded global / fit / overlap / extension aligner's host-only parts, no device needed (libswmi_banded_global.so,
include/swmi_banded_global.h, swmi.banded_global): the header and the library's symbols; every refusal with code and text, in
the stated order, in a process with no GPU bound; the slice arithmetic on hand-computed sizes; the compiler's resource remarks of
the four kernels; and the C restatement tests/native/banded_global_oracle.c tied to an independent numpy formulation and, by
the header's four identities, to the restatements of swmi_global_full_affine, swmi_global_full and
swmi_semiglobal_full_affine; shown to bind where the full path leaves the band, to tell a band that is off by one on either
side, and to say NO_ALIGNMENT exactly where the geometry leaves no start or no end.  Every comparison is exact integer equality."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from banded_global_support import (ALL_MASKS, ANYWHERE, BEGIN1, BEGIN2, END1, END2, IDENTITY_MASKS, INT32_MAX, INT32_MIN, NO_ALIGNMENT,
                                   RELATED_PARAMS, TB_BUDGET, BandedGlobalOracle, assert_same, band_leaver, code_bytes, feasible_by_hand,
                                   in_band, move_words, moves_of, numpy_banded_global, path_from, per_alignment, related_pairs)
from conftest import PKG, ROOT, match_matrix
from global_full_affine_support import GlobalFullAffineOracle
from global_full_support import GlobalFullOracle
from sgfull_affine_support import SgAffineOracle

ENTRIES = ["swmi_banded_global", "swmi_banded_global_device", "swmi_banded_global_slices_for", "swmi_banded_global_time_device",
           "swmi_banded_global_release_workspaces", "swmi_banded_global_last_error", "swmi_banded_global_version"]
MAX = 16384
# the issue's related family: (len1, len2) per diagonal, every one with -64 <= len2 - len1 - d0 <= 63
RELATED_SHAPES = {0: [(300, 300), (300, 330), (257, 300)], 40: [(300, 340), (300, 330), (257, 300)], -37: [(300, 263)]}


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return BandedGlobalOracle(tmp_path_factory.mktemp("banded_global_oracle"))


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    return GlobalFullAffineOracle(tmp_path_factory.mktemp("banded_global_full_affine"))


@pytest.fixture(scope="module")
def bg(swmi_mod):
    swmi_mod.banded_global.load()
    return swmi_mod.banded_global


def one(r, k):
    return tuple(y[k:k + 1] for y in r)


def test_header_declares_and_library_exports_exactly_the_seven_entries(bg):
    with open(os.path.join(ROOT, "include", "swmi_banded_global.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 7
    assert "expand_moves(" not in header.replace("swmi_local_full_expand_moves", "")          # one expander: libswmi.so's
    for text in ("SWMI_BANDED_END_ANYWHERE 16u", "SWMI_BANDED_ENDS_EXTEND 16u", "SWMI_BANDED_NO_ALIGNMENT INT32_MIN"):
        assert text in header, text
    lib = os.path.join(PKG, "lib", "libswmi_banded_global.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}     # it calls nothing of libswmi.so
    needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libswmi.so" in needed and "libswmi_wide" not in needed and "libswmi_banded.so" not in needed and "$ORIGIN" in needed
    assert bg.version() == 300
    # the local library keeps its seven
    local = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libswmi_banded.so")], stdout=subprocess.PIPE, text=True,
                           check=True).stdout
    assert len([line for line in local.splitlines() if " T " in line]) == 7 and "global" not in local


def test_every_refusal_works_with_no_device_in_the_stated_order(bg, swmi_mod):
    lib = bg.load()
    buf = np.zeros(4096, np.int64)
    sm = np.zeros(16, np.int8)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT
    ms = ctypes.c_float()

    def host(len1=8, len2=8, n=2, go=1, ge=1, fe=0, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_global(s1, len1, s2, len2, n, dg, m, go, ge, fe, sc, en, mv, st)

    def dev(len1=8, len2=8, n=2, go=1, ge=1, fe=0, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_global_device(s1, len1, s2, len2, n, dg, m, go, ge, fe, sc, en, mv, st, None)

    def timer(len1=8, len2=8, n=2, go=1, ge=1, fe=0, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_global_time_device(s1, len1, s2, len2, n, dg, m, go, ge, fe, sc, en, mv, st, None, 1, ctypes.byref(ms))

    for f in (host, dev, timer):
        for len1, len2 in ((0, 8), (8, 0), (MAX + 1, 8), (8, MAX + 1)):
            assert f(len1=len1, len2=len2) == INV and "len1 %d / len2 %d outside [1,16384]" % (len1, len2) in bg.last_error(), (len1, len2)
        for name in ("s1", "s2", "sc", "en"):
            assert f(**{name: None}) == INV and "NULL buffer with n = 2" in bg.last_error(), name
        assert f(m=None) == INV and "score_matrix is NULL" in bg.last_error()
        assert f(mv=None) == INV and "moves and steps" in bg.last_error()
        assert f(st=None) == INV and "moves and steps" in bg.last_error()
        for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
            assert f(go=go, ge=ge) == DOM and "gap_open %d / gap_extend %d outside [0,127]" % (go, ge) in bg.last_error()
        # the mask: 0 .. 19 are legal, END_ANYWHERE with END1 or END2 and everything above are not
        for fe in (20, 24, 31, 32, 2**32 - 1):
            assert f(fe=fe) == INV and "free_ends %d" % fe in bg.last_error(), fe
        # the order: matrix, gaps, mask, moves / steps pair, (n = 0,) buffers, lengths
        assert f(m=None, go=-1) == INV and "score_matrix" in bg.last_error()
        assert f(go=-1, fe=20) == DOM
        assert f(fe=20, mv=None) == INV and "free_ends" in bg.last_error()
        assert f(mv=None, sc=None) == INV and "moves and steps" in bg.last_error()
        assert f(sc=None, len1=0) == INV and "NULL buffer" in bg.last_error()
    for f in (host, dev):
        # n = 0 is a no-op behind the matrix, the gaps, the mask and the moves / steps pair and in front of the buffers and lengths
        assert f(n=0, s1=None, len1=0) == 0
        assert f(n=0, go=200) == DOM and f(n=0, fe=20) == INV and f(n=0, mv=None) == INV and f(n=0, m=None) == INV
    assert timer(n=0) == INV and "n is 0" in bg.last_error()
    for name in ("s1", "s2", "dg", "sc", "en", "mv", "st"):
        assert dev(**{name: p(buf) + 8}) == ALN and "16-byte aligned" in bg.last_error(), name
    assert dev(s1=p(buf) + 8, len1=0) == INV                   # the lengths before the alignment of the pointers
    # the Python layer
    a = np.zeros((2, 8), np.uint8)
    with pytest.raises(swmi_mod.SwmiError) as e:
        bg.align(a, a, sm, 1, 1, free_ends=20)
    assert e.value.code == INV and "free_ends 20" in str(e.value)
    with pytest.raises(swmi_mod.SwmiError) as e:
        bg.align(a, a, sm, 1, 1, free_ends=-1)
    assert e.value.code == INV
    with pytest.raises(swmi_mod.SwmiError) as e:
        bg.align(a, a, sm, 2**32 + 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        bg.align(np.zeros((1, MAX + 1), np.uint8), a[:1], sm, 1, 1)
    assert e.value.code == INV and "16385" in str(e.value)
    with pytest.raises(ValueError):
        bg.align(a, a, sm, 1, 1, diagonals=[0])
    r = bg.align(np.zeros((0, 8), np.uint8), np.zeros((0, 9), np.uint8), sm, 1, 1, free_ends=19)      # an empty batch needs no device
    assert len(r[0]) == 0 and r[1].shape == (0, 4) and r[2].shape == (0, move_words(8, 9))


def test_slices_for_on_hand_computed_sizes(bg):
    lib = bg.load()
    for tb in (0, 1):
        for len1, len2 in ((0, 8), (8, 0), (MAX + 1, 8), (8, MAX + 1)):
            assert lib.swmi_banded_global_slices_for(10, len1, len2, tb, None, 0) == 0 and "outside [1,16384]" in bg.last_error()
        assert lib.swmi_banded_global_slices_for(0, 8, 8, tb, None, 0) == 0
        sizes = (ctypes.c_size_t * 3)(99, 99, 99)
        assert lib.swmi_banded_global_slices_for(10, 8, 8, tb, sizes, 3) == 1 and list(sizes) == [10, 99, 99]
    assert bg.slices_for((1 << 20) + 5, 3, 2, traceback=False) == [1 << 20, 5]
    # ends-only: as the local library's, 32768 + 4 + 20 bytes each at the largest shape within 256 MiB
    assert per_alignment(MAX, MAX, False) == 32792 and (256 << 20) // 32792 == 8186
    assert bg.slices_for(2 * 8186 + 7, MAX, MAX, traceback=False) == [8186, 8186, 7]
    # with a traceback: the codes of len1 + 64 iterations in whole trips.  16384: 256 x 4112 as the local kernel's (16447 and
    # 16448 iterations both take 4112 trips); 1021: 1085 iterations are 272 trips where the local kernel's 1084 are 271
    assert TB_BUDGET == 4383801344
    assert code_bytes(MAX) == 256 * 4112 and code_bytes(1021) == 256 * 272 and code_bytes(1020) == 256 * 271 and code_bytes(1) == 256 * 17
    assert per_alignment(MAX, MAX, True) == 32792 + 1052672 + 8192 + 4 == 1093660 and TB_BUDGET // 1093660 == 4008
    assert bg.slices_for(10000, MAX, MAX) == [4008, 4008, 1984]
    assert move_words(1021, 1024) == 64
    assert per_alignment(1021, 1024, True) == 2045 + 24 + 69632 + 512 + 4 == 72217
    per_slice = TB_BUDGET // 72217
    assert per_slice == 60703 and 60703 * 72217 == 4383788551 <= TB_BUDGET < 4383788551 + 72217
    assert bg.slices_for(65536, 1021, 1024) == [per_slice, 65536 - per_slice]


def test_module_is_a_submodule_with_docstrings(swmi_mod):
    bg = swmi_mod.banded_global
    assert isinstance(bg, types.ModuleType) and bg.__name__ == "swmi.banded_global" and bg.__doc__
    for name in ["load", "align", "align_device", "time_device", "slices_for", "move_words", "paths", "release_workspaces", "last_error",
                 "version"]:
        fn = getattr(bg, name)
        assert inspect.isfunction(fn) and fn.__module__ == "swmi.banded_global" and fn.__doc__, name
    sig = inspect.signature(bg.align).parameters
    assert list(sig) == ["seq1s", "seq2s", "score_matrix", "gap_open", "gap_extend", "free_ends", "diagonals", "traceback"]
    assert sig["free_ends"].default == 0 and sig["diagonals"].default is None and sig["traceback"].default is True
    assert (bg.MAX_LEN, bg.WIDTH, bg.LO, bg.HI) == (MAX, 128, -64, 63)
    assert (bg.END_ANYWHERE, bg.ENDS_EXTEND, bg.NO_ALIGNMENT) == (16, 16, -2**31)
    assert not hasattr(swmi_mod, "align") and not hasattr(swmi_mod, "END_ANYWHERE")
    assert bg.move_words(300, 1025) == move_words(300, 1025)


def test_no_kernel_spills_or_uses_scratch(tmp_path):
    """The compiler's resource remarks of the four kernels (open >= extend x traceback), with csrc/Makefile's flags: no scratch,
    no VGPR or SGPR spill, 16 KiB of LDS in the traceback kernels (the walk windows of 4 wavefronts) and none in the ends-only
    ones, at most 128 VGPRs."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.s"), os.path.join(csrc, "banded_global_kernels.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=csrc)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stdout)[1:]
    seen = {}
    for b in blocks:
        m = re.match(r"_ZN4swmi6banded\d+_GLOBAL__N_1\d+banded_global_kernelILb([01])ELb([01])EE", b.split()[0])
        if not m:
            continue
        field = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))  # noqa: E731
        seen[m.groups()] = (field("ScratchSize [bytes/lane]"), field("SGPRs Spill"), field("VGPRs Spill"), field("LDS Size [bytes/block]"),
                            field("VGPRs"))
    assert sorted(seen) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(seen)
    for (oge, tb), (scratch, sgpr_spill, vgpr_spill, lds, vgprs) in seen.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (oge, tb, scratch, sgpr_spill, vgpr_spill)
        assert lds == (16384 if tb == "1" else 0), (oge, tb, lds)
        assert vgprs <= 128, (oge, tb, vgprs)


def test_the_restatement_equals_an_independent_numpy_formulation_on_small_shapes(orc):
    rng = np.random.default_rng(1)
    cases = 0
    for len1, len2, d0 in ((9, 9, 0), (12, 7, 0), (7, 12, 3), (10, 10, -4), (8, 13, 6), (13, 8, -6)):
        for lo, hi in ((-3, 2), (-1, 1), (0, 0), (-64, 63)):
            a = rng.integers(0, 4, (3, len1), dtype=np.uint8)
            b = rng.integers(0, 4, (3, len2), dtype=np.uint8)
            b[0, :min(len1, len2)] = a[0, :min(len1, len2)]
            for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 1, 3), (match_matrix(1, -1), 0, 0)):
                for mask in ALL_MASKS:
                    got = orc.align(a, b, sm, go, ge, mask, [d0] * 3, lo=lo, hi=hi)
                    for k in range(3):
                        score, end, path, _ = numpy_banded_global(a[k], b[k], sm, go, ge, mask, d0, lo, hi)
                        cases += 1
                        what = (len1, len2, d0, lo, hi, go, ge, mask, k)
                        if score is None:
                            assert got[0][k] == NO_ALIGNMENT and not got[1][k].any() and got[3][k] == 0, what
                            continue
                        assert got[0][k] == score and tuple(got[1][k][:2]) == end, what
                        assert np.array_equal(path_from(got[2][k], got[3][k], *got[1][k][:2]), path), what
                        assert tuple(got[1][k][2:]) == tuple(path[0]), what
    assert cases == 6 * 4 * 3 * 20 * 3


def test_identity_3_a_table_inside_the_band_equals_the_full_restatement_under_every_mask(orc, full, tmp_path):
    rng = np.random.default_rng(2)
    linear = GlobalFullOracle(tmp_path)
    sg = SgAffineOracle(tmp_path)
    for len1, len2, d0 in ((63, 63, 0), (40, 63, 0), (63, 17, 0), (1, 1, 0), (30, 50, 20), (50, 30, -20)):
        a, b = related_pairs(rng, 8, len1, len2, 0)
        b[::2] = rng.integers(0, 4, (4, len2), dtype=np.uint8)
        for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 1, 3), (match_matrix(3, -2), 2, 2)):
            for mask in range(16):
                got = orc.align(a, b, sm, go, ge, mask, [d0] * 8)
                assert_same(got, full.align(a, b, sm, go, ge, mask), ("identity 3", len1, len2, d0, go, ge, mask))
                if go == ge:
                    assert_same(got, linear.align(a, b, sm, go, mask), ("identity 2", len1, len2, d0, go, mask))
            # identity 4: extension against the exact semi-global restatement (whose walk also ends at (0,0))
            got = orc.align(a, b, sm, go, ge, ANYWHERE, [d0] * 8)
            want = sg.align(a, b, sm, go, ge)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1][:, :2], want[1]) and not got[1][:, 2:].any()
            assert np.array_equal(got[3], want[3] - 1)
            for k in range(8):
                assert np.array_equal(moves_of(got[2][k], got[3][k]), moves_of(want[2][k], want[3][k] - 1))


def test_identities_1_and_2_where_the_full_path_stays_in_the_band(orc, full, tmp_path):
    """The related family: seq2 is seq1 with 8 % substitutions and 3 indel runs of 1 - 8 bases along diagonal d0.  At least 95 %
    of the cases qualify (the full restatement's path, start cell included, lies in the band); at d0 = -37, 300 x 330 puts
    (len1, len2) outside the band: only masks with END2 qualify there, and mask 0 yields NO_ALIGNMENT."""
    linear = GlobalFullOracle(tmp_path)
    rng = np.random.default_rng(3)
    cases = inside = 0
    for d0, shapes in RELATED_SHAPES.items():
        for len1, len2 in shapes:
            assert -64 <= len2 - len1 - d0 <= 63
            a, b = related_pairs(rng, 10, len1, len2, d0)
            for m, x, go, ge in RELATED_PARAMS:
                sm = match_matrix(m, x)
                for mask in IDENTITY_MASKS:
                    got = orc.align(a, b, sm, go, ge, mask, [d0] * 10)
                    want = full.align(a, b, sm, go, ge, mask)
                    lin = linear.align(a, b, sm, go, mask) if go == ge else None
                    assert (got[0] <= want[0]).all()
                    for k in range(10):
                        cases += 1
                        if not in_band(path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1]), d0):
                            continue
                        inside += 1
                        assert_same(one(got, k), one(want, k), ("identity 1", d0, len1, len2, m, x, go, ge, mask, k))
                        if lin is not None:
                            assert_same(one(got, k), one(lin, k), ("identity 2", d0, len1, len2, m, x, go, mask, k))
    assert cases == 7 * 10 * 4 * 6 and inside >= 0.95 * cases, (inside, cases)
    # 300 x 330 at d0 = -37: len2 - len1 - d0 = 67
    a, b = related_pairs(rng, 10, 300, 330, -37)
    sm = match_matrix(2, -3)
    for mask in IDENTITY_MASKS:
        got = orc.align(a, b, sm, 5, 1, mask, [-37] * 10)
        want = full.align(a, b, sm, 5, 1, mask)
        stays = [in_band(path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1]), -37) for k in range(10)]
        if mask & END2:
            assert all(stays), mask
            assert_same(got, want, ("identity 1", "300 x 330 at -37", mask))
        else:
            assert not any(stays), mask
        if mask == 0:
            assert (got[0] == NO_ALIGNMENT).all() and not got[1].any() and not got[3].any()


def test_identity_4_extension_against_the_exact_semi_global_restatement(orc, tmp_path):
    sg = SgAffineOracle(tmp_path)
    rng = np.random.default_rng(4)
    cases = inside = 0
    for len1, len2 in ((300, 300), (300, 330), (257, 300)):
        a, b = related_pairs(rng, 10, len1, len2, 0)
        b[:, len2 // 2:] = rng.integers(0, 4, (10, len2 - len2 // 2), dtype=np.uint8)       # the score peaks half way
        for m, x, go, ge in RELATED_PARAMS:
            sm = match_matrix(m, x)
            got = orc.align(a, b, sm, go, ge, ANYWHERE)
            want = sg.align(a, b, sm, go, ge)
            for k in range(10):
                cases += 1
                if not in_band(path_from(want[2][k], want[3][k] - 1, want[1][k, 0], want[1][k, 1])):
                    continue
                inside += 1
                assert got[0][k] == want[0][k] and tuple(got[1][k]) == tuple(want[1][k]) + (0, 0), (len1, len2, go, ge, k)
                assert got[3][k] >= want[3][k] - 1
                assert np.array_equal(moves_of(got[2][k], want[3][k] - 1), moves_of(want[2][k], want[3][k] - 1))
    assert cases == 120 and inside >= 0.95 * cases, (inside, cases)


def test_the_band_binds_where_the_full_path_leaves_it(orc, full):
    rng = np.random.default_rng(5)
    a, b = band_leaver(rng, 12)
    sm = match_matrix(2, -3)
    for mask in (0, 15):
        want = full.align(a, b, sm, 5, 1, mask)
        got = orc.align(a, b, sm, 5, 1, mask)
        for k in range(12):
            assert not in_band(path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1])), (mask, k)
        assert (got[0] < want[0]).all() and (got[0] != NO_ALIGNMENT).all(), mask
        for k in range(12):
            assert in_band(path_from(got[2][k], got[3][k], got[1][k, 0], got[1][k, 1])), (mask, k)


def test_a_band_off_by_one_on_either_side_gets_a_case_wrong(orc):
    """Pairs with one gap of exactly 63 inserted bases (the path touches diagonal +63) and of exactly 64 deleted bases
    (diagonal -64): the contract's band holds the path, a band one narrower on that side does not; with gaps of 64 and 65 the
    contract's band loses it and a band one wider on that side holds it."""
    rng = np.random.default_rng(6)
    sm = match_matrix(2, -3)
    core = rng.integers(0, 4, (6, 200), dtype=np.uint8)

    def with_insert(g):          # seq2 = seq1 with g bases inserted at 100 and the tail cut to keep the length: diagonals 0 .. g
        ins = rng.integers(0, 4, (6, g), dtype=np.uint8)
        return core, np.concatenate([core[:, :100], ins, core[:, 100:]], axis=1)

    def with_delete(g):
        return core, np.concatenate([core[:, :100], core[:, 100 + g:]], axis=1)

    wrong = {}
    for name, (a, b), d_end, bands in (("insert 63", with_insert(63), 63, [(-64, 62)]), ("insert 64", with_insert(64), 64, [(-64, 64)]),
                                       ("delete 64", with_delete(64), -64, [(-63, 63)]), ("delete 65", with_delete(65), -65, [(-65, 63)])):
        # mask 0: the end cell is (len1, len2), on diagonal d_end
        right = orc.align(a, b, sm, 2, 1, 0)
        fits = -64 <= d_end <= 63
        assert (right[0] != NO_ALIGNMENT).all() == fits, name
        for lo, hi in bands:
            other = orc.align(a, b, sm, 2, 1, 0, lo=lo, hi=hi)
            wrong[(name, lo, hi)] = int((other[0] != right[0]).sum())
            assert (other[0] != NO_ALIGNMENT).all() == (not fits), (name, lo, hi)
    assert all(wrong.values()), wrong


def test_the_origin_and_the_corner_at_the_bands_edge(orc):
    """(0,0) is in the band for d0 in [-63, 64]; (len1, len2) for len2 - len1 - d0 in [-64, 63].  Which masks still align follows
    from the geometry alone (feasible_by_hand), and the hand-written expectations below agree with it."""
    rng = np.random.default_rng(7)
    sm = match_matrix(2, -3)
    # the origin: len1 = len2 + d0 keeps the corner on diagonal 0 of the band
    for d0, origin in ((-64, False), (-63, True), (64, True), (65, False)):
        len1, len2 = (100, 100 + d0) if d0 > 0 else (100 - d0, 100)
        a, b = related_pairs(rng, 4, len1, len2, d0)
        for mask in ALL_MASKS:
            got = orc.align(a, b, sm, 5, 1, mask, [d0] * 4)
            # without (0,0) the start must be a free border cell in the band: column 0 (BEGIN1) for d0 < 0, row 0 (BEGIN2) for d0 > 0
            want = origin or bool(mask & (BEGIN1 if d0 < 0 else BEGIN2))
            assert want == feasible_by_hand(len1, len2, d0, mask), (d0, mask)
            assert ((got[0] != NO_ALIGNMENT) == want).all(), (d0, mask)
            if want and not origin:
                assert (got[1][:, 2 + (d0 > 0)] > 0).all() and (got[1][:, 3 - (d0 > 0)] == 0).all(), (d0, mask)
    # the corner: d0 = 0, len2 - len1 = -65, -64, 63, 64
    for diff, corner in ((-65, False), (-64, True), (63, True), (64, False)):
        len1, len2 = (100 - diff, 100) if diff < 0 else (100, 100 + diff)
        a, b = related_pairs(rng, 4, len1, len2, 0)
        for mask in ALL_MASKS:
            got = orc.align(a, b, sm, 5, 1, mask)
            # without the corner the end must be free: column len2 (END1) for the tall table, row len1 (END2) for the wide one
            want = corner or bool(mask & (ANYWHERE | (END1 if diff < 0 else END2)))
            assert want == feasible_by_hand(len1, len2, 0, mask), (diff, mask)
            assert ((got[0] != NO_ALIGNMENT) == want).all(), (diff, mask)
    # every int32 is legal
    a, b = related_pairs(rng, 2, 70, 90, 0)
    for d0 in (INT32_MIN, INT32_MAX, 90 + 65, -70 - 64, 1 << 20):       # nothing of the band on the table
        for mask in (0, 15, 19):
            got = orc.align(a, b, sm, 5, 1, mask, [d0] * 2)
            assert (got[0] == NO_ALIGNMENT).all() and not got[1].any() and not got[3].any(), (d0, mask)
            assert np.array_equal(orc.align(a, b, sm, 5, 1, mask, [d0] * 2, traceback=False)[1], [[0, 0, -1, -1]] * 2)
    # one cell of the band on the table: (0, len2) or (len1, 0); overlap aligns nothing there at score 0
    for d0, cell in ((90 + 64, (0, 90)), (-70 - 63, (70, 0))):
        got = orc.align(a, b, sm, 5, 1, 15, [d0] * 2)
        assert (got[0] == 0).all() and [tuple(r) for r in got[1]] == [cell + cell] * 2 and not got[3].any(), d0
