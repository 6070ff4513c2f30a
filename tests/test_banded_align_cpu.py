"""The banded local aligner's host-only parts, no device needed (libswmi_banded.so, include/swmi_banded.h, swmi.banded): the
header and the library's symbols; every refusal with code and text in a process with no GPU bound; the slice arithmetic on
hand-computed sizes; the compiler's resource remarks of the four kernels; and the C restatement
tests/native/banded_align_oracle.c tied to code that exists -- to oracle/sw_oracle.c's sw_oracle_banded_affine (identity 1),
to tests/native/local_full_affine_oracle.c where that one's path stays in the band (identity 2), to
tests/native/local_full_oracle.c with open = extend (identity 3) -- and shown to tell a band that is off by one on either side
in every edge family of tests/banded_edges.py.  Every comparison is exact integer equality."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import banded_edges
from banded_align_support import (INT32_MAX, INT32_MIN, RELATED_DIAGONALS, RELATED_PARAMS, TB_BUDGET, BandedOracle, assert_same, code_bytes,
                                  in_band, move_words, numpy_band_table, path_from, per_alignment, related_pairs)
from conftest import PKG, ROOT, match_matrix
from local_full_affine_support import LocalFullAffineOracle
from local_full_support import LocalFullOracle

ENTRIES = ["swmi_banded_local", "swmi_banded_local_device", "swmi_banded_slices_for", "swmi_banded_time_device",
           "swmi_banded_release_workspaces", "swmi_banded_last_error", "swmi_banded_version"]
MAX = 16384


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return BandedOracle(tmp_path_factory.mktemp("banded_align_oracle"))


@pytest.fixture(scope="module")
def bd(swmi_mod):
    swmi_mod.banded.load()
    return swmi_mod.banded


def test_header_declares_and_library_exports_exactly_the_seven_entries(bd):
    with open(os.path.join(ROOT, "include", "swmi_banded.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 7
    assert "expand_moves(" not in header.replace("swmi_local_full_expand_moves", "")          # one expander: libswmi.so's
    lib = os.path.join(PKG, "lib", "libswmi_banded.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}     # it calls nothing of libswmi.so
    needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libswmi.so" in needed and "libswmi_wide" not in needed and "$ORIGIN" in needed
    assert bd.version() == 300


def test_every_refusal_works_with_no_device(bd, swmi_mod):
    lib = bd.load()
    buf = np.zeros(4096, np.int64)
    sm = np.zeros(16, np.int8)
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT
    ms = ctypes.c_float()

    def host(len1=8, len2=8, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_local(s1, len1, s2, len2, n, dg, m, go, ge, sc, en, mv, st)

    def dev(len1=8, len2=8, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_local_device(s1, len1, s2, len2, n, dg, m, go, ge, sc, en, mv, st, None)

    def timer(len1=8, len2=8, n=2, go=1, ge=1, s1=p(buf), s2=p(buf), dg=p(buf), m=p(sm), sc=p(buf), en=p(buf), mv=p(buf), st=p(buf)):
        return lib.swmi_banded_time_device(s1, len1, s2, len2, n, dg, m, go, ge, sc, en, mv, st, None, 1, ctypes.byref(ms))

    for f in (host, dev, timer):
        for len1, len2 in ((0, 8), (8, 0), (MAX + 1, 8), (8, MAX + 1)):
            assert f(len1=len1, len2=len2) == INV and "len1 %d / len2 %d outside [1,16384]" % (len1, len2) in bd.last_error(), (len1, len2)
        for name in ("s1", "s2", "sc", "en"):
            assert f(**{name: None}) == INV and "NULL buffer with n = 2" in bd.last_error(), name
        assert f(m=None) == INV and "score_matrix is NULL" in bd.last_error()
        assert f(mv=None) == INV and "moves and steps" in bd.last_error()
        assert f(st=None) == INV and "moves and steps" in bd.last_error()
        for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
            assert f(go=go, ge=ge) == DOM and "gap_open %d / gap_extend %d outside [0,127]" % (go, ge) in bd.last_error()
        # the order: the matrix before the gaps, those before the moves / steps pair, that before the buffers, those before the
        # lengths
        assert f(m=None, go=-1) == INV and "score_matrix" in bd.last_error()
        assert f(go=-1, mv=None) == DOM and f(mv=None, sc=None) == INV and "moves and steps" in bd.last_error()
        assert f(sc=None, len1=0) == INV and "NULL buffer" in bd.last_error()
    for f in (host, dev):
        # n = 0 is a no-op behind the matrix, the gaps and the moves / steps pair and in front of the buffers and the lengths
        assert f(n=0, s1=None, len1=0) == 0
        assert f(n=0, go=200) == DOM and f(n=0, mv=None) == INV and f(n=0, m=None) == INV
    assert timer(n=0) == INV and "n is 0" in bd.last_error()
    assert lib.swmi_banded_time_device(p(buf), 8, p(buf), 8, 2, None, p(sm), 1, 1, p(buf), p(buf), None, None, None, 0, ctypes.byref(ms)) == INV
    assert lib.swmi_banded_time_device(p(buf), 8, p(buf), 8, 2, None, p(sm), 1, 1, p(buf), p(buf), None, None, None, 1, None) == INV
    for name in ("s1", "s2", "dg", "sc", "en", "mv", "st"):
        assert dev(**{name: p(buf) + 8}) == ALN and "16-byte aligned" in bd.last_error(), name
    # the Python layer: what ctypes or the cast would wrap raises, as elsewhere
    a = np.zeros((2, 8), np.uint8)
    with pytest.raises(swmi_mod.SwmiError) as e:
        bd.local(a, a, sm, 2**32 + 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        bd.local(a, a, np.full(16, 300), 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        bd.local(np.zeros((1, MAX + 1), np.uint8), a[:1], sm, 1, 1)
    assert e.value.code == INV and "16385" in str(e.value)
    with pytest.raises(ValueError):
        bd.local(a, a, sm, 1, 1, diagonals=[0])
    with pytest.raises(ValueError):
        bd.local(a, a, sm, 1, 1, diagonals=[0, 2**31])
    with pytest.raises(ValueError):
        bd.local(a, a[:1], sm, 1, 1)
    # an empty batch needs no device
    r = bd.local(np.zeros((0, 8), np.uint8), np.zeros((0, 9), np.uint8), sm, 1, 1)
    assert len(r[0]) == 0 and r[1].shape == (0, 4) and r[2].shape == (0, move_words(8, 9))


def test_slices_for_on_hand_computed_sizes(bd, swmi_mod):
    lib = bd.load()
    for tb in (0, 1):
        for len1, len2 in ((0, 8), (8, 0), (MAX + 1, 8), (8, MAX + 1)):
            assert lib.swmi_banded_slices_for(10, len1, len2, tb, None, 0) == 0 and "outside [1,16384]" in bd.last_error()
        assert lib.swmi_banded_slices_for(0, 8, 8, tb, None, 0) == 0
        sizes = (ctypes.c_size_t * 3)(99, 99, 99)
        assert lib.swmi_banded_slices_for(10, 8, 8, tb, sizes, 3) == 1 and list(sizes) == [10, 99, 99]
    assert bd.slices_for(0, 5, 5) == []
    # the count cap: a slice holds at most 2^20 alignments
    assert bd.slices_for((1 << 20) + 5, 3, 2, traceback=False) == [1 << 20, 5]
    # ends-only: 256 MiB of sequences, diagonals and results: 32768 + 4 + 20 bytes each at the largest shape
    assert per_alignment(MAX, MAX, False) == 32792
    per_slice = (256 << 20) // 32792
    assert per_slice == 8186 and 8186 * 32792 == 268435312
    assert bd.slices_for(2 * per_slice + 7, MAX, MAX, traceback=False) == [per_slice, per_slice, 7]
    # with a traceback the budget is swmi_local_affine_slices_for's, 4096 alignments of its largest shape ...
    assert TB_BUDGET == 4383801344
    assert swmi_mod.local_affine_slices_for(5000, MAX) == [4096, 904]
    # ... of which an alignment of 16384 x 16384 takes 256 x 4112 of codes, 8 x 1024 of moves, 4 of steps and the 32792 above
    assert code_bytes(MAX) == 256 * 4112 == 64 * (MAX + 64) and move_words(MAX, MAX) == 1024
    assert per_alignment(MAX, MAX, True) == 32792 + 1052672 + 8192 + 4 == 1093660
    assert TB_BUDGET // 1093660 == 4008
    assert bd.slices_for(10000, MAX, MAX) == [4008, 4008, 1984]
    # 1024 x 1024: 256 x 272 of codes, 8 x 64 of moves
    assert per_alignment(1024, 1024, True) == 2048 + 24 + 69632 + 512 + 4 == 72220
    per_slice = TB_BUDGET // 72220
    assert per_slice == 60700 and 60700 * 72220 <= TB_BUDGET < 60701 * 72220
    assert bd.slices_for(65536, 1024, 1024) == [per_slice, 65536 - per_slice]
    # len2 only counts with its bytes and its move words: the codes depend on len1 alone
    assert per_alignment(1024, 1, True) == 1024 + 1 + 24 + 69632 + 8 * 34 + 4
    assert bd.slices_for(70000, 1024, 1) == [TB_BUDGET // per_alignment(1024, 1, True), 70000 - TB_BUDGET // per_alignment(1024, 1, True)]


def test_module_is_a_submodule_with_docstrings(swmi_mod):
    bd = swmi_mod.banded
    assert isinstance(bd, types.ModuleType) and bd.__name__ == "swmi.banded" and bd.__doc__
    for name in ["local", "local_device", "slices_for", "move_words", "paths", "time_device", "release_workspaces", "last_error", "version",
                 "load"]:
        fn = getattr(bd, name)
        assert inspect.isfunction(fn) and fn.__module__ == "swmi.banded" and fn.__doc__, name
    assert list(inspect.signature(bd.local).parameters) == ["seq1s", "seq2s", "score_matrix", "gap_open", "gap_extend", "diagonals", "traceback"]
    assert inspect.signature(bd.local).parameters["diagonals"].default is None and inspect.signature(bd.local).parameters["traceback"].default is True
    assert not hasattr(swmi_mod, "paths")
    assert (bd.MAX_LEN, bd.WIDTH, bd.LO, bd.HI) == (MAX, 128, -64, 63)
    assert bd.move_words(300, 1025) == move_words(300, 1025) == swmi_mod.local_full_move_words(300, 1025)


def test_no_kernel_spills_or_uses_scratch(tmp_path):
    """The compiler's resource remarks of the four kernels (open >= extend x traceback), with csrc/Makefile's flags: no scratch,
    no VGPR or SGPR spill, and an LDS that does not depend on any length: the walk window of the traceback kernels (4 wavefronts
    x 16 trips x 256 bytes), nothing in the ends-only kernels."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.s"), os.path.join(csrc, "banded_align_kernels.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=csrc)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stdout)[1:]
    seen = {}
    for b in blocks:
        m = re.match(r"_ZN4swmi6banded\d+_GLOBAL__N_1\d+banded_local_kernelILb([01])ELb([01])EE", b.split()[0])
        if not m:
            continue
        field = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))  # noqa: E731
        seen[m.groups()] = (field("ScratchSize [bytes/lane]"), field("SGPRs Spill"), field("VGPRs Spill"), field("LDS Size [bytes/block]"),
                            field("VGPRs"))
    assert sorted(seen) == [("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")], sorted(seen)
    for (oge, tb), (scratch, sgpr_spill, vgpr_spill, lds, vgprs) in seen.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (oge, tb, scratch, sgpr_spill, vgpr_spill)
        assert lds == (4 * 16 * 256 if tb == "1" else 0), (oge, tb, lds)
        assert vgprs <= 128, (oge, tb, vgprs)                # four wavefronts per SIMD or more


def test_identity_1_the_restatement_scores_what_the_scorers_oracle_scores(orc, oracle):
    rng = np.random.default_rng(1)
    for length in (64, 65, 81, 128, 333):
        a, b = banded_edges.related(rng, 12, length)
        b[::3] = rng.integers(0, 4, (4, length), dtype=np.uint8)
        for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 1, 4), (match_matrix(3, 1), 0, 0),
                           (rng.integers(-128, 128, 16).astype(np.int8), 127, 0)):
            assert np.array_equal(orc.align(a, b, sm, go, ge, traceback=False)[0], oracle.banded_affine(a, b, sm, go, ge)), (length, go, ge)
    for c in banded_edges.shift_cases([128]) + banded_edges.corner_cases([79, 128]):
        assert np.array_equal(orc.align(c.a, c.b, c.sm, c.gap_open, c.gap_ext)[0], oracle.banded_affine(c.a, c.b, c.sm, c.gap_open, c.gap_ext)), c


def test_identities_2_and_3_the_restatement_equals_the_full_restatements_where_their_path_stays_in_the_band(orc, tmp_path):
    """The "related" family: seq2 is seq1 with 8 % substitutions and 3 indel runs of 1 - 8 bases behind max(d0, 0) random
    bases, d0 in {0, 40, -37}, len1 = 300 (len2 = 300 and 320).  At least 95 % of the cases must qualify."""
    full = LocalFullAffineOracle(tmp_path)
    linear = LocalFullOracle(tmp_path)
    rng = np.random.default_rng(2)
    cases = inside = 0
    for d0 in RELATED_DIAGONALS:
        for len2 in (300, 320):
            a, b = related_pairs(rng, 25, 300, len2, d0)
            d = np.full(25, d0, np.int32)
            for m, x, go, ge in RELATED_PARAMS:
                sm = match_matrix(m, x)
                got = orc.align(a, b, sm, go, ge, d)
                want = full.align(a, b, sm, go, ge)
                lin = linear.align(a, b, sm, go) if go == ge else None
                assert (got[0] <= want[0]).all()
                for k in range(25):
                    cases += 1
                    path = path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1])
                    if not in_band(path[1:], d0):
                        continue
                    inside += 1
                    one = lambda r: tuple(y[k:k + 1] for y in r)  # noqa: E731
                    assert_same(one(got), one(want), ("identity 2", d0, len2, m, x, go, ge, k))
                    if lin is not None:
                        assert_same(one(got), one(lin), ("identity 3", d0, len2, m, x, go, k))
    assert cases == 600 and inside >= 0.95 * cases, (inside, cases)


def test_the_band_binds_on_unrelated_sequences(orc, tmp_path):
    """Random unrelated 200-mers: the full aligner's path leaves the band in a good part of the cases, and there the banded
    score is lower or the alignment another one; the restatement still equals an independent numpy table."""
    full = LocalFullAffineOracle(tmp_path)
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, (60, 200), dtype=np.uint8)
    b = rng.integers(0, 4, (60, 200), dtype=np.uint8)
    left = lower = 0
    for m, x, go, ge in RELATED_PARAMS:
        sm = match_matrix(m, x)
        got = orc.align(a, b, sm, go, ge)
        want = full.align(a, b, sm, go, ge)
        assert (got[0] <= want[0]).all()
        for k in range(60):
            if not in_band(path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1])[1:]):
                left += 1
                lower += int(got[0][k] < want[0][k])
    assert left >= 20 and lower >= 10, (left, lower)
    for k in range(4):
        H = numpy_band_table(a[k], b[k], match_matrix(2, -3), 5, 1)
        r = orc.align(a[k:k + 1], b[k:k + 1], match_matrix(2, -3), 5, 1)
        assert H.max() == r[0][0] and divmod(int(np.argmax(H.reshape(-1))), 201) == (r[1][0, 0], r[1][0, 1])


def test_a_band_off_by_one_on_either_side_gets_a_case_of_every_edge_family_wrong(orc):
    """test_banded_edges_cpu.py's method on the restatement with the band bounds as arguments: in each family of
    tests/banded_edges.py the contract's band gives the hand values, and every neighbouring band differs on at least one pair."""
    families = {"shift": banded_edges.shift_cases([128, 333]), "gap_run": banded_edges.gap_run_cases([333]),
                "corner": banded_edges.corner_cases([79, 128])}
    for family, cases in families.items():
        wrong = {band: 0 for band in banded_edges.NEIGHBOUR_BANDS}
        for c in cases:
            right = orc.align(c.a, c.b, c.sm, c.gap_open, c.gap_ext)
            hand = c.want >= 0
            assert np.array_equal(right[0][hand], c.want[hand]), c
            bound = c.below >= 0
            assert (right[0][bound] < c.below[bound]).all(), c
            for lo, hi in banded_edges.NEIGHBOUR_BANDS:
                other = orc.align(c.a, c.b, c.sm, c.gap_open, c.gap_ext, lo=lo, hi=hi)
                wrong[(lo, hi)] += int((other[0] != right[0]).sum())
        assert all(wrong.values()), (family, wrong)


def test_the_restatement_on_diagonals_that_leave_little_or_nothing(orc):
    a = np.zeros((1, 70), np.uint8)
    b = np.zeros((1, 90), np.uint8)
    sm = match_matrix(1, -1)
    for d0, score, end in ((90 + 63, 1, (1, 90)), (-70 - 62, 1, (70, 1)), (90 + 62, 2, (2, 90)), (90 + 64, 0, (0, 0)), (-70 - 63, 0, (0, 0)),
                           (INT32_MAX, 0, (0, 0)), (INT32_MIN, 0, (0, 0)), (0, 70, (70, 70)), (84, 70, (70, 90)), (85, 69, (69, 90))):
        r = orc.align(a, b, sm, 127, 127, [d0])
        assert (int(r[0][0]), tuple(r[1][0][:2])) == (score, end), d0
        assert tuple(r[1][0][2:]) == (end[0] - score, end[1] - score) and int(r[3][0]) == score
        eo = orc.align(a, b, sm, 127, 127, [d0], traceback=False)
        assert tuple(eo[1][0]) == end + (-1, -1)
