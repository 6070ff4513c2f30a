"""The profile aligners' host-only parts, no device needed (libswmi_wide_profile.so, include/swmi_wide_profile.h,
swmi.wide_profile): the C restatement tests/native/wide_profile_oracle.c tied three ways to code that exists -- to
wide_affine_oracle.c through from_sequence profiles, to it again through arbitrary profiles read as a matrix against the
sequence 0, 1, .., len2 - 1, and to an independent numpy Gotoh with position scores; the header and the library's symbols;
every refusal with code and text in a process with no GPU bound; the host-only entries; that the batch the GPU tests run is not
trivial; and the compiler's resource remarks of the 16 kernels.  Every comparison is exact integer equality."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from conftest import PKG, ROOT
from wide_profile_support import (GAPS, SEAMS, ProfileOracle, all_len2s, from_sequence, numpy_gotoh_profile, path_cells, profile_for,
                                  sequences_for)
from wide_support import ALL_MASKS, GLOBAL, LOCAL, WideOracle, assert_same, asymmetric_matrix, inputs, moves_of, scoring_matrix

ENTRIES = ["swmi_wide_profile_local", "swmi_wide_profile_global", "swmi_wide_profile_local_device", "swmi_wide_profile_global_device",
           "swmi_wide_profile_from_sequence", "swmi_wide_profile_move_offsets", "swmi_wide_profile_slices_for",
           "swmi_wide_profile_time_device", "swmi_wide_profile_release_workspaces", "swmi_wide_profile_last_error",
           "swmi_wide_profile_version"]
MAX1, MAX2 = 16384, 4096


def _off(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, np.uint64))
    return off


@pytest.fixture(scope="module")
def poracle(tmp_path_factory):
    return ProfileOracle(tmp_path_factory.mktemp("wide_profile_oracle"))


@pytest.fixture(scope="module")
def woracle(tmp_path_factory):
    return WideOracle(tmp_path_factory.mktemp("wide_oracle_for_profile"))


@pytest.fixture(scope="module")
def wp(swmi_mod):
    swmi_mod.wide_profile.load()
    return swmi_mod.wide_profile


def _masks(kind):
    return [0] if kind == LOCAL else ALL_MASKS


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_with_from_sequence_profiles_equals_the_wide_restatement(poracle, woracle, seed):
    rng = np.random.default_rng(seed)
    for len2 in (0, 1, 17, 40, 130):
        shapes = [(int(rng.integers(0, 90)), len2) for _ in range(7)] + [(0, len2), (1, len2), (90, len2)]
        a, b = inputs(shapes, seed=seed * 100 + len2)
        b = [b[0]] * len(a)                                        # one query for the whole batch
        for sm, gaps in ((asymmetric_matrix(seed), (5, 2)), (scoring_matrix(seed + 3), (4, 1)), (scoring_matrix(seed + 4), (0, 0))):
            profile = from_sequence(b[0], sm)
            for kind in (LOCAL, GLOBAL):
                for mask in _masks(kind):
                    assert_same(poracle.align(kind, a, profile, gaps[0], gaps[1], mask), woracle.align(kind, a, b, sm, gaps[0], gaps[1], mask),
                                ("from_sequence", kind, mask, len2, gaps))
            eo = poracle.align(LOCAL, a, profile, gaps[0], gaps[1], traceback=False)
            assert_same(eo, woracle.align(LOCAL, a, b, sm, gaps[0], gaps[1], traceback=False), ("ends-only", len2), traceback=False)


@pytest.mark.parametrize("seed", [3, 4])
def test_restatement_with_arbitrary_profiles_equals_the_wide_restatement_on_the_counting_sequence(poracle, woracle, seed):
    """profile[j, a] read as sm[a, j], against seq2 = (0, 1, .., len2 - 1): only possible up to 32 columns."""
    rng = np.random.default_rng(seed)
    for len2 in (1, 5, 31, 32):
        profile = rng.integers(-128, 128, (len2, 32)).astype(np.int8)
        sm = np.zeros((32, 32), np.int8)
        sm[:, :len2] = profile.T
        a, _ = inputs([(int(rng.integers(0, 70)), 1) for _ in range(8)], seed=seed + len2)
        b = [np.arange(len2, dtype=np.uint8)] * len(a)
        for gaps in ((30, 7), (0, 0), (3, 9)):
            for kind in (LOCAL, GLOBAL):
                for mask in _masks(kind):
                    assert_same(poracle.align(kind, a, profile, gaps[0], gaps[1], mask), woracle.align(kind, a, b, sm, gaps[0], gaps[1], mask),
                                ("counting", kind, mask, len2, gaps))


@pytest.mark.parametrize("seed", [5, 6])
def test_restatement_equals_an_independent_numpy_gotoh_with_position_scores(poracle, seed):
    rng = np.random.default_rng(seed)
    for len2, lo, hi, gaps in ((40, -6, 9, (3, 1)), (33, -128, 127, (5, 2)), (7, -3, 4, (0, 0)), (1, -6, 9, (1, 4)), (0, 0, 1, (2, 1))):
        profile = rng.integers(lo, hi + 1, (len2, 32)).astype(np.int8)
        a, _ = inputs([(int(rng.integers(0, 41)), 1) for _ in range(6)] + [(40, 1), (1, 1), (0, 1)], seed=seed * 10 + len2)
        for kind in (LOCAL, GLOBAL):
            for mask in _masks(kind):
                got = poracle.align(kind, a, profile, gaps[0], gaps[1], mask)
                for k in range(len(a)):
                    score, ends, moves = numpy_gotoh_profile(kind, a[k], profile, gaps[0], gaps[1], mask)
                    what = (kind, mask, len(a[k]), len2, gaps)
                    assert int(got[0][k]) == score and list(got[1][k]) == ends, (what, int(got[0][k]), score, list(got[1][k]), ends)
                    assert moves_of(got, k) == moves, what


def test_header_declares_and_library_exports_exactly_the_eleven_entries(wp):
    with open(os.path.join(ROOT, "include", "swmi_wide_profile.h")) as fh:
        header = fh.read()
    for name in ENTRIES:
        assert re.search(r"SWMI_API\s+[\w \*]+?\b%s\(" % name, header), name
    assert len(re.findall(r"SWMI_API", header)) == len(ENTRIES) == 11
    assert "swmi_wide_profile_expand_moves" not in header            # one expander: libswmi.so's
    lib = os.path.join(PKG, "lib", "libswmi_wide_profile.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if " T " in line}
    assert exported == set(ENTRIES), sorted(exported ^ set(ENTRIES))
    undefined = subprocess.run(["nm", "-D", "--undefined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    taken = {line.split()[-1] for line in undefined.splitlines() if re.search(r"\bswmi_", line)}
    assert taken <= {"swmi_local_full_ragged_move_offsets", "swmi_last_error", "swmi_local_full_expand_moves"}, taken
    needed = subprocess.run(["readelf", "-d", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "libswmi.so" in needed and "libswmi_wide.so" not in needed and "$ORIGIN" in needed
    assert wp.version() == 300


def test_every_refusal_works_with_no_device(wp, swmi_mod):
    lib = wp.load()
    prof = np.zeros(64 * 32, np.int8)
    big = np.zeros((MAX2 + 1) * 32, np.int8)
    s1 = np.zeros(64, np.uint8)
    out = np.zeros(64, np.int64)
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    long1 = np.array([0, 3, 3 + MAX1 + 1, 3 + MAX1 + 2, 3 + MAX1 + 3], np.uint64)      # a length of 16385
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    INV, DOM, ALN = swmi_mod.ERR_INVALID_ARGUMENT, swmi_mod.ERR_DOMAIN, swmi_mod.ERR_ALIGNMENT

    def local(o1, go=1, ge=1, s1p=p(s1), mv=p(out), st=p(out), n=4, pp=p(prof), len2=64, sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_profile_local(s1p, p(o1), n, pp, len2, go, ge, sc, en, mv, st)

    def glob(o1, go=1, ge=1, s1p=p(s1), mv=p(out), st=p(out), n=4, pp=p(prof), len2=64, sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_profile_global(s1p, p(o1), n, pp, len2, go, ge, mask, sc, en, mv, st)

    def local_dev(o1, go=1, ge=1, s1p=p(s1), mv=p(out), st=p(out), n=4, pp=p(prof), len2=64, sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_profile_local_device(s1p, p(o1), n, pp, len2, go, ge, sc, en, mv, st, None)

    def glob_dev(o1, go=1, ge=1, s1p=p(s1), mv=p(out), st=p(out), n=4, pp=p(prof), len2=64, sc=p(out), en=p(out), mask=0):
        return lib.swmi_wide_profile_global_device(s1p, p(o1), n, pp, len2, go, ge, mask, sc, en, mv, st, None)

    for f in (local, glob, local_dev, glob_dev):
        # the new ones
        assert f(good, pp=p(big), len2=MAX2 + 1) == INV and "len2 4097 > 4096" in wp.last_error()
        assert f(good, pp=None) == INV and "profile is NULL with len2 > 0" in wp.last_error()
        assert f(good, pp=None, len2=1) == INV and "profile is NULL" in wp.last_error()
        assert f(long1) == INV and "seq1_offsets: sequence 1 has length 16385 > 16384" in wp.last_error()
        # swmi_wide.h's
        assert f(bad_dec) == INV and "seq1_offsets decrease at 1" in wp.last_error()
        assert f(None) == INV and "seq1_offsets is NULL" in wp.last_error()
        assert f(good, mv=None) == INV and "moves and steps" in wp.last_error()
        assert f(good, st=None) == INV and "moves and steps" in wp.last_error()
        for name in ("s1p", "sc", "en"):
            assert f(good, **{name: None}) == INV and "NULL buffer" in wp.last_error(), name
        for go, ge in ((-1, 1), (128, 1), (1, -1), (1, 128)):
            assert f(good, go=go, ge=ge) == DOM and "outside [0,127]" in wp.last_error()
        # n = 0 returns before the buffers, the offsets and len2 are looked at, but after the profile, the gaps and moves / steps
        assert f(bad_dec, n=0, s1p=None) == 0 and f(None, n=0, pp=p(big), len2=MAX2 + 1) == 0
        assert f(good, n=0, go=200) == DOM and f(good, n=0, mv=None) == INV and f(good, n=0, pp=None) == INV
        # the order: the profile before the gaps, those before the moves / steps pair, that before the buffers, those before
        # the offsets, those before len2
        assert f(good, pp=None, go=-1) == INV and "profile is NULL" in wp.last_error()
        assert f(bad_dec, go=-1, mv=None) == DOM and f(bad_dec, mv=None, sc=None) == INV and "moves and steps" in wp.last_error()
        assert f(bad_dec, sc=None) == INV and "NULL buffer" in wp.last_error()
        assert f(bad_dec, pp=p(big), len2=MAX2 + 1) == INV and "seq1_offsets decrease" in wp.last_error()
    for f in (glob, glob_dev):
        assert f(good, mask=16) == INV and "free_ends 16 above 15" in wp.last_error()
        assert f(good, mask=16, go=-1, pp=None) == INV and "free_ends" in wp.last_error()       # the mask comes first
    for f in (local_dev, glob_dev):
        assert f(good, sc=p(out) + 8) == ALN and "16-byte aligned" in wp.last_error()
    ms = ctypes.c_float()
    t = lambda kind=0, iters=1, n=4, ms=ctypes.byref(ms): lib.swmi_wide_profile_time_device(kind, p(s1), p(good), n, p(prof), 64, 1, 1, 0,   # noqa: E731
                                                                                             p(out), p(out), None, None, None, iters, ms)
    assert t(kind=2) == INV and t(iters=0) == INV and t(n=0) == INV and t(ms=None) == INV
    # the Python layer: what ctypes or the cast would wrap raises, as elsewhere
    seqs = [np.zeros(3, np.uint8)]
    with pytest.raises(swmi_mod.SwmiError) as e:
        wp.local(seqs, prof, 2**32 + 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wp.global_(seqs, np.full(64, 300), 1, 1)
    assert e.value.code == DOM
    with pytest.raises(swmi_mod.SwmiError) as e:
        wp.global_(seqs, prof, 1, 1, free_ends=-1)
    assert e.value.code == INV
    with pytest.raises(swmi_mod.SwmiError) as e:
        wp.local(seqs, big, 1, 1)
    assert e.value.code == INV and "4097" in str(e.value)
    with pytest.raises(swmi_mod.SwmiError) as e:
        wp.local([np.zeros(MAX1 + 1, np.uint8)], prof, 1, 1)
    assert e.value.code == INV and "16385" in str(e.value)
    with pytest.raises(ValueError):
        wp.local(seqs, np.zeros(33, np.int8), 1, 1)
    # an empty batch needs no device
    r = wp.local([], prof, 1, 1)
    assert len(r[0]) == 0 and r[1].shape == (0, 4)


def test_from_sequence_byte_by_byte(wp, swmi_mod):
    rng = np.random.default_rng(7)
    sm = asymmetric_matrix(8)
    for len2 in (0, 1, 33, MAX2):
        q = rng.integers(0, 256, len2, dtype=np.uint8)           # junk in bits 5 - 7
        got = wp.from_sequence(q, sm)
        assert got.dtype == np.int8 and got.shape == (len2, 32)
        m = sm.reshape(32, 32)
        for j in (range(len2) if len2 <= 33 else (0, 1, 1023, 1024, MAX2 - 1)):
            for a in range(32):
                assert got[j, a] == m[a, q[j] & 31], (len2, j, a)
        assert np.array_equal(got, from_sequence(q, sm))
    lib = wp.load()
    out = np.zeros(64, np.int8)
    q = np.zeros(8, np.uint8)
    INV = swmi_mod.ERR_INVALID_ARGUMENT
    assert lib.swmi_wide_profile_from_sequence(q.ctypes.data, MAX2 + 1, sm.ctypes.data, out.ctypes.data) == INV and "4097" in wp.last_error()
    assert lib.swmi_wide_profile_from_sequence(q.ctypes.data, 2, None, out.ctypes.data) == INV and "score_matrix is NULL" in wp.last_error()
    assert lib.swmi_wide_profile_from_sequence(None, 2, sm.ctypes.data, out.ctypes.data) == INV and "NULL buffer" in wp.last_error()
    assert lib.swmi_wide_profile_from_sequence(None, 0, sm.ctypes.data, None) == 0


def test_move_offsets_equal_the_ragged_layout_on_k_times_len2(wp, swmi_mod):
    rng = np.random.default_rng(9)
    for len2 in (0, 1, 31, 1025, MAX2):
        lens = list(rng.integers(0, 300, 50)) + [0, MAX1, 1]
        off1 = _off(lens)
        off2 = np.arange(len(lens) + 1, dtype=np.uint64) * np.uint64(len2)
        got = wp.move_offsets(off1, len2)
        assert np.array_equal(got, swmi_mod.local_full_ragged_move_offsets(off1, off2)), len2
        assert got[-1] == sum((((int(x) + len2 + 31) // 32) + 1) & ~1 for x in lens)
    lib = wp.load()
    out = np.zeros(8, np.uint64)
    good = _off([3, 4])
    INV = swmi_mod.ERR_INVALID_ARGUMENT
    assert lib.swmi_wide_profile_move_offsets(good.ctypes.data, 2, 5, None) == INV and "move_offsets is NULL" in wp.last_error()
    assert lib.swmi_wide_profile_move_offsets(None, 2, 5, out.ctypes.data) == INV and "seq1_offsets is NULL" in wp.last_error()
    assert lib.swmi_wide_profile_move_offsets(good.ctypes.data, 2, MAX2 + 1, out.ctypes.data) == INV and "len2 4097" in wp.last_error()
    assert np.array_equal(wp.move_offsets(np.zeros(1, np.uint64), 7), [0])


def test_slices_for_on_hand_checkable_offsets(wp, swmi_mod):
    lib = wp.load()
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    good = _off([3, 0, 10, 5])
    bad_dec = np.array([0, 3, 2, 10, 15], np.uint64)
    long1 = np.array([0, 3, 3 + MAX1 + 1, 3 + MAX1 + 2, 3 + MAX1 + 3], np.uint64)
    for tb in (0, 1):
        for bad in (bad_dec, None, long1):
            assert lib.swmi_wide_profile_slices_for(p(bad), 4, 10, tb, None, 0) == 0
        assert lib.swmi_wide_profile_slices_for(p(good), 4, MAX2 + 1, tb, None, 0) == 0
        assert lib.swmi_wide_profile_slices_for(p(good), 4, MAX2, tb, None, 0) == 1
        sizes = (ctypes.c_size_t * 2)(99, 99)
        assert lib.swmi_wide_profile_slices_for(p(good), 4, 0, tb, sizes, 2) == 1
        assert list(sizes) == [4, 99]
    assert wp.slices_for(np.zeros(1, np.uint64), 5) == []
    # the count cap: a slice holds at most 2^20 alignments
    n = (1 << 20) + 5
    assert wp.slices_for(_off(np.ones(n, np.uint64)), 3, traceback=False) == [1 << 20, 5]

    # the traceback budget is swmi_wide's: what 256 alignments of 16384 x 4096 take there, a seq2 of 4096 bytes each included.
    # Here an alignment takes len1 + 48 (slot) + 20 (results) + 4 (steps) + 8 x (codes + moves) and no seq2, and the profile's
    # 32768 x waves bytes count once per slice.
    def bytes_tb(len1, len2, seq2):
        trips = ((len1 + 63 + 31) // 32) * 8
        codes = ((len2 + 1023) // 1024) * trips * 256
        return len1 + seq2 + 48 + 20 + 4 + 8 * (codes + ((((len1 + len2 + 31) // 32) + 1) & ~1))
    budget = 256 * bytes_tb(MAX1, MAX2, MAX2)
    # 300 of the largest shape: 256 of them leave 256 x 4096 - 131072 bytes of the budget, less than one more
    assert 256 * bytes_tb(MAX1, MAX2, 0) + 4 * 32768 <= budget < 257 * bytes_tb(MAX1, MAX2, 0) + 4 * 32768
    assert wp.slices_for(_off([MAX1] * 300), MAX2) == [256, 44]
    # 16384 x 1024 has a quarter of the codes: the bytes cut the batch
    per_slice = (budget - 32768) // bytes_tb(MAX1, 1024, 0)
    assert 1000 < per_slice < 1100
    assert wp.slices_for(_off([MAX1] * 2100), 1024) == [per_slice, per_slice, 2100 - 2 * per_slice]
    # the profile's bytes grow with the waves: 1025 columns are two
    per_slice2 = (budget - 2 * 32768) // bytes_tb(MAX1, 1025, 0)
    assert wp.slices_for(_off([MAX1] * (per_slice2 + 3)), 1025) == [per_slice2, 3]
    # ends-only: 256 MiB of sequences, slots and results, and the profile once
    per_slice = ((256 << 20) - 4 * 32768) // (MAX1 + 48 + 20)
    assert wp.slices_for(_off([MAX1] * (per_slice + 7)), MAX2, traceback=False) == [per_slice, 7]
    # ... and one more alignment would fit where the wide aligners ship a seq2 each
    assert per_slice > (256 << 20) // (MAX1 + MAX2 + 48 + 20)


def test_module_is_a_submodule_with_docstrings(swmi_mod):
    wp = swmi_mod.wide_profile
    assert isinstance(wp, types.ModuleType) and wp.__name__ == "swmi.wide_profile" and wp.__doc__
    public = ["local", "global_", "local_device", "global_device", "from_sequence", "move_offsets", "slices_for", "time_device",
              "release_workspaces", "search", "last_error", "version", "load"]
    for name in public:
        fn = getattr(wp, name)
        assert inspect.isfunction(fn) and fn.__module__ == "swmi.wide_profile" and fn.__doc__, name
    for name in ("from_sequence", "search"):
        assert not hasattr(swmi_mod, name), name
    assert list(inspect.signature(wp.search).parameters) == ["seqs", "profile", "gap_open", "gap_extend", "top", "kind", "free_ends"]
    assert (wp.LOCAL, wp.GLOBAL, wp.MAX_LEN1, wp.MAX_LEN2, wp.LETTERS) == (0, 1, MAX1, MAX2, 32)


def test_the_gpu_batch_is_not_trivial(poracle):
    """What test_wide_profile_gpu.py's comparisons rest on, shown through the restatement alone (seeds chosen here)."""
    go, ge = GAPS["scoring"]
    kinds_of_move, zero_scores = set(), 0
    for len2 in all_len2s():
        seqs = sequences_for(len2)
        cat = np.concatenate(seqs)
        if len2 == 4096:
            assert len(np.unique(cat & 31)) == 32 and len(np.unique(cat >> 5)) == 8          # all 32 letters, junk in bits 5 - 7
        local = poracle.align(LOCAL, seqs, profile_for("scoring", len2), go, ge)
        for k in range(len(seqs)):
            kinds_of_move |= set(moves_of(local, k))
        zero_scores += int(np.sum((local[0] == 0) & (np.array([len(x) for x in seqs]) > 0)))
    assert kinds_of_move == {1, 2, 3}
    assert zero_scores >= 1                                                                   # a local score of 0, both lengths non-zero
    # len2 = 4096: the sequences of 127, 128 and 129 hold a window across column 1024, 2048 and 3072, and their local paths
    # straddle it
    seqs = sequences_for(4096)
    profile = profile_for("scoring", 4096)
    local = poracle.align(LOCAL, seqs, profile, go, ge)
    lens = [len(x) for x in seqs]
    for len1, seam in zip((127, 128, 129), SEAMS):
        k = lens.index(len1)
        cols = [j for _, j in path_cells(local, k)]
        assert min(cols) <= seam - 20 and max(cols) >= seam + 20, (len1, seam, min(cols), max(cols))
        assert int(local[0][k]) > 100
    # ... and the global path of the sequence of 200 has diagonal moves in every wave's columns
    glob = poracle.align(GLOBAL, seqs, profile, go, ge, 0)
    k = lens.index(200)
    waves = {(j - 1) // 1024 for _, j in path_cells(glob, k)}
    assert waves == {0, 1, 2, 3} and list(glob[1][k]) == [200, 4096, 0, 0]
    assert {1, 2, 3} <= set(moves_of(glob, k))
    # the extremes do what they are there for: -128 everywhere floors every local score, 127 everywhere never does
    assert (poracle.align(LOCAL, seqs, profile_for("all_-128", 4096), 3, 2)[0] == 0).all()
    assert (poracle.align(LOCAL, seqs[1:], profile_for("all_127", 4096), 0, 0)[0] == 127 * np.array(lens[1:])).all()
    # the last columns: the sequences of 31 .. 33 end their local paths in the last lane's columns at the lane edges
    for len2 in (15, 17, 1023, 1025, 3073):
        s = sequences_for(len2)
        r = poracle.align(LOCAL, s, profile_for("scoring", len2), go, ge)
        assert max(int(r[1][k, 1]) for k in range(len(s))) >= len2 - 2, len2


def test_no_kernel_spills_or_uses_scratch(tmp_path):
    """The compiler's resource remarks of the 16 kernels (kind x traceback x wave count), with csrc/Makefile's flags: no scratch,
    no VGPR or SGPR spill, and the wide kernels' static LDS per wave count."""
    hipcc = "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc)
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.s"), os.path.join(csrc, "wide_profile_kernels.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=csrc)
    assert r.returncode == 0, r.stdout[-3000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stdout)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        m = re.match(r"_ZN4swmi\d+_GLOBAL__N_1\d+wide_profile_(local|global)_kernelILb([01])ELi([1-4])E", name)
        if not m:
            continue
        field = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))  # noqa: E731
        seen[m.groups()] = (field("ScratchSize [bytes/lane]"), field("SGPRs Spill"), field("VGPRs Spill"), field("LDS Size [bytes/block]"))
    assert len(seen) == 16, sorted(seen)
    for (kind, tb, waves), (scratch, sgpr_spill, vgpr_spill, lds) in seen.items():
        assert scratch == 0 and sgpr_spill == 0 and vgpr_spill == 0, (kind, tb, waves, scratch, sgpr_spill, vgpr_spill)
        # W x 32 KiB of profile, the ring of max(W - 1, 1) x 256 int2, a few words
        base = int(waves) * 32768 + max(int(waves) - 1, 1) * 2048
        assert base <= lds <= base + 64, (kind, tb, waves, lds)
