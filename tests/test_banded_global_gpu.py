"""The banded global / fit / overlap / extension aligner on the GPU (libswmi_banded_global.so, include/swmi_banded_global.h,
swmi.banded_global): every field and every move against the C restatement tests/native/banded_global_oracle.c, with a
traceback and ends-only, in both template forms of the kernel (open >= extend and open < extend) and under every mask; the four
identities that tie it to merged code; path validity without any oracle; the host entry in two slices, the Python module and the
C++ overload.  Every comparison is exact integer equality.

The kernel sweeps whole trips of 4 iterations, i_hi - i_lo + 64 of them rounded up with row 0 swept, so len1 = 61 .. 68 run every
remainder of the trip; it stages no sequence; its walk window holds 64 iterations, which len1 = 127 .. 129 and 191 .. 193 stand
either side of."""
import os
import subprocess

import numpy as np
import pytest
import torch

from banded_global_support import (ALL_MASKS, ANYWHERE, BEGIN1, BEGIN2, END1, END2, IDENTITY_MASKS, INT32_MAX, INT32_MIN, NO_ALIGNMENT,
                                   RELATED_PARAMS, BandedGlobalOracle, assert_same, band_leaver, in_band, move_words, moves_of, path_from,
                                   related_pairs)
from conftest import PKG, ROOT, match_matrix
from global_full_affine_support import check_path

pytestmark = pytest.mark.gpu

FORMS = [(5, 1), (1, 3)]                    # open >= extend, open < extend: the two instantiations


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return BandedGlobalOracle(tmp_path_factory.mktemp("banded_global_oracle"))


@pytest.fixture(scope="module")
def bg(swmi_mod):
    swmi_mod.banded_global.load()
    return swmi_mod.banded_global


def device_call(bg, a, b, sm, go, ge, mask, diagonals=None, traceback=True, stream=None):
    """swmi.banded_global.align_device on fresh tensors; the result as numpy arrays in the host entry's layout."""
    n, len1 = a.shape
    len2 = b.shape[1]
    dev = torch.device("cuda:0")
    ta, tb_ = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    td = None if diagonals is None else torch.from_numpy(np.ascontiguousarray(diagonals, np.int32)).to(dev)
    scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ends = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    moves = torch.zeros((n, move_words(len1, len2)), dtype=torch.int64, device=dev) if traceback else None
    steps = torch.full((n,), -7, dtype=torch.int32, device=dev) if traceback else None
    bg.align_device(ta, tb_, sm, go, ge, scores, ends, moves, steps, free_ends=mask, diagonals=td, stream=stream)
    torch.cuda.synchronize()
    return (scores.cpu().numpy(), ends.cpu().numpy(), moves.cpu().numpy().view(np.uint64) if traceback else None,
            steps.cpu().numpy().view(np.uint32) if traceback else None)


def both_ways(bg, orc, a, b, sm, go, ge, mask, diagonals, what):
    """with a traceback and ends-only against the restatement; returns the traceback result"""
    want = orc.align(a, b, sm, go, ge, mask, diagonals)
    got = device_call(bg, a, b, sm, go, ge, mask, diagonals)
    assert_same(got, want, what)
    eo = device_call(bg, a, b, sm, go, ge, mask, diagonals, traceback=False)
    assert_same(eo, orc.align(a, b, sm, go, ge, mask, diagonals, traceback=False), (what, "ends-only"), traceback=False)
    return got


def mixed_pairs(rng, n, len1, len2, d0=0):
    """half related along diagonal d0, half random, one homopolymer pair (ties)"""
    a, b = related_pairs(rng, n, len1, len2, int(np.clip(d0, 1 - len1, len2 - 1)))
    b[1::2] = rng.integers(0, 4, (len(b[1::2]), len2), dtype=np.uint8)
    a[-1], b[-1] = 2, 2
    return a, b


@pytest.mark.parametrize("shape", [(1, 1, 0), (1, 200, 0), (200, 1, 0), (63, 127, 64), (64, 64, 0), (65, 129, 0), (130, 130, 0)])
def test_small_shapes_under_every_mask(bg, orc, shape):
    len1, len2, d0 = shape
    rng = np.random.default_rng(len1 * 1000 + len2)
    a, b = mixed_pairs(rng, 6, len1, len2, d0)
    # diagonals: the shape's own, the corner's, and one either side
    d = np.array([d0, d0, len2 - len1, len2 - len1, d0 + 1, d0 - 1], np.int32)
    feasible = 0
    for mask in ALL_MASKS:
        for go, ge in FORMS:
            got = both_ways(bg, orc, a, b, match_matrix(2, -3), go, ge, mask, d, (shape, mask, go, ge))
            feasible += int((got[0] != NO_ALIGNMENT).sum())
    assert feasible >= 6 * 2 * 4                        # (at 1 x 200 and 200 x 1 only the masks with a free end align)


def test_every_remainder_of_the_trip_and_either_side_of_the_walk_window(bg, orc):
    rng = np.random.default_rng(2)
    seen = set()
    for length in (61, 62, 63, 64, 65, 66, 67, 68, 127, 128, 129, 191, 192, 193):
        seen.add((length + 64) % 4)
        a, b = mixed_pairs(rng, 5, length, length)
        for go, ge in FORMS:
            for mask in (0, 15, 16):
                got = both_ways(bg, orc, a, b, match_matrix(1, -1), go, ge, mask, None, (length, go, ge, mask))
            assert int(got[3].max()) >= length - 8      # a walk as long as the table: it crosses every window seam there is
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("shape", [(1000, 1024), (4096, 4100)])
def test_larger_shapes(bg, orc, shape):
    rng = np.random.default_rng(sum(shape))
    len1, len2 = shape
    a, b = mixed_pairs(rng, 5, len1, len2)               # an odd n: the second workgroup is partly empty
    d = np.array([0, 0, len2 - len1, 30, -30], np.int32)
    for go, ge in FORMS:
        for mask in (0, 10, 15, 17):
            got = both_ways(bg, orc, a, b, match_matrix(2, -3), go, ge, mask, d, (shape, go, ge, mask))
            assert int(got[3].max()) > min(shape) // 2


def test_three_alignments_of_16384_with_a_path_of_more_than_16384_steps(bg, orc):
    rng = np.random.default_rng(16384)
    a, b = related_pairs(rng, 3, 16384, 16384, 0, sub=0.05, runs=40, max_run=3)
    sm = match_matrix(2, -3)
    got = both_ways(bg, orc, a, b, sm, 5, 1, 0, None, "16384 x 16384")
    assert int(got[3].max()) > 16384 and int(got[0].min()) > 16384
    for k in range(3):
        check_path(a[k], b[k], sm, 5, 1, 0, got[0][k], got[1][k], got[2][k], got[3][k])


def test_the_origin_and_the_corner_at_the_bands_edge_and_bands_off_the_table(bg, orc):
    rng = np.random.default_rng(3)
    sm = match_matrix(2, -3)
    for d0 in (-64, -63, 64, 65):                          # (0,0) in the band for -63 .. 64
        len1, len2 = (100, 100 + d0) if d0 > 0 else (100 - d0, 100)
        a, b = related_pairs(rng, 4, len1, len2, d0)
        for mask in ALL_MASKS:
            got = both_ways(bg, orc, a, b, sm, 5, 1, mask, np.full(4, d0, np.int32), ("origin", d0, mask))
            want = -63 <= d0 <= 64 or bool(mask & (BEGIN1 if d0 < 0 else BEGIN2))
            assert ((got[0] != NO_ALIGNMENT) == want).all(), (d0, mask)
    for diff in (-65, -64, 63, 64):                        # (len1, len2) in the band for -64 .. 63
        len1, len2 = (100 - diff, 100) if diff < 0 else (100, 100 + diff)
        a, b = related_pairs(rng, 4, len1, len2, 0)
        for mask in ALL_MASKS:
            got = both_ways(bg, orc, a, b, sm, 1, 3, mask, None, ("corner", diff, mask))
            want = -64 <= diff <= 63 or bool(mask & (ANYWHERE | (END1 if diff < 0 else END2)))
            assert ((got[0] != NO_ALIGNMENT) == want).all(), (diff, mask)
    # every int32 is legal; a mixed vector in one call
    a, b = mixed_pairs(rng, 14, 70, 90)
    d = np.array([INT32_MIN, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1, 1 << 20, -(1 << 20), 90 + 65, -70 - 64, 90 + 64, -70 - 63, 90 + 63, -70 - 62,
                  0, 20], np.int64).astype(np.int32)
    for mask in (0, 3, 12, 15, 16, 19):
        got = both_ways(bg, orc, a, b, sm, 5, 1, mask, d, ("mixed vector", mask))
        assert (got[0][:8] == NO_ALIGNMENT).all() and not got[1][:8].any() and not got[3][:8].any()
        # a cell or three of the band on the table, on row 0 or column 0 only: they are a start and an end under 15 and 19 alone
        assert (got[0][8:12] != NO_ALIGNMENT).all() == (mask in (15, 19)) and (got[0][8:12] != NO_ALIGNMENT).any() == (mask in (15, 19))
    got = both_ways(bg, orc, a, b, sm, 5, 1, 15, d, "one cell")
    assert list(got[1][8]) == [0, 90, 0, 90] and list(got[1][9]) == [70, 0, 70, 0] and got[0][8] == got[0][9] == 0


def test_cells_outside_the_table_are_not_seen(bg, orc):
    """All-match sequences with len2 != len1 and gap costs 0 and 1: the sweep computes cells past the last column and the last
    row, and an E or an F would carry a value out of the table and back if those cells were not put to minus infinity."""
    for len1, len2 in ((100, 37), (37, 100), (130, 129), (129, 130), (200, 150), (150, 200), (5, 3), (3, 5)):
        for letter in (0, 3):
            a = np.full((3, len1), letter, np.uint8)
            b = np.full((3, len2), letter, np.uint8)
            d = np.array([0, len2 - len1, (len2 - len1) // 2], np.int32)
            for go, ge in ((0, 0), (1, 1), (0, 1), (1, 0)):
                for mask in (0, 5, 10, 15, 16):
                    got = both_ways(bg, orc, a, b, match_matrix(1, -1), go, ge, mask, d, (len1, len2, go, ge, mask))
                    assert (got[1][:, 0] <= len1).all() and (got[1][:, 1] <= len2).all()


def test_the_first_cell_in_row_major_order_across_lanes_with_negative_bests(bg, orc):
    """Two-letter and periodic sequences under END1, END2 and END_ANYWHERE: several candidates hold the maximum, on different
    lanes; with a matrix that is negative everywhere every score below row 1 is negative and the ties are among negative values."""
    rng = np.random.default_rng(4)
    negative = 0
    for len1, len2 in ((96, 96), (150, 131), (131, 150)):
        a = np.stack([np.arange(len1) % 2, np.arange(len1) % 3, np.arange(len1) % 4, (np.arange(len1) // 5) % 2,
                      rng.integers(0, 2, len1), np.tile([0, 0, 1], len1)[:len1]]).astype(np.uint8)
        b = np.stack([np.arange(len2) % 2, np.arange(len2) % 3, np.arange(len2) % 4, (np.arange(len2) // 5) % 2,
                      rng.integers(0, 2, len2), np.tile([0, 1, 1], len2)[:len2]]).astype(np.uint8)
        for sm, go, ge in ((match_matrix(1, -1), 1, 1), (match_matrix(-1, -2), 3, 1), (match_matrix(-2, -2), 1, 2), (match_matrix(1, 0), 0, 0),
                           (match_matrix(-1, -1), 127, 127)):
            for d in (None, np.array([3, -3, 10, -10, 0, 1], np.int32)):
                for mask in (4, 8, 12, 7, 11, 16, 19):
                    got = both_ways(bg, orc, a, b, sm, go, ge, mask, d, (len1, len2, go, ge, mask))
                    negative += int(((got[0] < 0) & (got[0] != NO_ALIGNMENT)).sum())
    assert negative > 100


def test_random_extreme_and_asymmetric_matrices(bg, orc):
    rng = np.random.default_rng(5)
    a, b = mixed_pairs(rng, 9, 300, 280)
    d = rng.integers(-70, 70, 9).astype(np.int32)
    mats = [rng.integers(-128, 128, 16).astype(np.int8) for _ in range(3)]
    mats += [np.full(16, 127, np.int8), np.full(16, -128, np.int8), match_matrix(127, -128), np.arange(-8, 8, dtype=np.int8),
             (np.arange(16, dtype=np.int8) * 7 % 23 - 11).astype(np.int8)]
    for x, sm in enumerate(mats):
        for y, (go, ge) in enumerate(((0, 0), (127, 127), (127, 0), (0, 127), (7, 2), (2, 7))):
            for mask in ((0, 15, 16) if (x + y) % 2 else (10, 5, 19)):
                both_ways(bg, orc, a, b, sm, go, ge, mask, d, (list(sm), go, ge, mask))
    # junk in bits 2 - 7 of the bases
    both_ways(bg, orc, a | 0xA4, b | 0x58, mats[0], 4, 1, 15, d, "junk bits")


def test_identities_1_and_2_every_field_equals_the_full_aligners_where_their_path_stays_in_the_band(bg, gpu):
    rng = np.random.default_rng(7)
    cases = inside = 0
    for d0, len1, len2 in ((0, 300, 330), (40, 257, 300), (-37, 300, 263)):
        a, b = related_pairs(rng, 12, len1, len2, d0)
        d = np.full(12, d0, np.int32)
        for m, x, go, ge in RELATED_PARAMS:
            sm = match_matrix(m, x)
            for mask in IDENTITY_MASKS:
                got = device_call(bg, a, b, sm, go, ge, mask, d)
                full = gpu.global_affine.global_full_affine(a, b, sm, go, ge, mask)
                linear = gpu.global_full(a, b, sm, go, mask) if go == ge else None
                assert (got[0] <= full[0]).all()
                for k in range(12):
                    cases += 1
                    if not in_band(path_from(full[2][k], full[3][k], full[1][k, 0], full[1][k, 1]), d0):
                        continue
                    inside += 1
                    one = lambda r: tuple(y[k:k + 1] for y in r)  # noqa: E731
                    assert_same(one(got), one(full), ("identity 1", d0, m, x, go, ge, mask, k))
                    if linear is not None:
                        assert_same(one(got), one(linear), ("identity 2", d0, m, x, go, mask, k))
    assert cases == 3 * 12 * 4 * 6 and inside >= 0.95 * cases, (inside, cases)


def test_identities_3_and_4_a_table_inside_the_band_and_extension(bg, gpu):
    rng = np.random.default_rng(8)
    for len1, len2, d0 in ((63, 63, 0), (40, 63, 0), (30, 50, 20)):
        a, b = mixed_pairs(rng, 8, len1, len2)
        d = np.full(8, d0, np.int32)
        for go, ge in FORMS + [(2, 2)]:
            sm = match_matrix(2, -3)
            for mask in range(16):
                assert_same(device_call(bg, a, b, sm, go, ge, mask, d), gpu.global_affine.global_full_affine(a, b, sm, go, ge, mask),
                            ("identity 3", len1, len2, go, ge, mask))
    # identity 4: mask 16 against swmi_semiglobal_full_affine where its path stays in the band
    cases = inside = 0
    a, b = related_pairs(rng, 12, 300, 330, 0)
    b[:, 170:] = rng.integers(0, 4, (12, 160), dtype=np.uint8)          # the score peaks half way
    for m, x, go, ge in RELATED_PARAMS:
        sm = match_matrix(m, x)
        got = device_call(bg, a, b, sm, go, ge, ANYWHERE)
        want = gpu.semiglobal_full_affine(a, b, sm, go, ge)
        for k in range(12):
            cases += 1
            if not in_band(path_from(want[2][k], want[3][k] - 1, want[1][k, 0], want[1][k, 1])):
                continue
            inside += 1
            assert got[0][k] == want[0][k] and tuple(got[1][k]) == tuple(want[1][k]) + (0, 0), (go, ge, k)
            assert got[3][k] >= want[3][k] - 1
            assert np.array_equal(moves_of(got[2][k], want[3][k] - 1), moves_of(want[2][k], want[3][k] - 1))
    assert inside >= 0.95 * cases, (inside, cases)


def test_paths_are_valid_without_any_oracle_and_the_band_binds(bg, gpu):
    """global_full_affine_support.check_path: the path runs from a start the mask allows to an end the mask allows and re-scores
    to the score; it stays in the band; and where the full aligner's path leaves the band the banded score is strictly lower."""
    rng = np.random.default_rng(9)
    for len1, len2, d0 in ((90, 110, 20), (130, 70, -50), (64, 64, 0), (300, 300, 0)):
        a, b = mixed_pairs(rng, 6, len1, len2, d0)
        d = np.full(6, d0, np.int32)
        for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 1, 1), (match_matrix(3, -2), 2, 6)):
            for mask in range(16):
                got = device_call(bg, a, b, sm, go, ge, mask, d)
                for k in range(6):
                    if got[0][k] == NO_ALIGNMENT:
                        continue
                    path = check_path(a[k], b[k], sm, go, ge, mask, got[0][k], got[1][k], got[2][k], got[3][k])
                    assert in_band(path, d0), (len1, len2, d0, mask, k)
    a, b = band_leaver(rng, 8)
    sm = match_matrix(2, -3)
    for mask in (0, 15):
        got = device_call(bg, a, b, sm, 5, 1, mask)
        full = gpu.global_affine.global_full_affine(a, b, sm, 5, 1, mask)
        assert (got[0] < full[0]).all() and (got[0] != NO_ALIGNMENT).all()


def test_two_device_calls_back_to_back_on_one_stream_and_the_module(bg, orc):
    rng = np.random.default_rng(10)
    a, b = mixed_pairs(rng, 8, 400, 380)
    sm = match_matrix(2, -3)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    ta, tb_ = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    outs = []
    with torch.cuda.stream(st):
        for d0, mask in ((-20, 15), (35, 2)):
            td = torch.full((8,), d0, dtype=torch.int32, device=dev)
            out = (torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros((8, 4), dtype=torch.int32, device=dev),
                   torch.zeros((8, move_words(400, 380)), dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
            bg.align_device(ta, tb_, sm, 5, 1, *out, free_ends=mask, diagonals=td, stream=st)
            outs.append((d0, mask, td, out))
    st.synchronize()
    for d0, mask, _, out in outs:
        got = (out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint64), out[3].cpu().numpy().view(np.uint32))
        assert_same(got, orc.align(a, b, sm, 5, 1, mask, np.full(8, d0, np.int32)), ("back to back", d0, mask))
    # the module's host entry, paths() and the refusals that need tensors
    d = np.array([-20, 35, 0, 0, 1, 2, 3, 600], np.int32)           # the last band misses the table
    res = bg.align(a, b, sm, 5, 1, 15, diagonals=d)
    assert_same(res, orc.align(a, b, sm, 5, 1, 15, d), "swmi.banded_global.align")
    assert_same(bg.align(a, b, sm, 5, 1, traceback=False), orc.align(a, b, sm, 5, 1, 0, None, traceback=False), "ends-only", traceback=False)
    assert res[0][7] == NO_ALIGNMENT == bg.NO_ALIGNMENT
    for k, p in enumerate(bg.paths(res)):
        assert p is None if k == 7 else np.array_equal(p, path_from(res[2][k], res[3][k], res[1][k, 0], res[1][k, 1]))
    with pytest.raises(ValueError):
        bg.align_device(ta, tb_, sm, 5, 1, outs[0][3][0], outs[0][3][1], moves=outs[0][3][2])
    ms = bg.time_device(ta, tb_, sm, 5, 1, outs[0][3][0], outs[0][3][1], free_ends=16, iters=2)
    assert ms > 0
    bg.release_workspaces()
    assert_same(bg.align(a, b, sm, 5, 1, 15, diagonals=d), res, "after release")


def test_a_host_call_of_two_slices(bg, orc):
    """slices_for finds the n: ends-only the count cap binds on a tiny shape; with a traceback the byte budget does on
    16384 x 1, whose band meets 65 rows of the table."""
    n = bg.slices_for(1 << 21, 3, 2, traceback=False)[0] + 5
    assert bg.slices_for(n, 3, 2, traceback=False) == [1 << 20, 5]
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, (n, 3), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 2), dtype=np.uint8)
    d = rng.integers(-2, 3, n).astype(np.int32)
    got = bg.align(a, b, match_matrix(2, -1), 1, 1, 0, diagonals=d, traceback=False)
    assert_same(got, orc.align(a, b, match_matrix(2, -1), 1, 1, 0, d, traceback=False), "two ends-only slices", traceback=False)
    per = bg.slices_for(1 << 20, 16384, 1)[0]
    n = per + 3
    assert bg.slices_for(n, 16384, 1) == [per, 3] and per < 4200
    a = rng.integers(0, 4, (n, 16384), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 1), dtype=np.uint8)
    d = rng.integers(-70, 5, n).astype(np.int32)
    got = bg.align(a, b, match_matrix(2, -1), 1, 1, 7, diagonals=d)          # BEGIN1 | BEGIN2 | END1: a start and an end in every band
    assert_same(got, orc.align(a, b, match_matrix(2, -1), 1, 1, 7, d), "two traceback slices")
    assert (got[0][:per] != NO_ALIGNMENT).any() and (got[0][per:] != NO_ALIGNMENT).any()
    bg.release_workspaces()


def test_the_cpp_overload(bg, orc, tmp_path):
    exe = str(tmp_path / "compat_banded_global")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_banded_global.cpp"), "-o", exe, "-L", lib, "-lswmi_banded_global", "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    rng = np.random.default_rng(12)
    a, b = mixed_pairs(rng, 5, 210, 190)
    d = np.array([0, 10, -10, 64, 300], np.int32)
    a.tofile(str(tmp_path / "a.bin"))
    b.tofile(str(tmp_path / "b.bin"))
    d.tofile(str(tmp_path / "d.bin"))
    out = subprocess.run([exe, str(tmp_path), "5", "210", "190", "2", "-3", "5", "1", "10"], stdout=subprocess.PIPE, text=True, check=True,
                         timeout=120).stdout
    want = orc.align(a, b, match_matrix(2, -3), 5, 1, 10, d)
    lines = out.strip().splitlines()
    assert len(lines) == 5
    for k, line in enumerate(lines):
        f = [int(x) for x in line.split()]
        path = path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1])
        assert f[0] == want[0][k] and f[1:5] == list(want[1][k]) and f[5] == len(path)
        assert f[6:] == [int(x) for x in path.reshape(-1)], k
    assert moves_of(want[2][0], want[3][0]).size > 100 and want[0][4] == NO_ALIGNMENT
