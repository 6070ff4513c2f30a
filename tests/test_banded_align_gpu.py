"""The banded local aligner on the GPU (libswmi_banded.so, include/swmi_banded.h, swmi.banded): every field and every move
against the C restatement tests/native/banded_align_oracle.c, with a traceback and ends-only, in both template forms of the
kernel (open >= extend and open < extend); the three identities that tie it to merged code; path validity without any
oracle; the host entry in two slices, the Python module and the C++ overload.  Every comparison is exact integer equality.

The kernel sweeps whole trips of 4 iterations, i_hi - i_lo + 64 of them rounded up, so the shapes 64 .. 67 squared run every
remainder of the trip; it stages no sequence (every lane loads its own bases a trip ahead), so there is no staging chunk;
its walk window holds 64 iterations, which the lengths 1, 2, 63, 64, 65 stand either side of."""
import os
import subprocess

import numpy as np
import pytest
import torch

import banded_edges
from banded_align_support import (INT32_MAX, INT32_MIN, RELATED_DIAGONALS, RELATED_PARAMS, BandedOracle, assert_same, check_path, in_band,
                                  move_words, moves_of, numpy_band_table, path_from, related_pairs)
from conftest import PKG, ROOT, match_matrix

pytestmark = pytest.mark.gpu

FORMS = [(5, 1), (1, 3)]                    # open >= extend, open < extend: the two instantiations
SMALL = [1, 2, 63, 64, 65, 127, 128, 129, 130]


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return BandedOracle(tmp_path_factory.mktemp("banded_align_oracle"))


@pytest.fixture(scope="module")
def bd(swmi_mod):
    swmi_mod.banded.load()
    return swmi_mod.banded


def device_call(bd, a, b, sm, go, ge, diagonals=None, traceback=True, stream=None):
    """swmi.banded.local_device on fresh tensors; the result as numpy arrays in the host entry's layout."""
    n, len1 = a.shape
    len2 = b.shape[1]
    dev = torch.device("cuda:0")
    ta, tb_ = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    td = None if diagonals is None else torch.from_numpy(np.ascontiguousarray(diagonals, np.int32)).to(dev)
    scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ends = torch.full((n, 4), -7, dtype=torch.int32, device=dev)
    moves = torch.zeros((n, move_words(len1, len2)), dtype=torch.int64, device=dev) if traceback else None
    steps = torch.full((n,), -7, dtype=torch.int32, device=dev) if traceback else None
    bd.local_device(ta, tb_, sm, go, ge, scores, ends, moves, steps, diagonals=td, stream=stream)
    torch.cuda.synchronize()
    return (scores.cpu().numpy(), ends.cpu().numpy(), moves.cpu().numpy().view(np.uint64) if traceback else None,
            steps.cpu().numpy().view(np.uint32) if traceback else None)


def both_ways(bd, orc, a, b, sm, go, ge, diagonals, what):
    """with a traceback and ends-only against the restatement; returns the traceback result"""
    want = orc.align(a, b, sm, go, ge, diagonals)
    got = device_call(bd, a, b, sm, go, ge, diagonals)
    assert_same(got, want, what)
    eo = device_call(bd, a, b, sm, go, ge, diagonals, traceback=False)
    assert_same(eo, orc.align(a, b, sm, go, ge, diagonals, traceback=False), (what, "ends-only"), traceback=False)
    return got


def mixed_pairs(rng, n, len1, len2, d0=0):
    """half related along diagonal d0, half random, one homopolymer pair (ties)"""
    a, b = related_pairs(rng, n, len1, len2, int(np.clip(d0, 1 - len1, len2 - 1)))
    b[1::2] = rng.integers(0, 4, (len(b[1::2]), len2), dtype=np.uint8)
    a[-1], b[-1] = 2, 2
    return a, b


def test_small_shapes_where_the_band_is_wider_equal_or_narrower_than_the_table(bd, orc):
    rng = np.random.default_rng(1)
    sm = match_matrix(2, -3)
    for len1 in SMALL:
        for len2 in SMALL:
            a, b = mixed_pairs(rng, 6, len1, len2)
            d = np.array([0, 0, len2 - len1, len2 - len1, 1, 0], np.int32)
            for go, ge in FORMS:
                both_ways(bd, orc, a, b, sm, go, ge, d, (len1, len2, go, ge))


def test_every_remainder_of_the_trip_and_either_side_of_the_walk_window(bd, orc):
    rng = np.random.default_rng(2)
    seen = set()
    for length in (61, 62, 63, 64, 65, 66, 67, 191, 192, 193):
        seen.add((length + 63) % 4)
        a, b = mixed_pairs(rng, 5, length, length)
        for go, ge in FORMS:
            got = both_ways(bd, orc, a, b, match_matrix(1, -1), go, ge, None, (length, go, ge))
            assert int(got[3].max()) >= length - 8          # a walk as long as the table: it crosses every window seam there is
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("shape", [(1100, 900), (900, 1100), (1792, 1792)])
def test_larger_shapes(bd, orc, shape):
    rng = np.random.default_rng(sum(shape))
    len1, len2 = shape
    a, b = mixed_pairs(rng, 7, len1, len2)               # an odd n: the second workgroup is partly empty
    d = np.array([0, 0, len2 - len1, len2 - len1, 30, -30, 0], np.int32)
    for go, ge in FORMS:
        got = both_ways(bd, orc, a, b, match_matrix(2, -3), go, ge, d, (shape, go, ge))
        assert int(got[3].max()) > min(shape) // 2


def test_three_alignments_of_16384_with_a_path_of_more_than_16384_steps(bd, orc):
    rng = np.random.default_rng(16384)
    a, b = related_pairs(rng, 3, 16384, 16384, 0, sub=0.05, runs=40, max_run=3)
    sm = match_matrix(2, -3)
    got = both_ways(bd, orc, a, b, sm, 5, 1, None, "16384 x 16384")
    assert int(got[3].max()) > 16384 and int(got[0].min()) > 16384
    for k in range(3):
        check_path(a[k], b[k], sm, 5, 1, 0, got[0][k], got[1][k], got[2][k], got[3][k])


def test_diagonals_at_small_shapes(bd, orc):
    rng = np.random.default_rng(3)
    for len1, len2 in ((70, 90), (130, 129), (1, 130), (129, 1), (64, 64)):
        values = [0, 1, -1, 63, -63, 64, -64, 65, -65, len2 - len1,
                  len2 + 63, -len1 - 62,                  # one cell of the band on the table: (1, len2), (len1, 1)
                  len2 + 62, -len1 - 61,                  # two diagonals of it
                  len2 + 64, -len1 - 63,                  # nothing
                  INT32_MIN, INT32_MAX, INT32_MIN + 1, INT32_MAX - 1, 1 << 20, -(1 << 20)]
        for d0 in values:                                  # every alignment of a call on one diagonal, pairs related along it
            a, b = mixed_pairs(rng, 4, len1, len2, int(np.clip(d0, -(1 << 20), 1 << 20)))
            d = np.full(4, d0, np.int64).astype(np.int32)
            for go, ge in FORMS:
                got = both_ways(bd, orc, a, b, match_matrix(2, -3), go, ge, d, (len1, len2, d0, go, ge))
                if d0 in (len2 + 64, -len1 - 63, INT32_MIN, INT32_MAX, 1 << 20):
                    assert not got[0].any() and not got[1].any() and not got[3].any()
        # a mixed vector within one call, all-match sequences: the score says how much of the band is on the table
        d = np.array(values + [5, -5], np.int32)
        a = np.zeros((len(d), len1), np.uint8)
        b = np.zeros((len(d), len2), np.uint8)
        got = both_ways(bd, orc, a, b, match_matrix(1, -1), 0, 0, d, (len1, len2, "mixed vector"))
        assert got[0][values.index(len2 + 63)] == 1 and got[0][values.index(-len1 - 62)] == 1
        assert list(got[1][values.index(len2 + 63)][:2]) == [1, len2] and list(got[1][values.index(-len1 - 62)][:2]) == [len1, 1]


def test_cells_outside_the_table_are_not_seen(bd, orc):
    """All-match sequences with len2 < len1 and len1 < len2: the best cell lies in the last column or the last row, the cells
    past it are computed by the sweep, and with gap costs 0 and 1 an E or an F carries the best value out of the table."""
    for len1, len2 in ((100, 37), (37, 100), (130, 129), (129, 130), (200, 64), (64, 200), (5, 3), (3, 5)):
        for letter in (0, 3):
            a = np.full((3, len1), letter, np.uint8)
            b = np.full((3, len2), letter, np.uint8)
            d = np.array([0, len2 - len1, (len2 - len1) // 2], np.int32)
            for go, ge in ((0, 0), (1, 1), (0, 1), (1, 0)):
                for sm in (match_matrix(1, -1), match_matrix(3, 1)):
                    got = both_ways(bd, orc, a, b, sm, go, ge, d, (len1, len2, go, ge))
                    assert (got[1][:, 0] == len1).any() or (got[1][:, 1] == len2).any()
                    assert (got[1][:, 0] <= len1).all() and (got[1][:, 1] <= len2).all()


def test_the_first_cell_in_row_major_order_across_lanes(bd, orc):
    """Two-letter and periodic sequences: several cells hold the maximum, on different lanes at one iteration."""
    rng = np.random.default_rng(4)
    for len1, len2 in ((96, 96), (150, 131), (131, 150)):
        a = np.stack([np.arange(len1) % 2, np.arange(len1) % 3, np.arange(len1) % 4, (np.arange(len1) // 5) % 2,
                      rng.integers(0, 2, len1), np.tile([0, 0, 1], len1)[:len1]]).astype(np.uint8)
        b = np.stack([np.arange(len2) % 2, np.arange(len2) % 3, np.arange(len2) % 4, (np.arange(len2) // 5) % 2,
                      rng.integers(0, 2, len2), np.tile([0, 1, 1], len2)[:len2]]).astype(np.uint8)
        for sm, go, ge in ((match_matrix(1, -1), 1, 1), (match_matrix(2, -120), 127, 127), (match_matrix(1, -1), 1, 2), (match_matrix(1, 0), 0, 0)):
            for d in (None, np.array([3, -3, 10, -10, 0, 1], np.int32)):
                both_ways(bd, orc, a, b, sm, go, ge, d, (len1, len2, go, ge))
    # a block that matches at several places: priced-out gaps, the maxima are exact ties
    a = np.zeros((1, 120), np.uint8)
    b = np.ones((1, 120), np.uint8)
    for at in (3, 40, 77):
        a[0, at:at + 8] = banded_edges.BLOCK
    for at in (20, 50, 99):
        b[0, at:at + 8] = banded_edges.BLOCK
    got = both_ways(bd, orc, a, b, match_matrix(5, -30), 127, 127, None, "tied blocks")
    assert got[0][0] == 40 and list(got[1][0]) == [11, 28, 3, 20]


def test_band_edges_with_the_families_of_banded_edges(bd, orc):
    cases = [banded_edges.shift_case(128, 2, -3, go, ge) for go, ge in banded_edges.SHIFT_GAPS]
    cases += [banded_edges.shift_case(333, 2, -3, 127, 127), banded_edges.shift_case(333, 2, -3, 126, 127)]
    cases += [banded_edges.gap_run_case(333, 2, -3, go, ge) for go, ge in banded_edges.HAND_GAP_SETS]
    cases += [banded_edges.gap_run_case(1024, 2, -3, go, ge) for go, ge in banded_edges.GAP_SETS]
    cases += [banded_edges.corner_case(length, 5, -30, go, ge) for length in (79, 128, 333) for go, ge in banded_edges.SHIFT_GAPS]
    for c in cases:
        got = both_ways(bd, orc, c.a, c.b, c.sm, c.gap_open, c.gap_ext, None, c.what())
        hand = c.want >= 0
        assert np.array_equal(got[0][hand], c.want[hand]), c.what()
        bound = c.below >= 0
        assert (got[0][bound] < c.below[bound]).all(), c.what()


def test_random_extreme_and_asymmetric_matrices(bd, orc):
    rng = np.random.default_rng(5)
    a, b = mixed_pairs(rng, 9, 300, 280)
    d = rng.integers(-70, 70, 9).astype(np.int32)
    mats = [rng.integers(-128, 128, 16).astype(np.int8) for _ in range(3)]
    mats += [np.full(16, 127, np.int8), np.full(16, -128, np.int8), match_matrix(127, -128), np.arange(-8, 8, dtype=np.int8),
             (np.arange(16, dtype=np.int8) * 7 % 23 - 11).astype(np.int8)]
    for sm in mats:
        for go, ge in ((0, 0), (127, 127), (127, 0), (0, 127), (7, 2), (2, 7)):
            both_ways(bd, orc, a, b, sm, go, ge, d, (list(sm), go, ge))
    # junk in bits 2 - 7 of the bases
    both_ways(bd, orc, a | 0xA4, b | 0x58, mats[0], 4, 1, d, "junk bits")


def test_identity_1_scores_equal_the_banded_scorer(bd, gpu):
    """len1 = len2 in [64, 1792], diagonals NULL: scores equal swmi_score_banded_affine_device, under parameters that select
    each of its six kernels."""
    rng = np.random.default_rng(6)
    seen = set()
    dev = torch.device("cuda:0")
    for length in (64, 81, 128, 333, 1024, 1792):
        a, b = banded_edges.related(rng, 16, length)
        b[::4] = rng.integers(0, 4, (4, length), dtype=np.uint8)
        ta, tb_ = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        out = torch.zeros(16, dtype=torch.int32, device=dev)
        for body in banded_edges.BODIES:
            if body != "pk" and length not in banded_edges.BODY_LENGTHS:
                continue                                    # below len 259 no int8 matrix leaves the packed kernel's domain
            for go, ge in ((5, 1), (1, 4)):
                m = banded_edges.match_for(length, body, 2)
                sm = match_matrix(m, max(-128, -(3 * m + 1) // 2))
                if banded_edges.body_of(length, sm, go, ge) != body:
                    continue
                name = gpu.banded_affine_kernel_for(length, sm, go, ge)[0]
                assert name == banded_edges.kernel_name(length, sm, go, ge)
                seen.add(name)
                gpu.score_banded_affine_device(ta.data_ptr(), tb_.data_ptr(), 16, length, sm, go, ge, out.data_ptr())
                torch.cuda.synchronize()
                got = device_call(bd, a, b, sm, go, ge, None, traceback=False)
                assert np.array_equal(got[0], out.cpu().numpy()), (length, name)
    assert seen == set(banded_edges.KERNELS)


def test_identities_2_and_3_every_field_equals_the_full_aligners_where_their_path_stays_in_the_band(bd, gpu):
    rng = np.random.default_rng(7)
    cases = inside = 0
    for d0 in RELATED_DIAGONALS:
        a, b = related_pairs(rng, 24, 300, 300, d0)
        d = np.full(24, d0, np.int32)
        for m, x, go, ge in RELATED_PARAMS:
            sm = match_matrix(m, x)
            got = device_call(bd, a, b, sm, go, ge, d)
            full = gpu.local_full_affine(a, b, sm, go, ge)
            linear = gpu.local_full(a, b, sm, go) if go == ge else None
            for k in range(24):
                cases += 1
                assert got[0][k] <= full[0][k]
                path = path_from(full[2][k], full[3][k], full[1][k, 0], full[1][k, 1])
                if not in_band(path[1:], d0):
                    continue
                inside += 1
                one = lambda r: tuple(x[k:k + 1] for x in r)  # noqa: E731
                assert_same(one(got), one(full), ("identity 2", d0, m, x, go, ge, k))
                if linear is not None:
                    assert_same(one(got), one(linear), ("identity 3", d0, m, x, go, k))
    assert cases == 288 and inside >= 0.95 * cases, (inside, cases)


def test_paths_are_valid_without_any_oracle(bd):
    """The expanded path re-scored by numpy gives the score, starts at a cell with H = 0 of an independent numpy table, ends at
    the first maximum of that table, and stays in the band."""
    rng = np.random.default_rng(8)
    for len1, len2, d0 in ((90, 110, 20), (130, 70, -50), (64, 64, 0)):
        a, b = mixed_pairs(rng, 6, len1, len2, d0)
        d = np.full(6, d0, np.int32)
        for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 1, 1), (match_matrix(3, -2), 2, 6)):
            got = device_call(bd, a, b, sm, go, ge, d)
            for k in range(6):
                check_path(a[k], b[k], sm, go, ge, d0, got[0][k], got[1][k], got[2][k], got[3][k])
                H = numpy_band_table(a[k], b[k], sm, go, ge, d0)
                assert H.max() == got[0][k]
                first = divmod(int(np.argmax(H.reshape(-1))), len2 + 1) if H.max() > 0 else (0, 0)
                assert first == (got[1][k, 0], got[1][k, 1])
                assert H[got[1][k, 2], got[1][k, 3]] == 0


def test_two_device_calls_back_to_back_on_one_stream_and_the_module(bd, orc):
    rng = np.random.default_rng(9)
    a, b = mixed_pairs(rng, 8, 400, 380)
    sm = match_matrix(2, -3)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    ta, tb_ = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    outs = []
    with torch.cuda.stream(st):
        for d0 in (-20, 35):
            td = torch.full((8,), d0, dtype=torch.int32, device=dev)
            out = (torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros((8, 4), dtype=torch.int32, device=dev),
                   torch.zeros((8, move_words(400, 380)), dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
            bd.local_device(ta, tb_, sm, 5, 1, *out, diagonals=td, stream=st)
            outs.append((d0, td, out))
    st.synchronize()
    for d0, _, out in outs:
        got = (out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy().view(np.uint64), out[3].cpu().numpy().view(np.uint32))
        assert_same(got, orc.align(a, b, sm, 5, 1, np.full(8, d0, np.int32)), ("back to back", d0))
    # the module's host entry, paths() and the refusals that need tensors
    d = np.array([-20, 35, 0, 0, 1, 2, 3, 4], np.int32)
    res = bd.local(a, b, sm, 5, 1, diagonals=d)
    assert_same(res, orc.align(a, b, sm, 5, 1, d), "swmi.banded.local")
    assert_same(bd.local(a, b, sm, 5, 1, traceback=False), orc.align(a, b, sm, 5, 1, None, traceback=False), "ends-only", traceback=False)
    for k, p in enumerate(bd.paths(res)):
        assert np.array_equal(p, path_from(res[2][k], res[3][k], res[1][k, 0], res[1][k, 1]))
    with pytest.raises(ValueError):
        bd.local_device(ta, tb_, sm, 5, 1, outs[0][2][0], outs[0][2][1], moves=outs[0][2][2])
    with pytest.raises(ValueError):
        bd.local(a, b, sm, 5, 1, diagonals=d[:3])
    ms = bd.time_device(ta, tb_, sm, 5, 1, outs[0][2][0], outs[0][2][1], iters=2)
    assert ms > 0
    bd.release_workspaces()
    assert_same(bd.local(a, b, sm, 5, 1, diagonals=d), res, "after release")


def test_a_host_call_of_two_slices(bd, orc):
    """slices_for finds the n: ends-only the count cap binds on a tiny shape; with a traceback the byte budget does on
    16384 x 1, whose band meets 65 rows of the table."""
    n = bd.slices_for(1 << 21, 3, 2, traceback=False)[0] + 5
    assert bd.slices_for(n, 3, 2, traceback=False) == [1 << 20, 5]
    rng = np.random.default_rng(10)
    a = rng.integers(0, 4, (n, 3), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 2), dtype=np.uint8)
    d = rng.integers(-2, 3, n).astype(np.int32)
    got = bd.local(a, b, match_matrix(2, -1), 1, 1, diagonals=d, traceback=False)
    assert_same(got, orc.align(a, b, match_matrix(2, -1), 1, 1, d, traceback=False), "two ends-only slices", traceback=False)
    per = bd.slices_for(1 << 20, 16384, 1)[0]
    n = per + 3
    assert bd.slices_for(n, 16384, 1) == [per, 3] and per < 4200
    a = rng.integers(0, 4, (n, 16384), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 1), dtype=np.uint8)
    d = rng.integers(-70, 5, n).astype(np.int32)
    got = bd.local(a, b, match_matrix(2, -1), 1, 1, diagonals=d)
    assert_same(got, orc.align(a, b, match_matrix(2, -1), 1, 1, d), "two traceback slices")
    assert got[0][:per].any() and got[0][per:].any()
    bd.release_workspaces()


def test_the_cpp_overload(bd, orc, tmp_path):
    exe = str(tmp_path / "compat_banded")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "compat_banded.cpp"),
                            "-o", exe, "-L", lib, "-lswmi_banded", "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    rng = np.random.default_rng(11)
    a, b = mixed_pairs(rng, 5, 210, 190)
    d = np.array([0, 10, -10, 64, -20], np.int32)
    a.tofile(str(tmp_path / "a.bin"))
    b.tofile(str(tmp_path / "b.bin"))
    d.tofile(str(tmp_path / "d.bin"))
    out = subprocess.run([exe, str(tmp_path), "5", "210", "190", "2", "-3", "5", "1"], stdout=subprocess.PIPE, text=True, check=True, timeout=120).stdout
    want = orc.align(a, b, match_matrix(2, -3), 5, 1, d)
    lines = out.strip().splitlines()
    assert len(lines) == 5
    for k, line in enumerate(lines):
        f = [int(x) for x in line.split()]
        path = path_from(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1])
        assert f[0] == want[0][k] and f[1:5] == list(want[1][k]) and f[5] == len(path)
        assert f[6:] == [int(x) for x in path.reshape(-1)], k
    assert moves_of(want[2][0], want[3][0]).size > 100
