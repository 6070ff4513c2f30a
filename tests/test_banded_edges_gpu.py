"""The banded affine scorer (swmi_score_banded_affine) on the GPU at the edges of its band, in every kernel body: shifted
copies on diagonals -66 .. -62 and 62 .. 65, single gap runs that land on diagonals +-62 .. +-65, blocks whose diagonal run
starts or ends in a corner of the band, at lengths that cover every remainder of both kernels' trips; the table of 64 x 64
(all of it in band); the packed kernel's bias against its hand-over cost; the last score the 16-bit maxes hold; bytes 0..255;
the reference's own gapped results (F7) and the affine local aligner.  Every score bit-exact against oracle/sw_oracle.c, the
kernel instantiation asserted by name; banded_edges.py builds the inputs and test_banded_edges_cpu.py checks, without a
device, that each reaches the edge it claims and that a band off by one fails them."""
import numpy as np
import pytest

import affine_edges as ae
import banded_edges as be
from banded_edges import cross_pin, cross_pin_inputs, in_band
from conftest import match_matrix
from local_affine_support import AFFINE_GAPS
from local_support import load_f7, random_matrix

pytestmark = pytest.mark.gpu

RAN = {}                                                  # family -> kernel instantiations its cases ran, by name


def _score(gpu, a, b, sm, go, ge, want_kernel=None):
    """one launch, the kernel it runs asserted by name"""
    name, per = gpu.banded_affine_kernel_for(a.shape[1], sm, go, ge)
    assert per == (2 if "_pk_" in name else 1)
    if want_kernel is not None:
        assert name == want_kernel, (name, want_kernel, a.shape[1], go, ge)
    return gpu.score_banded_affine(a, b, sm, go, ge), name


def _run_case(gpu, oracle, case):
    """The case's pairs each next to an unrelated pair in an odd batch, against the oracle and the hand values; then pairs
    2k and 2k + 1 exchanged: the scores exchange (the packed kernel's X and Y halves do not leak into each other)."""
    a, b, at = be.mixed_batch(case)
    go, ge = case.gap_open, case.gap_ext
    got, name = _score(gpu, a, b, case.sm, go, ge, case.kernel)
    want = oracle.banded_affine(a, b, case.sm, go, ge)
    for k, i in enumerate(at):
        assert got[i] == want[i], (case.what(k), "gpu %d oracle %d" % (got[i], want[i]))
        if case.want[k] >= 0:
            assert got[i] == case.want[k], (case.what(k), "gpu %d by hand %d" % (got[i], case.want[k]))
        if case.below[k] >= 0:
            assert got[i] < case.below[k], (case.what(k), "gpu %d not below %d" % (got[i], case.below[k]))
    assert np.array_equal(got, want), (case.what(), "unrelated neighbours", np.nonzero(got != want)[0])
    assert got[-1] == got[0], (case.what(0), "the odd batch's last pair")
    a2, perm = be.swap_halves(a)
    got2, _ = _score(gpu, a2, b[perm], case.sm, go, ge, case.kernel)
    assert np.array_equal(got2, got[perm]), (case.what(), "halves exchanged", np.nonzero(got2 != got[perm])[0])
    return name


def _run_family(gpu, oracle, family):
    names = RAN.setdefault(family, set())
    for case in be.FAMILIES[family]():
        names.add(_run_case(gpu, oracle, case))


@pytest.mark.parametrize("family", list(be.FAMILIES))
def test_constructed_edges_in_every_body(gpu, oracle, family):
    """shift: copies on the band's last and first-outside diagonals; gap_run: one gap run that lands there; corner: the
    first and last iterations of lanes 0, 32 and 63 and the cells past either sequence's end.  Each in the packed, the
    16-bit and the plain body, open >= extend and open < extend, at every remainder of the trips."""
    _run_family(gpu, oracle, family)
    assert RAN[family] == set(be.KERNELS), family


def test_one_input_through_three_bodies_scales_with_its_parameters(gpu, oracle):
    """Local alignment scores are homogeneous: (sm, open, extend) times k gives the score times k.  (1, -2 | 3, 1) and
    (1, -2 | 1, 3) times 1, 31 and 40 run the packed, the 16-bit and the plain body on the SAME sequences."""
    for length in (1024, 1057):
        rng = np.random.default_rng(length)
        ra, rb = be.related(rng, 9, length, indel=0.01)
        shift = be.shift_case(length, 1, -2, 3, 1)
        run = be.gap_run_case(length, 1, -2, 3, 1, hand=False)
        a = np.concatenate([shift.a, run.a, ra])
        b = np.concatenate([shift.b, run.b, rb])
        labels = shift.labels + run.labels + ["related %d" % k for k in range(len(ra))]
        assert len(a) % 2 == 0
        for go, ge in ((3, 1), (1, 3)):
            oge = int(go >= ge)
            got = {}
            for k, kernel in ((1, "sw_banded_affine_pk_kernel<%d>" % oge), (31, "sw_banded_affine_kernel<%d,1>" % oge),
                              (40, "sw_banded_affine_kernel<%d,0>" % oge)):
                sm = match_matrix(k, -2 * k)
                got[k], _ = _score(gpu, a, b, sm, go * k, ge * k, kernel)
                want = oracle.banded_affine(a, b, sm, go * k, ge * k)
                bad = np.nonzero(got[k] != want)[0]
                assert not len(bad), (length, kernel, [(labels[i], int(got[k][i]), int(want[i])) for i in bad[:4]])
            assert np.array_equal(got[31], 31 * got[1]) and np.array_equal(got[40], 40 * got[1]), (length, go, ge)
            inside = [i for i, s in enumerate(be.SHIFTS) if be.LO <= s <= be.HI]
            assert list(got[1][inside]) == [length - abs(be.SHIFTS[i]) for i in inside]


def test_at_len_64_the_band_is_the_whole_table(gpu, oracle):
    """the banded score is the unbanded local Gotoh score of affine_edges.py's whole-table formulation, for any input"""
    rng = np.random.default_rng(64)
    a, b = be.related(rng, 11, 64, sub=0.1, indel=0.05)
    a[6:] = rng.integers(0, 4, (5, 64), dtype=np.uint8)
    a[9], b[9] = be.shifted_pair(rng, 64, -30)
    a[10], b[10] = be.shifted_pair(rng, 64, 31)
    for sm in (match_matrix(2, -3), match_matrix(1, -1), random_matrix(), match_matrix(3, 1)):
        for go, ge in AFFINE_GAPS:
            got, _ = _score(gpu, a, b, sm, go, ge, "sw_banded_affine_pk_kernel<%d>" % (go >= ge))
            assert list(got) == [ae.numpy_affine(a[k], b[k], sm, go, ge, local=True)[0] for k in range(len(a))], (sm, go, ge)
            assert np.array_equal(got, oracle.banded_affine(a, b, sm, go, ge)), (sm, go, ge)


@pytest.mark.parametrize("length", [64, 65, 66, 67, 79, 80, 81])
def test_short_lengths_random_and_related(gpu, oracle, length):
    """the lengths the shifted copies and gap runs leave out: the band reaches (nearly) every cell, what is under test is
    the trips of one after len // 16 trips of 16, and the pad rows and columns that follow at once"""
    rng = np.random.default_rng(length)
    a, b = be.related(rng, 37, length, sub=0.1, indel=0.05)
    a[30:] = rng.integers(0, 4, (7, length), dtype=np.uint8)
    a[0], b[0] = be.shifted_pair(rng, length, length - 64)       # the copy ends in the band's corner or next to it
    a[1], b[1] = be.shifted_pair(rng, length, 63 - length)
    for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(2, -3), 1, 4), (match_matrix(3, 1), 2, 2), (match_matrix(127, -128), 127, 0),
                       (match_matrix(127, -128), 0, 127), (random_matrix(), 0, 0)):
        got, _ = _score(gpu, a, b, sm, go, ge, "sw_banded_affine_pk_kernel<%d>" % (go >= ge))
        want = oracle.banded_affine(a, b, sm, go, ge)
        assert np.array_equal(got, want), (length, go, ge, np.nonzero(got != want)[0])


@pytest.mark.parametrize("length", [333, 1024])
def test_packed_kernel_bias_against_cost(gpu, oracle, length):
    """B = max(0, -min s) in {cost - 1, cost, cost + 1}: the addend B - cost that a value gains across an iteration is a
    plain per-half number for B >= cost and a two's-complement pair whose low half must carry for B < cost; related pairs
    with real gap runs, the constructed gap runs and the shifted copies"""
    rng = np.random.default_rng(length)
    ra, rb = be.related(rng, 12, length, sub=0.05, indel=0.03)
    for sm, go, ge, bias, cost in be.bias_cost_params():
        match, mismatch = int(sm[0]), int(sm[1])
        shift = be.shift_case(length, match, mismatch, go, ge)
        run = be.gap_run_case(length, match, mismatch, go, ge, hand=False) if length in be.FREE_GAP_LENGTHS else None
        a = np.concatenate([shift.a, ra] + ([run.a] if run else []))
        b = np.concatenate([shift.b, rb] + ([run.b] if run else []))
        got, _ = _score(gpu, a, b, sm, go, ge, "sw_banded_affine_pk_kernel<%d>" % (go >= ge))
        want = oracle.banded_affine(a, b, sm, go, ge)
        assert np.array_equal(got, want), ("B %d cost %d" % (bias, cost), length, go, ge, np.nonzero(got != want)[0], got[:9], want[:9])
        if mismatch < 0 and min(go, ge) > 0:
            inside = [i for i, s in enumerate(be.SHIFTS) if be.LO <= s <= be.HI]
            assert list(got[inside]) == [match * (length - abs(be.SHIFTS[i])) for i in inside], (bias, cost)


def test_the_16_bit_bodies_at_the_end_of_their_domain(gpu, oracle):
    """len 1057 x match 31 = 32767, the last H a v_max_i16 holds: an identical pair scores exactly that; 1024 x 32 = 32768
    runs the plain cell.  Related pairs with gaps alongside."""
    for length, match, i16, top in ((1057, 31, 1, 32767), (1024, 32, 0, 32768)):
        rng = np.random.default_rng(match)
        a, b = be.related(rng, 21, length, sub=0.02, indel=0.01)
        b[0] = a[0]                                       # identical
        a[1] = 3; b[1] = 3                                # identical homopolymer: every diagonal of the band climbs
        a[2], b[2] = be.shifted_pair(rng, length, 1)
        for mismatch, go, ge in ((-40, 5, 1), (-40, 1, 4), (-128, 127, 127), (-1, 0, 0), (-40, 0, 127)):
            sm = match_matrix(match, mismatch)
            got, _ = _score(gpu, a, b, sm, go, ge, "sw_banded_affine_kernel<%d,%d>" % (go >= ge, i16))
            want = oracle.banded_affine(a, b, sm, go, ge)
            assert np.array_equal(got, want), (length, match, mismatch, go, ge, np.nonzero(got != want)[0], got[:3], want[:3])
            assert got[0] == top and got[1] == top and got[2] == match * (length - 1)


def test_bytes_that_are_no_base_count_by_their_low_two_bits(gpu, oracle):
    """the scorer masks with & 3 (the semi-global aligner does not): in every body"""
    rng = np.random.default_rng(255)
    a, b = be.related(rng, 9, 1024)
    seen = set()
    for k in (1, 31, 40):
        for go, ge in ((3, 1), (1, 3)):
            sm = match_matrix(k, -2 * k)
            want = oracle.banded_affine(a, b, sm, go * k, ge * k)
            got, name = _score(gpu, a | 0xFC, b | 0x54, sm, go * k, ge * k)
            seen.add(name)
            assert np.array_equal(got, want), name
            assert np.array_equal(gpu.score_banded_affine(rng.integers(0, 64, a.shape, dtype=np.uint8) << 2 | a, b, sm, go * k, ge * k), want), name
    assert seen == set(be.KERNELS)


def test_the_reference_results_of_f7(gpu):
    """the 28 alignments of two 128-mers of F7 (SmithWaterman_111_long at (1, -1, 1), 16 of them gapped, all paths in band):
    open = extend = 1 gives the reference's score, with the sequences in either order"""
    f7 = [v for v in load_f7() if v["len1"] == 128]
    assert len(f7) == 28 and sum(in_band(v["path"], -63, 63) for v in f7) == 28
    a = np.stack([v["seq1"] for v in f7])
    b = np.stack([v["seq2"] for v in f7])
    want = np.array([v["score"] for v in f7], np.int32)
    for x, y in ((a, b), (b, a), (a[:27], b[:27])):
        got, _ = _score(gpu, x, y, match_matrix(1, -1), 1, 1, "sw_banded_affine_pk_kernel<1>")
        assert np.array_equal(got, want[:len(x)]), [(f7[k]["kind"], int(got[k]), int(want[k])) for k in np.nonzero(got != want[:len(x)])[0]]


def test_banded_scorer_against_the_affine_local_aligner(gpu, oracle):
    """two independent kernels tied together at len 128: swmi_score_banded_affine <= swmi_local_align_affine, equal wherever
    the aligner's path stays in band (at least 90 % of the cases), strictly lower somewhere; and the scorer against its
    oracle on the same inputs"""
    a, b = cross_pin_inputs()

    def banded(sm, go, ge):
        got = gpu.score_banded_affine(a, b, sm, go, ge)
        assert np.array_equal(got, oracle.banded_affine(a, b, sm, go, ge)), (sm, go, ge)
        return got
    cases, inside, lower = cross_pin(a, b, banded, lambda sm, go, ge: gpu.local_align_affine(a, b, sm, go, ge), gpu.local_expand_moves)
    assert cases == 3360 and inside >= 0.9 * cases and lower >= 1, (cases, inside, lower)


def test_zz_every_kernel_body_ran_every_family(gpu, oracle):
    """The closing assertion: each of the six instantiations ran the shifted copies, the gap runs and the corner blocks, by
    name.  A change of the choice function that drops a body from a family fails here.  (A family that has not run in this
    process -- this test selected alone -- is run now.)"""
    for family in be.FAMILIES:
        if family not in RAN:
            _run_family(gpu, oracle, family)
        assert sorted(RAN[family]) == sorted(be.KERNELS), (family, sorted(set(be.KERNELS) - RAN[family]))
