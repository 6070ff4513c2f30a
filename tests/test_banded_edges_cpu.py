"""The generators of banded_edges.py checked without a device: every score a generator claims by hand is what the C oracle
(oracle/sw_oracle.c) and the numpy formulations give, every input placed one diagonal outside the band scores strictly
below what it would score inside, and -- the teeth -- a band that is off by one on either side, in either direction,
gets at least one case of every length wrong.  Two pins for the oracle itself: the reference's own SmithWaterman_111_long
results (fixture F7, 16 of them gapped) and the affine local aligner's C restatement wherever its optimal path stays in the
band.  test_banded_edges_gpu.py sends the same cases through every kernel body."""
import numpy as np
import pytest

import affine_edges as ae
import banded_edges as be
from conftest import match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle
from banded_edges import cross_pin, cross_pin_inputs, in_band
from local_support import load_f7, move_words, random_matrix


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


def test_lengths_and_bodies_the_generators_cover(swmi_mod):
    """every remainder of both kernels' trips, both ends of the domain; the lengths a family leaves out are listed, not
    dropped; each family reaches all six kernel instantiations, and the body a case names (the formula of DESIGN.md 9,
    restated in banded_edges.body_of) is the one the library's choice function answers"""
    assert {l % 4 for l in be.LENGTHS} == {0, 1, 2, 3} and {0, 1, 15} <= {l % 16 for l in be.LENGTHS}
    assert {64, 65, 66, 67, 79, 80, 81, 1057, 1791, 1792} <= set(be.LENGTHS) and min(be.LENGTHS) == 64 and max(be.LENGTHS) == 1792
    assert {l % 4 for l in be.BODY_LENGTHS} == {0, 1, 2, 3} and {0, 1, 15} <= {l % 16 for l in be.BODY_LENGTHS + [79, 81]}
    for family, make in be.FAMILIES.items():
        cases = make()
        assert {c.kernel for c in cases} == set(be.KERNELS), family
        for c in cases:
            assert swmi_mod.banded_affine_kernel_for(c.length, c.sm, c.gap_open, c.gap_ext)[0] == c.kernel, c
        for kernel in be.KERNELS:                        # every remainder of the trip, in every instantiation
            lengths = {c.length for c in cases if c.kernel == kernel}
            want = {0, 1, 2, 3} if family != "gap_run" or "<1" in kernel else {0, 1, 3}     # (1, 4) from len 1024 on only
            assert want <= {l % 4 for l in lengths}, (family, kernel, sorted(lengths))
    every = [c for make in be.FAMILIES.values() for c in make()]
    for kernel in be.KERNELS:
        assert {0, 1, 2, 3} == {c.length % 4 for c in every if c.kernel == kernel}, kernel
    assert {0, 1, 15} <= {c.length % 16 for c in every if "_pk_" in c.kernel}


def test_packed_domain_boundary_is_the_formula_of_the_header(swmi_mod):
    """include/swmi.h and DESIGN.md 9: packed while len * max(s, 0) + 18 * max(0, -min s) + open + extend + 64 < 0x7C00
    (18 = kBandedTrip + 2).  With (20, -100) the growing bias takes 1800 of the range, not 200: the last packed length at
    (5, 1) is 1493, where a formula with 2 B would say 1573."""
    k = swmi_mod.banded_affine_kernel_for
    sm = match_matrix(20, -100)
    assert 20 * 1493 + 18 * 100 + 5 + 1 + 64 < 0x7C00 <= 20 * 1494 + 18 * 100 + 5 + 1 + 64
    assert 20 * 1573 + 2 * 100 + 5 + 1 + 64 < 0x7C00 <= 20 * 1574 + 2 * 100 + 5 + 1 + 64
    assert k(1493, sm, 5, 1) == ("sw_banded_affine_pk_kernel<1>", 2) and k(1494, sm, 5, 1) == ("sw_banded_affine_kernel<1,1>", 1)
    assert k(1493, sm, 1, 5) == ("sw_banded_affine_pk_kernel<0>", 2) and k(1494, sm, 1, 5) == ("sw_banded_affine_kernel<0,1>", 1)
    assert k(1573, sm, 5, 1)[0] == "sw_banded_affine_kernel<1,1>" and k(1639, sm, 5, 1)[0] == "sw_banded_affine_kernel<1,0>"   # 32780
    rng = np.random.default_rng(18)
    for _ in range(400):                                  # ... and everywhere else: the restated rule against the library's
        m = rng.integers(-128, 128, 16).astype(np.int8) if rng.random() < 0.5 else match_matrix(int(rng.integers(0, 128)), int(rng.integers(-128, 2)))
        length, go, ge = int(rng.integers(64, 1793)), int(rng.integers(0, 128)), int(rng.integers(0, 128))
        assert k(length, m, go, ge)[0] == be.kernel_name(length, m, go, ge), (length, m, go, ge)


def test_the_two_numpy_formulations_and_the_oracle_agree(oracle):
    """the per-cell formulation (test_banded_affine.py's, with the bounds as parameters) and the batched anti-diagonal one
    at every band, and both against the oracle at the true band"""
    rng = np.random.default_rng(5)
    for length in (64, 67, 81, 150):
        a, b = be.related(rng, 3, length, indel=0.04)
        a[2], b[2] = be.shifted_pair(rng, length, 63 if length > 100 else -40)
        for sm, go, ge in ((match_matrix(2, -3), 5, 1), (match_matrix(1, -1), 0, 0), (random_matrix(), 2, 9), (match_matrix(3, 1), 4, 2)):
            for lo, hi in [(be.LO, be.HI)] + be.NEIGHBOUR_BANDS + [(-3, 5), (0, 0)]:
                want = [be.numpy_banded_gotoh(a[k], b[k], sm, go, ge, lo, hi) for k in range(3)]
                assert list(be.band_scores(a, b, sm, go, ge, lo, hi)) == want, (length, go, ge, lo, hi)
            assert list(oracle.banded_affine(a, b, sm, go, ge)) == list(be.band_scores(a, b, sm, go, ge)), (length, go, ge)


@pytest.mark.parametrize("family", list(be.FAMILIES))
def test_every_claim_of_a_family_holds(oracle, family):
    """through the oracle for every case; through the numpy formulation for the packed body's cases (the other bodies run
    the same sequences with a larger match)"""
    claimed = bounded = 0
    for case in be.FAMILIES[family]():
        got = oracle.banded_affine(case.a, case.b, case.sm, case.gap_open, case.gap_ext)
        for k in range(len(got)):
            if case.want[k] >= 0:
                assert got[k] == case.want[k], (case.what(k), int(got[k]), int(case.want[k]))
                claimed += 1
            if case.below[k] >= 0:
                assert got[k] < case.below[k], (case.what(k), int(got[k]), int(case.below[k]))
                bounded += 1
        if "_pk_" in case.kernel:
            assert np.array_equal(be.band_scores(case.a, case.b, case.sm, case.gap_open, case.gap_ext), got), case
    print("%s: %d scores claimed by hand, %d bounded from above" % (family, claimed, bounded))
    assert claimed >= 100 and bounded >= 60


def test_issue_figures_of_the_shifted_copies_and_corners(oracle):
    """what the generators were designed from: a shift of 63 scores 2 (len - 63), all six in-band corners 8 * 5 = 40"""
    for length in (128, 333, 1024):
        c = be.shift_case(length, 2, -3, 127, 127)
        got = oracle.banded_affine(c.a, c.b, c.sm, 127, 127)
        assert got[be.SHIFTS.index(63)] == 2 * (length - 63) and got[be.SHIFTS.index(-64)] == 2 * (length - 64)
        assert got[be.SHIFTS.index(64)] < 40 and got[be.SHIFTS.index(-65)] < 40
    for length in (81, 333, 1057):
        c = be.corner_case(length, 5, -30, 127, 127)
        got = oracle.banded_affine(c.a, c.b, c.sm, 127, 127)
        assert list(got[:6]) == [40] * 6 and (got[6:] < 40).all() and (got[6:] > 0).all(), (length, got)


def test_a_band_off_by_one_gets_a_case_of_every_length_wrong(oracle):
    """The teeth.  The numpy formulation at the four neighbouring bands: each disagrees with the true band on a shifted copy
    AND on a gap run at every length (so the GPU file fails on a kernel whose band is off by one on either side), and with
    the cheap gap sets (0, 0) and (1, 4) from len 1024 on."""
    for length in be.SHIFT_LENGTHS:
        cases = [be.shift_case(length, 2, -3, 127, 127)]
        if length in be.GAP_LENGTHS:
            cases.append(be.gap_run_case(length, 2, -3, 5, 1))
        if length in (1024, 1792):
            cases += [be.gap_run_case(length, 2, -3, 0, 0), be.gap_run_case(length, 2, -3, 1, 4)]
        for c in cases:
            true = be.band_scores(c.a, c.b, c.sm, c.gap_open, c.gap_ext)
            assert np.array_equal(true, oracle.banded_affine(c.a, c.b, c.sm, c.gap_open, c.gap_ext)), c
            for lo, hi in be.NEIGHBOUR_BANDS:
                other = be.band_scores(c.a, c.b, c.sm, c.gap_open, c.gap_ext, lo, hi)
                wrong = [c.labels[k] for k in np.nonzero(other != true)[0]]
                print("%-8s len %4d (%d,%d) band [%d,%d]: differs on %s" % (c.name, length, c.gap_open, c.gap_ext, lo, hi, wrong))
                assert wrong, (c, lo, hi)
                # ... on the case that sits on the moved edge, by the whole run, not by noise
                edge = {(-63, 63): -64, (-65, 63): -65, (-64, 62): 63, (-64, 64): 64}[(lo, hi)]
                label = "shift %+d" % edge if c.family == "shift" else "%s %d (%d,%d)" % ("insert" if edge > 0 else "delete", abs(edge), c.gap_open, c.gap_ext)
                k = c.labels.index(label)
                assert abs(int(other[k]) - int(true[k])) > length // 8, (c, lo, hi, label, int(other[k]), int(true[k]))


def test_the_corner_blocks_separate_the_bands_too():
    """a block of 8 one diagonal outside scores the full 8 * match as soon as the band is one wider on that side, and an
    in-band corner loses it as soon as the band is one narrower"""
    for length in (79, 81, 334):
        c = be.corner_case(length, 5, -30, 127, 127)
        true = be.band_scores(c.a, c.b, c.sm, 127, 127)
        for (lo, hi), moved in zip(be.NEIGHBOUR_BANDS, (("corner (65,1)", "corner (len,len-64)"), ("outside (66,1)", "outside (len,len-65)"),
                                                       ("corner (1,64)", "corner (len-63,len)"), ("outside (1,65)", "outside (len-64,len)"))):
            other = be.band_scores(c.a, c.b, c.sm, 127, 127, lo, hi)
            assert {c.labels[k] for k in np.nonzero(other != true)[0]} == set(moved), (length, lo, hi)


def test_at_len_64_the_band_is_the_whole_table(oracle):
    """-64 <= j - i <= 63 holds for every cell of a 64 x 64 table: the banded score is the unbanded local Gotoh score of
    affine_edges.py's whole-table formulation, for any input and every gap set"""
    rng = np.random.default_rng(64)
    a, b = be.related(rng, 10, 64, sub=0.1, indel=0.05)
    a[6:] = rng.integers(0, 4, (4, 64), dtype=np.uint8)
    a[9], b[9] = be.shifted_pair(rng, 64, -30)
    for sm in (match_matrix(2, -3), match_matrix(1, -1), random_matrix(), match_matrix(3, 1)):
        for go, ge in AFFINE_GAPS:
            want = [ae.numpy_affine(a[k], b[k], sm, go, ge, local=True)[0] for k in range(len(a))]
            assert list(oracle.banded_affine(a, b, sm, go, ge)) == want, (sm, go, ge)
            assert list(be.band_scores(a, b, sm, go, ge)) == want, (sm, go, ge)


def test_bias_against_cost_parameter_sets(swmi_mod):
    """B - cost in {-1, 0, +1} in both packed bodies, cost = 0 and B = 0 among them, all inside the packed domain"""
    params = be.bias_cost_params()
    for oge in (True, False):
        seen = {(bias - cost, cost) for sm, go, ge, bias, cost in params if (go >= ge) == oge}
        assert {(d, c) for c in (1, 5, 20, 126) for d in (-1, 0, 1)} | {(0, 0), (1, 0)} <= seen, oge
        assert any(bias == 0 for sm, go, ge, bias, cost in params if (go >= ge) == oge)
    for sm, go, ge, bias, cost in params:
        assert bias == max(0, -int(sm.min())) and cost == (ge if go >= ge else go)
        for length in (333, 1024):
            assert swmi_mod.banded_affine_kernel_for(length, sm, go, ge) == ("sw_banded_affine_pk_kernel<%d>" % (go >= ge), 2)


def test_the_16_bit_bodies_end_at_32767(swmi_mod, oracle):
    """len 1057 x match 31 = 2^15 - 1, the last H a v_max_i16 holds; 1024 x 32 = 2^15 runs the plain cell"""
    k = swmi_mod.banded_affine_kernel_for
    assert k(1057, match_matrix(31, -40), 5, 1) == ("sw_banded_affine_kernel<1,1>", 1)
    assert k(1057, match_matrix(31, -40), 1, 4) == ("sw_banded_affine_kernel<0,1>", 1)
    assert k(1024, match_matrix(32, -40), 5, 1) == ("sw_banded_affine_kernel<1,0>", 1)
    assert k(1024, match_matrix(32, -40), 1, 4) == ("sw_banded_affine_kernel<0,0>", 1)
    a = np.random.default_rng(1).integers(0, 4, (1, 1057), dtype=np.uint8)
    assert oracle.banded_affine(a, a, match_matrix(31, -40), 5, 1)[0] == 32767
    assert oracle.banded_affine(a[:, :1024], a[:, :1024], match_matrix(32, -40), 1, 4)[0] == 32768


def test_bytes_that_are_no_base_count_by_their_low_two_bits(oracle):
    rng = np.random.default_rng(255)
    a, b = be.related(rng, 6, 333)
    for sm, go, ge in ((match_matrix(2, -3), 5, 1), (random_matrix(), 1, 4)):
        want = oracle.banded_affine(a, b, sm, go, ge)
        assert np.array_equal(oracle.banded_affine(a | 0xFC, b | 0x54, sm, go, ge), want)
        assert np.array_equal(be.band_scores(a | 0xFC, b | 0x54, sm, go, ge), want)


def test_the_oracle_equals_the_reference_on_f7(oracle):
    """F7: 28 alignments of two 128-mers by the reference's SmithWaterman_111_long at (1, -1, 1), with paths.  All 28 paths
    lie inside the band (a condition: the test cannot pass by leaving cases out), 16 contain gaps; the banded affine oracle
    at open = extend = 1 gives the reference's score for each, with the sequences in either order."""
    f7 = [v for v in load_f7() if v["len1"] == 128]
    assert len(f7) == 28 and all(len(v["seq2"]) == 128 for v in f7)
    assert sum(in_band(v["path"], -63, 63) for v in f7) == 28            # within 63 either way: in band in both orders
    steps = [np.diff(np.asarray(v["path"]), axis=0) for v in f7]
    assert sum(bool((s.sum(axis=1) == 1).any()) for s in steps) == 16    # a step that moves one index only: a gap
    a = np.stack([v["seq1"] for v in f7])
    b = np.stack([v["seq2"] for v in f7])
    want = np.array([v["score"] for v in f7], np.int32)
    sm = match_matrix(1, -1)
    assert np.array_equal(oracle.banded_affine(a, b, sm, 1, 1), want)
    assert np.array_equal(oracle.banded_affine(b, a, sm, 1, 1), want)
    assert np.array_equal(be.band_scores(a, b, sm, 1, 1), want)


def test_the_oracle_equals_the_affine_local_aligner_wherever_its_path_stays_in_band(oracle, loracle, swmi_mod):
    """len 128, 4 matrices x the 7 gap sets of AFFINE_GAPS x 120 pairs against tests/native/local_affine_oracle.c, the path
    expanded on the host: at least 90 % of the cases are in band (a cap on what is left out) and every one of those is
    equal; no banded score is above the unbanded one, and some are strictly below, so the inequality is not vacuous"""
    a, b = cross_pin_inputs()
    assert move_words(128) == swmi_mod.local_move_words(128)
    cases, inside, lower = cross_pin(a, b, lambda sm, go, ge: oracle.banded_affine(a, b, sm, go, ge),
                                     lambda sm, go, ge: loracle.align(a, b, sm, go, ge), swmi_mod.local_expand_moves)
    print("cross-pin: %d cases, %d in band (all equal), %d of the other %d strictly lower" % (cases, inside, lower, cases - inside))
    assert cases == 3360 and inside >= 0.9 * cases and lower >= 1
