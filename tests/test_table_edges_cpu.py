"""The edge generators of table_edges.py checked without a device: every edge a generator claims is met, through the C
restatements (tests/native/local_oracle.c, sgfull_oracle.c) or the whole-table numpy formulation, by at least as many
alignments as test_table_edges_gpu.py relies on, so that a later edit of a generator cannot quietly drop an edge; the
restatements against numpy on the tie and pad cases; the grids against the kernels' constants."""
import numpy as np
import pytest

import table_edges as te
from local_support import LocalOracle
from sgfull_support import SgFullOracle, moves_to_path, numpy_sgfull


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def test_grids_follow_the_kernel_constants():
    sg, loc = te.SG, te.LOC
    # the constants the grids are derived from, as the kernels' headers describe them
    assert (sg["kCols"], sg["kMaxWaves"], sg["kUnroll"], sg["kChunk"], sg["kDelay"], sg["kRing"], sg["kStageRows"],
            sg["kStageLanes"]) == (16, 16, 4, 32, 3, 256, 128, 64)
    assert (loc["kLanes"], loc["kCols"], loc["kAlnPerWave"], loc["kAlnPerBlock"], loc["kUnroll"]) == (16, 8, 4, 16, 8)
    grid = te.sg_shape_grid()
    assert {l1 for l1, _, _ in grid} == set(te.SG_LEN1) and {l2 for _, l2, _ in grid} == set(te.SG_LEN2)
    assert {te.sg_waves(l2) for _, l2, _ in grid} == set(range(1, sg["kMaxWaves"] + 1))          # every W
    for W in te.SG_FULL_W:                                                                    # every edge of the last wave
        l2s = {l2 for _, l2, _ in grid if te.sg_waves(l2) == W}
        assert {1024 * W, 1024 * W - 1, 1024 * (W - 1) + 1} <= l2s and any(v % 16 == 15 for v in l2s), W
    for x in (4, 32, 128, 256):                                                               # trip, chunk, block, ring
        assert {x - 1, x, x + 1} <= set(te.SG_LEN1)
    assert {33, 65, 129, 257, 4097} <= set(te.SG_LEN1)                                         # local_chunks steps up
    assert max(n for l1, l2, n in grid if l1 * l2 >= 1 << 25) <= 2                           # a few alignments of the large
    assert any(l1 == 16384 for l1, _, _ in grid) and any(l2 == 16384 for _, l2, _ in grid)
    lgrid = te.local_shape_grid()
    assert {n for _, n in lgrid} == {1, 3, 4, 5, 15, 16, 17, 63, 64, 65}
    steps = {(l1 + 15) % 8 for l1, _ in lgrid}
    assert {0, 1, 7} <= steps and {127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 16383, 16384} <= {l1 for l1, _ in lgrid}


def _report(case, counts):
    print("%-40s %s" % (case.name + " %dx%d n=%d" % (case.shape + (len(case.a),)),
                        ", ".join("%s %d" % kv for kv in sorted(counts.items()))))


def _check(case, counts):
    _report(case, counts)
    for claim, need in case.claims.items():
        assert counts[claim] >= need, (case, claim, counts[claim], need)


def test_sgfull_long_gap_runs_cross_waves_and_blocks(sgoracle):
    """interior left runs of >= 1100 columns across j = 1024 k, interior up runs of more than 128 rows"""
    for case in te.sg_gap_run_cases():
        _check(case, te.sg_claim_counts(case, sgoracle.align(case.a, case.b, case.sm, case.gap)))


def test_sgfull_staircases_leave_blocks_every_way(sgoracle):
    """several interior gaps of 100..250 both ways; staging blocks left through the top and a corner (the long insertions
    leave them through the left edge), and blocks that span two waves"""
    for case in te.sg_staircase_cases() + te.sg_corner_cases():
        _check(case, te.sg_claim_counts(case, sgoracle.align(case.a, case.b, case.sm, case.gap)))


def test_sgfull_best_cell_at_a_wave_edge(sgoracle):
    for case in te.sg_wave_edge_end_cases():
        _check(case, te.sg_claim_counts(case, sgoracle.align(case.a, case.b, case.sm, case.gap)))


def test_sgfull_ties_across_lanes_and_waves(sgoracle):
    """the maximum in two lanes of one wave and in two waves, the row-major-first occurrence in a later wave / lane than an
    occurrence in a later row; the restatement equals numpy on every one of them"""
    for case in te.sg_tie_cases():
        res = sgoracle.align(case.a, case.b, case.sm, case.gap)
        _check(case, te.sg_claim_counts(case, res))
        _restatement_equals_numpy_sgfull(case, res)


def test_sgfull_best_cell_in_column_len2_with_gap_0(sgoracle):
    """gap 0 and len2 % 16 != 0: the best cell in column len2, the pad column beside it holding the same value"""
    for case in te.sg_pad_cases():
        res = sgoracle.align(case.a, case.b, case.sm, case.gap)
        _check(case, te.sg_claim_counts(case, res))
        if case.shape[1] <= 1025:
            _restatement_equals_numpy_sgfull(case, res)
        for k in range(len(case.a)):                    # the pad column's value equals the best on the best cell's row
            H = te.sgfull_table(case.a[k], case.b[k], case.sm, 0) if case.shape[1] <= 1025 else None
            if H is not None and res[1][k, 1] == case.shape[1]:
                i = res[1][k, 0]
                assert H[i, -1] == res[0][k] and H[i, :-1].max() < res[0][k]


def _restatement_equals_numpy_sgfull(case, res):
    sc, ends, moves, lengths = res
    for k in range(len(sc)):
        want_score, want_end, want_path = numpy_sgfull(case.a[k], case.b[k], case.sm, case.gap)
        assert sc[k] == want_score and tuple(ends[k]) == want_end, (case, k)
        assert np.array_equal(moves_to_path(moves[k], lengths[k], ends[k, 0], ends[k, 1]), want_path), (case, k)


def test_sgfull_extremes_reach_the_bounds_of_h(sgoracle):
    """16384 x 16384: the highest H (127 * 16384 at the corner) and a table whose every cell is at most 0"""
    cases = {c.name: c for c in te.sg_extreme_cases()}
    c = cases["extreme/all+127/0"]
    sc, ends, _, _ = sgoracle.align(c.a[:1], c.b[:1], c.sm, c.gap, traceback=False)
    assert sc[0] == 127 * 16384 and tuple(ends[0]) == (16384, 16384)
    c = cases["extreme/all-128/127"]
    sc, ends, _, _ = sgoracle.align(c.a[:1], c.b[:1], c.sm, c.gap, traceback=False)
    assert sc[0] == 0 and tuple(ends[0]) == (0, 0)
    # the lowest H: -128 per diagonal step (cheaper than two gaps of 127), -128 * 16384 = -2^21 at the corner
    H = te.sgfull_table(c.a[0, :300], c.b[0, :300], c.sm, c.gap)
    i, j = np.indices(H.shape)
    assert np.array_equal(H, -128 * np.minimum(i, j) - 127 * abs(i - j)) and H.min() == -128 * 300


def test_local_insertions_make_long_up_runs(loracle):
    for case in te.local_insertion_cases():
        res = loracle.align(case.a, case.b, case.sm, case.gap)
        _check(case, te.local_claim_counts(case, res))


def test_local_ties_over_lanes_columns_and_rows(loracle):
    """the maximum in two of the 16 lanes, the first occurrence in a later lane than one in a later row, in an earlier
    column of the same lane in a later row, in the same column in a later row; the restatement equals numpy on each"""
    for case in te.local_tie_cases():
        res = loracle.align(case.a, case.b, case.sm, case.gap)
        _check(case, te.local_claim_counts(case, res))
        sc, ends, moves, steps = res
        for k in range(len(sc)):
            score, end, start, path = te.numpy_local(case.a[k], case.b[k], case.sm, case.gap)
            assert sc[k] == score and tuple(ends[k]) == end + start, (case, k)
            c, i, j = te.walk_cells(moves[k], int(steps[k]), end[0], end[1])
            assert np.array_equal(np.stack([i, j], axis=1)[::-1], path), (case, k)


def test_local_extremes(loracle):
    cases = {c.name: c for c in te.local_extreme_cases()}
    c = cases["local_extreme/all+127/0"]
    sc, ends, _, steps = loracle.align(c.a, c.b, c.sm, c.gap)
    assert (sc == 127 * 128).all() and (ends[:, :2] == 128).all()          # 16256: the most the key's H field holds
    c = cases["local_extreme/all-128/127"]
    sc, ends, _, steps = loracle.align(c.a, c.b, c.sm, c.gap)
    assert (sc == 0).all() and (ends == 0).all() and (steps == 0).all()
    assert (127 * 128 + 127) << 17 < 1 << 31                                # H + s of a diagonal candidate still fits


def test_numpy_local_matches_the_restatement_on_small_sizes(loracle):
    rng = np.random.default_rng(41)
    for name, sm, gap in te.LOCAL_PARAMS:
        for len1 in (1, 7, 40, 130):
            a, b = te.local_mixed_pairs(6, len1, int(rng.integers(0, 1 << 30)))
            sc, ends, moves, steps = loracle.align(a, b, sm, gap)
            for k in range(6):
                score, end, start, path = te.numpy_local(a[k], b[k], sm, gap)
                assert sc[k] == score and tuple(ends[k]) == end + start and steps[k] + 1 == len(path), (name, len1, k)


def test_path_predicates_on_hand_made_walks():
    """the run, wave-crossing and staging-block predicates on walks written out by hand"""
    # from (200, 3000): 100 diagonal, a left run of 1500 at row 100 (columns 2900 .. 1400), then diagonal and up to (0, 0)
    codes = [3] * 100 + [1] * 1500 + [3] * 100 + [1] * 1300
    words = np.zeros(96, np.uint64)
    for t, c in enumerate(codes):
        words[t // 32] |= np.uint64(c << (2 * (t % 32)))
    facts = te.sg_path_facts(10, (200, 3000), words, len(codes) + 1)
    assert facts["left_run_1100_across_waves"] and facts["left_run_over_1024"] and not facts["up_run_over_128"]
    assert facts["block_exit_left"] and not facts["end_at_wave_edge"]
    c, i, j = te.walk_cells(words, len(codes), 200, 3000)
    assert (i[-1], j[-1]) == (0, 0)
    assert te.gap_runs(c, i, j)[0] == (1, 1500, 100, 2900)
