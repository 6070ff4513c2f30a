"""The edge generators of affine_edges.py checked without a device: every edge a generator claims is met, through the C
restatements (tests/native/local_affine_oracle.c, sgfull_affine_oracle.c) and the whole-table numpy formulation, by at least
as many alignments as test_affine_edges_gpu.py relies on, so that a later edit of a generator cannot quietly drop an edge.
The predicates need the walk's state, which no aligner returns: it comes from the numpy tables, whose score, best cell and
moves are first shown equal to the restatement's on every alignment of every case.  Also: the numpy formulation against the
older per-cell one (gotoh_numpy) and both restatements over the gap families; the (open = extend) cases against the LINEAR
restatements; the grids against the affine kernels' constants; the bounds the keys' shifts are argued from; the predicates
on walks written out by hand."""
import numpy as np
import pytest

import affine_edges as ae
import local_affine_support as las
import sgfull_affine_support as sas
import table_edges as te
from conftest import match_matrix
from local_affine_support import AFFINE_GAPS, AffineOracle
from local_support import LocalOracle, random_matrix
from local_support import move_words as local_move_words
from sgfull_affine_support import SgAffineOracle
from sgfull_support import SgFullOracle
from sgfull_support import move_words as sg_move_words


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_affine_oracle"))


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


@pytest.fixture(scope="module")
def linear_sg(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


@pytest.fixture(scope="module")
def linear_local(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def test_grids_follow_the_affine_kernel_constants():
    sg, loc = ae.SGA, ae.LOCA
    # A changed constant fails here.  kStageLanes / kStageRows: revisit sg_corner_cases, sg_open_exit_cases and the run
    # lengths of sg_run_cases (longer than a block is wide and high); the others: the shape grids and the wave / lane
    # boundaries of the run and tie generators.
    assert (sg["kStageLanes"], sg["kStageRows"]) == (32, 128), "the block-exit generators assume 128 rows x 512 columns"
    assert (sg["kCols"], sg["kMaxWaves"], sg["kUnroll"], sg["kChunk"], sg["kDelay"], sg["kRing"]) == (16, 16, 4, 32, 3, 256), \
        "sg_shape_grid, and the columns 1024 k of the run generators"
    assert (loc["kLanes"], loc["kCols"], loc["kAlnPerWave"], loc["kAlnPerBlock"], loc["kUnroll"]) == (16, 8, 4, 16, 8), \
        "local_shape_grid, and the columns 8 l of local_run_cases"
    assert (sg["kTagH"], sg["kTagE"], sg["kTagF"]) == (48, 32, 16) and sg["kMinusInf"] == loc["kMinusInf"] == ae.NEG
    assert loc["kValue"] == -(1 << 17) and (loc["kFloor"], loc["kBoundary"]) == (3 << 15, 2 << 15)
    grid = ae.sg_shape_grid()
    assert {l1 for l1, _, _ in grid} == set(ae.SGA_LEN1) and {l2 for _, l2, _ in grid} == set(ae.SGA_LEN2)
    assert {te.sg_waves(l2) for _, l2, _ in grid} == set(range(1, sg["kMaxWaves"] + 1))          # every W
    for W in te.SG_FULL_W:                                                                    # every edge of the last wave
        l2s = {l2 for _, l2, _ in grid if te.sg_waves(l2) == W}
        assert {1024 * W, 1024 * W - 1, 1024 * (W - 1) + 1} <= l2s and any(v % 16 == 15 for v in l2s), W
    for x in (4, 32, 64, 128, 256, 4096):                                                     # trip, chunk, 64, block, ring, 16 rings
        assert {x - 1, x, x + 1} <= set(ae.SGA_LEN1)
    assert {16383, 16384} <= set(ae.SGA_LEN1)
    assert max(n for l1, l2, n in grid if l1 * l2 >= 1 << 25) <= 2
    # the three gap families on every shape, (0, 0), (5, 0), (0, 5) in turn
    assert {tuple(p[2:]) for k in range(3) for p in ae.grid_params(k)} == {(11, 1), (3, 7), (0, 0), (5, 0), (0, 5)}
    lgrid = ae.local_shape_grid()
    assert {n for _, n in lgrid} == {1, 3, 4, 5, 15, 16, 17, 63, 64, 65}
    steps = {(l1 + 15) % 8 for l1, _ in lgrid}
    assert {0, 1, 7} <= steps and {127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 16383, 16384} <= {l1 for l1, _ in lgrid}
    # the linear grids are what they were: the parameters of table_edges.py default to the linear kernels' constants
    assert te.sg_shape_grid() == te.sg_shape_grid(te.sg_len1_grid(te.SG), te.sg_len2_grid(te.SG))
    assert te.local_shape_grid() == te.local_shape_grid(te.local_len1_grid(te.LOC), te.local_n_grid(te.LOC))
    assert te.SG["kStageLanes"] == 2 * sg["kStageLanes"]


def _report(case, counts):
    print("%-44s %-9s %s" % (case.name + " %dx%d n=%d" % (case.shape + (len(case.a),)), "%d,%d" % case.gaps,
                             ", ".join("%s %d" % kv for kv in sorted(counts.items()))))


def _check(case, oracle, local, linear=None):
    """the restatement equals numpy field for field on every alignment; every claim is met; the hand-made score"""
    counts, results = ae.claim_counts(case, local)
    _report(case, counts)
    want = oracle.align(case.a, case.b, case.sm, case.gap_open, case.gap_extend)
    if local:
        te.assert_same(ae.local_result_of(results, local_move_words(case.shape[0])), want, ("numpy", repr(case)), "local")
    else:
        te.assert_same(ae.sg_result_of(results, sg_move_words(*case.shape)), want, ("numpy", repr(case)), "sgfull")
    if case.score is not None:
        assert (want[0] == case.score).all(), (case, want[0].tolist(), case.score)
    if linear is not None and case.linear_gap is not None:       # open = extend: the affine restatement is the linear one
        te.assert_same(want, linear.align(case.a, case.b, case.sm, case.linear_gap), ("linear", repr(case)), "local" if local else "sgfull")
    for claim, need in case.claims.items():
        assert counts[claim] >= need, (case, claim, counts[claim], need)
    return want


def test_sgfull_single_runs_extend_across_waves_and_leave_blocks_inside_the_gap(sgoracle):
    """one gap run of exactly |R| (the score identity), left runs inside F across j = 1024 k up to the last boundary of 16
    waves, up runs inside E of more than 128 rows, blocks left inside the run; extend = 0 along a whole row"""
    cases = ae.sg_run_cases()
    assert [c.score for c in cases[:5]] == [1991, 6391, 3591, 2591, 2591]
    for case in cases + ae.sg_extend0_cases():
        _check(case, sgoracle, False)


def test_sgfull_staircases_corners_and_exits_on_the_opening_move(sgoracle):
    for case in ae.sg_staircase_cases() + ae.sg_corner_cases() + ae.sg_open_exit_cases() + ae.sg_wave_edge_end_cases():
        _check(case, sgoracle, False)
    lo = 16 * (ae.STAGE_LANES - 1) - (ae.STAGE_ROWS - 1)
    assert lo == 369 and {int(c.name.split("L=")[1]) for c in ae.sg_corner_cases()} <= set(range(lo, lo + 16))


def test_sgfull_best_cell_ties_equal_the_linear_restatement(sgoracle, linear_sg):
    for case in ae.sg_best_tie_cases():
        assert case.linear_gap is not None
        _check(case, sgoracle, False, linear_sg)


def test_sgfull_path_ties_meet_every_tag_order(sgoracle):
    """every path tie on at least 4 alignments per gap family, where the family allows it"""
    cases = ae.sg_path_tie_cases()
    for case in cases:
        _check(case, sgoracle, False)
    assert all(set(ae.PATH_TIES[:3]) <= set(c.claims) for c in cases)
    assert sum("tie_E_open_extend" in c.claims and "tie_F_open_extend" in c.claims for c in cases) == 3


def test_sgfull_best_cell_in_column_len2_with_open_0(sgoracle, linear_sg):
    """open = 0 and len2 % 16 != 0: the best cell in column len2, the pad column beside it reaching the same value"""
    for case in ae.sg_pad_cases():
        want = _check(case, sgoracle, False, linear_sg)
        if case.shape[1] <= 1025:
            for k in range(len(case.a)):
                if want[1][k, 1] == case.shape[1]:          # no earlier column of the best cell's row holds the best value
                    H = ae.affine_tables(case.a[k], case.b[k], case.sm, 0, case.gap_extend)[0]
                    assert H[want[1][k, 0], -1] == want[0][k] and H[want[1][k, 0], :-1].max() < want[0][k]


def test_local_runs_extend_across_lanes(loracle):
    for case in ae.local_run_cases():
        _check(case, loracle, True)


def test_local_best_cell_ties_equal_the_linear_restatement(loracle, linear_local):
    for case in ae.local_best_tie_cases():
        assert case.linear_gap is not None
        _check(case, loracle, True, linear_local)


def test_local_path_ties_meet_every_tag_order(loracle):
    cases = ae.local_path_tie_cases()
    for case in cases:
        _check(case, loracle, True)
    assert all(set(ae.PATH_TIES[:3] + ae.FLOOR_TIES) <= set(c.claims) for c in cases)


def _letters(walk):
    return ["?LUD"[c] for c in walk.codes]


def test_numpy_tables_equal_both_restatements_and_gotoh_numpy(sgoracle, loracle):
    """affine_tables and the state walk against the restatements on a grid of small random shapes for each of the seven
    gap pairs (both regimes: open >= extend and open < extend), and against the per-cell gotoh_numpy of both support
    modules, tables included"""
    rng = np.random.default_rng(77)
    assert any(go < ge for go, ge in AFFINE_GAPS) and any(go > ge for go, ge in AFFINE_GAPS)
    for g, (go, ge) in enumerate(AFFINE_GAPS):
        for len1, len2 in ((1, 1), (2, 17), (33, 5), (40, 64), (130, 90), (70, 300)):
            sm = [match_matrix(2, -3), random_matrix(g), te.TIE_MATRICES[2][1]][(g + len1) % 3]
            a, b = te.sg_mixed_pairs(6, len1, len2, int(rng.integers(1 << 30)))
            case = ae.Case("random", a, b, sm, go, ge, {})
            _, results = ae.claim_counts(case, False)
            te.assert_same(ae.sg_result_of(results, sg_move_words(len1, len2)), sgoracle.align(a, b, sm, go, ge), (go, ge, len1, len2), "sgfull")
            for k in (0, 1):
                score, end, letters = sas.gotoh_numpy(a[k], b[k], sm, go, ge)
                assert (score, end, letters) == (results[k][0], results[k][1], _letters(results[k][2])), (go, ge, len1, len2, k)
        for len1 in (1, 7, 40, 130):
            sm = [match_matrix(2, -3), random_matrix(g), te.TIE_MATRICES[2][1]][(g + len1) % 3]
            a, b = te.local_mixed_pairs(6, len1, int(rng.integers(1 << 30)))
            case = ae.Case("random", a, b, sm, go, ge, {})
            _, results = ae.claim_counts(case, True)
            te.assert_same(ae.local_result_of(results, local_move_words(len1)), loracle.align(a, b, sm, go, ge), (go, ge, len1), "local")
            for k in (0, 1):
                score, ends, letters = las.gotoh_numpy(a[k], b[k], sm, go, ge)
                walk = results[k][2]
                assert (score, ends[:2], ends[2:], letters) == (results[k][0], results[k][1], (walk.i[-1], walk.j[-1]), _letters(walk)), (go, ge, len1, k)


def _corner_tables(sm, go, ge, n):
    """H, E, F of the n x n corner of a table whose matrix holds one value (the sequences do not matter then)"""
    H, E, F, _ = ae.affine_tables(np.zeros(n, np.uint8), np.zeros(n, np.uint8), sm, go, ge)
    return H.astype(np.int64), E.astype(np.int64), F.astype(np.int64)


def test_extremes_reach_the_bounds_the_keys_are_argued_from(sgoracle, loracle):
    cases = {c.name: c for c in ae.sg_extreme_cases()}
    c = cases["extreme/all+127/0,0"]
    sc, ends, _, _ = sgoracle.align(c.a[:1], c.b[:1], c.sm, 0, 0, traceback=False)
    assert sc[0] == 127 * 16384 and tuple(ends[0]) == (16384, 16384)          # the highest H, at the corner
    for name in ("extreme/all-128/127,127", "extreme/all-128/127,0", "extreme/all-128/0,127"):
        c = cases[name]
        sc, ends, _, _ = sgoracle.align(c.a[:1], c.b[:1], c.sm, c.gap_open, c.gap_extend, traceback=False)
        assert sc[0] == 0 and tuple(ends[0]) == (0, 0), name
    # the lowest values, on the 300 x 300 corner of the all -128 tables
    n = 300
    i, j = np.indices((n + 1, n + 1))
    inner = (slice(1, None), slice(1, None))
    # (127, 127) is the linear aligner at gap 127: a diagonal step (-128) is cheaper than two gap steps
    H, E, F = _corner_tables(ae._MINUS, 127, 127, n)
    assert np.array_equal(H, -128 * np.minimum(i, j) - 127 * abs(i - j)) and H.min() == -128 * n
    assert np.array_equal(E[inner], H[:-1, 1:] - 127) and np.array_equal(F[inner], H[1:, :-1] - 127)
    assert min(E[inner].min(), F[inner].min()) == -128 * (n - 1) - 2 * 127
    # (127, 0): a gap of any length costs 127, so no cell lies below one gap up and one gap left, -254
    H, E, F = _corner_tables(ae._MINUS, 127, 0, n)
    assert np.array_equal(H[inner], np.maximum(-128 * np.minimum(i, j) - 127 * (i != j), -254)[inner]) and H.min() == -254
    assert (H[0, 1:] == -127).all() and (H[1:, 0] == -127).all()
    assert (E[inner] == -254).all() and (F[inner] == -254).all()               # opened from the border, -127, and never decaying
    # (0, 127): opening is free, so every interior cell is 0; the border is the one gap of 127 (j - 1) the semantics charge
    H, E, F = _corner_tables(ae._MINUS, 0, 127, n)
    assert (H[inner] == 0).all() and np.array_equal(H[0, 1:], -127 * np.arange(n)) and H.min() == -127 * (n - 1)
    assert np.array_equal(E[1, 1:], -127 * np.arange(n)) and (E[2:, 1:] == 0).all() and (F[1:, 2:] == 0).all()
    # every reachable value lies in [-127 (len1 + len2), 127 min(len1, len2)] up to one score, and so does value << 6
    for go, ge in ((127, 127), (127, 0), (0, 127)):
        H, E, F = _corner_tables(ae._MINUS, go, ge, n)
        assert min(H.min(), E[inner].min(), F[inner].min()) >= -127 * 2 * n - 128
    assert (127 * 16384 + 127) << 6 < 1 << 31 and (127 * 2 * 16384 + 127 * 1023 + 128) << 6 < 1 << 30
    # local: 127 * 128 is the most the key's H field holds; a candidate one score above it still fits
    lcases = {c.name: c for c in ae.local_extreme_cases()}
    c = lcases["local_extreme/all+127/0,0"]
    sc, ends, _, steps = loracle.align(c.a, c.b, c.sm, 0, 0)
    assert (sc == 127 * 128).all() and (ends[:, :2] == 128).all()
    for name in ("local_extreme/all-128/127,127", "local_extreme/all-128/127,0", "local_extreme/all-128/0,127"):
        c = lcases[name]
        sc, ends, _, steps = loracle.align(c.a, c.b, c.sm, c.gap_open, c.gap_extend)
        assert (sc == 0).all() and (ends == 0).all() and (steps == 0).all(), name
    assert (127 * 128 + 127) << 17 < 1 << 31


def test_new_predicates_on_hand_made_walks():
    """the state predicates on walks written out by hand"""
    D, EE, EO, FF, FO = (0, 0), (1, 1), (1, 0), (2, 2), (2, 0)      # (state the move is made in, state after it)
    case = ae.Case("hand", np.zeros((1, 700), np.uint8), np.zeros((1, 3001), np.uint8), match_matrix(1, -1), 5, 1, {})
    # from (600, 3000): the block holds rows 473 .. 600 and lanes 156 .. 187, columns 2497 .. 3000
    # 20 diagonal moves, a left run of 600 (columns 2980 .. 2381): out through the left edge inside F at column 2497 -> 2496
    walk = ae.Walk(600, 3000, [D] * 20 + [FF] * 599 + [FO] + [D] * 580)
    assert (walk.i[-1], walk.j[-1]) == (0, 1800) and list(walk.codes[18:22]) == [3, 3, 1, 1]
    f = ae.sg_walk_facts(case, 10, walk)
    assert f["exit_left_in_F"] and not f["exit_left_on_open"] and not f["exit_top_in_E"] and not f["exit_corner"]
    assert not f["F_extends_across_wave"] and f["one_gap_run"] and f["block_exit_left"]       # 2381 .. 2980 crosses no 1024 k
    # the same run from column 3092: it extends from 2049 to 2048
    walk = ae.Walk(600, 3092, [D] * 20 + [FF] * 1099 + [FO] + [D] * 580)
    f = ae.sg_walk_facts(case, 10, walk)
    assert f["F_extends_across_wave"] and not f["F_across_last_wave_of_16"]
    assert not ae.sg_walk_facts(ae.Case("hand", case.a, case.b, case.sm, 1, 1, {}), 10, walk)["F_extends_across_wave"]   # extend = open
    # ... and one whose opening move is the one from 2049 to 2048: the ring's first word only
    walk = ae.Walk(600, 3092, [D] * 20 + [FF] * 1023 + [FO] + [D] * 580)
    assert walk.j[20 + 1023] == 2049 and not ae.sg_walk_facts(case, 10, walk)["F_extends_across_wave"]
    # the cell the walk enters the next block on, (580, 2496): its H takes the diagonal, takes E, or takes F as the walk does
    walk = ae.Walk(600, 3000, [D] * 20 + [FF] * 599 + [FO] + [D] * 580)
    flags = np.zeros((601, 3001), np.uint8)
    for bits, decides in ((ae.DIAG | ae.H_IS_F, True), (ae.H_IS_E | ae.H_IS_F, True), (ae.H_IS_F | ae.F_EXT, False), (ae.H_IS_E, True)):
        flags[580, 2496] = bits
        assert ae.sg_walk_facts(case, 10, walk, flags)["carried_F_decides"] == decides, bits
    assert not ae.sg_walk_facts(case, 10, walk)["carried_F_decides"] and not ae.sg_walk_facts(case, 10, walk, flags)["carried_E_decides"]
    walk = ae.Walk(600, 3000, [D] * 20 + [EE] * 199 + [EO] + [D] * 300)      # enters the next block on (472, 2980)
    for bits, decides in ((ae.DIAG | ae.H_IS_E, True), (ae.H_IS_E | ae.H_IS_F, False), (ae.H_IS_F, True)):
        flags[472, 2980] = bits
        assert ae.sg_walk_facts(case, 10, walk, flags)["carried_E_decides"] == decides, bits
    # a left run whose last move, the opening one, goes from the block's first column to the one before it
    walk = ae.Walk(600, 3000, [D] * 20 + [FF] * 483 + [FO] + [D] * 400)
    assert walk.j[20 + 483] == 2497
    f = ae.sg_walk_facts(case, 10, walk)
    assert f["exit_left_on_open"] and not f["exit_left_in_F"]
    # an up run of 200 from row 580: out through the top inside E; one of 108: out on the opening move
    f = ae.sg_walk_facts(case, 10, ae.Walk(600, 3000, [D] * 20 + [EE] * 199 + [EO] + [D] * 300))
    assert f["exit_top_in_E"] and f["E_run_over_128"] and not f["exit_top_on_open"] and f["up_run_over_128"]
    f = ae.sg_walk_facts(case, 10, ae.Walk(600, 3000, [D] * 20 + [EE] * 107 + [EO] + [D] * 300))
    assert f["exit_top_on_open"] and not f["exit_top_in_E"] and not f["E_run_over_128"]
    # 127 diagonal moves to row 473, a left run to column 2497, a diagonal move through the corner
    f = ae.sg_walk_facts(case, 10, ae.Walk(600, 3000, [D] * 127 + [FF] * 375 + [FO] + [D] * 300))
    assert f["exit_corner"] and not f["exit_left_on_open"] and not f["exit_left_in_F"]
    # two up gaps back to back (open, then a new gap): 129 up moves, but no E state of 128
    f = ae.sg_walk_facts(case, 10, ae.Walk(600, 3000, [EE] * 63 + [EO] + [EE] * 64 + [EO] + [D] * 100))
    assert f["up_run_over_128"] and not f["E_run_over_128"]
    # the pad column: open = 0, the best cell in column len2 = 3001
    pad = ae.Case("hand", case.a, case.b, case.sm, 0, 3, {})
    assert ae.sg_walk_facts(pad, 5, ae.Walk(600, 3001, [D] * 10))["end_at_len2_open0"]
    assert not ae.sg_walk_facts(pad, 5, ae.Walk(600, 3000, [D] * 10))["end_at_len2_open0"]
    assert not ae.sg_walk_facts(case, 5, ae.Walk(600, 3001, [D] * 10))["end_at_len2_open0"]
    # local: a left run inside F from column 20 to 12 passes 17 -> 16 extending; one that opens there does not
    lcase = ae.Case("hand", np.zeros((1, 300), np.uint8), np.zeros((1, 128), np.uint8), match_matrix(1, -1), 5, 1, {})
    f = ae.local_walk_facts(lcase, 10, ae.Walk(100, 30, [D] * 10 + [FF] * 7 + [FO] + [D] * 5))
    assert f["F_extends_across_lane"] and not f["one_left_run_over_8"] and not f["up_run_over_128"]
    f = ae.local_walk_facts(lcase, 10, ae.Walk(100, 30, [D] * 10 + [FF] * 3 + [FO] + [D] * 5))
    assert not f["F_extends_across_lane"]
    f = ae.local_walk_facts(lcase, 10, ae.Walk(250, 30, [D] * 10 + [EE] * 128 + [EO] + [D] * 5))
    assert f["up_run_over_128"] and f["E_run_over_128"]
    # path ties from flags written by hand: a 3 x 3 table, the walk from (2, 2)
    flags = np.zeros((3, 3), np.uint8)
    flags[2, 2] = ae.DIAG | ae.H_IS_E
    flags[1, 1] = ae.H_IS_E | ae.H_IS_F | ae.E_OPEN
    walk = ae.Walk.from_flags(flags, 2, 2, False)
    assert list(walk.codes) == [3, 2, 1] and list(walk.state) == [0, 1, 0]      # diagonal, up (opened), forced left
    f = ae.path_tie_facts(walk, flags)
    assert f["tie_diag_E"] and f["tie_E_F_above_diag"] and not f["tie_diag_F"] and not f["tie_E_open_extend"]
    flags[2, 2] = ae.H_IS_E | ae.E_OPEN | ae.E_EXT                              # E's candidates equal; (1, 2) goes left next
    flags[1, 1] = ae.DIAG
    flags[1, 2] = ae.H_IS_F | ae.F_OPEN
    walk = ae.Walk.from_flags(flags, 2, 2, False)
    assert list(walk.codes) == [2, 1, 3] and ae.path_tie_facts(walk, flags)["tie_E_open_extend"]
    flags[1, 2] = ae.H_IS_E | ae.E_OPEN                                         # ... goes up next: either order gives these moves
    assert not ae.path_tie_facts(ae.Walk.from_flags(flags, 2, 2, False), flags)["tie_E_open_extend"]
    flags[:] = 0
    flags[2, 2] = ae.DIAG
    flags[1, 1] = ae.FLOOR | ae.DIAG | ae.H_IS_F
    walk = ae.Walk.from_flags(flags, 2, 2, True)
    f = ae.path_tie_facts(walk, flags, True)
    assert list(walk.codes) == [3] and f["tie_floor_diag"] and f["tie_floor_gap"] and not f["tie_diag_F"]
