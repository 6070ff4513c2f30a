"""The hand-built inputs of local_full_affine_edges.py without a device: every expected field equals what the C restatement
(tests/native/local_full_affine_oracle.c) and the whole-table numpy formulation (affine_edges.numpy_affine) give, and every
edge a case claims is confirmed on the numpy tables -- so that an edit to a generator that loses its edge fails here."""
import numpy as np
import pytest

import affine_edges as ae
import local_full_affine_edges as lfe
from local_full_affine_support import LocalFullAffineOracle, inputs, moves_of


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return LocalFullAffineOracle(tmp_path_factory.mktemp("local_full_affine_oracle"))


def test_the_grid_follows_the_kernels_constants():
    """the new kernel keeps the mapping of sgfull_affine_kernels.hip, whose predicates affine_edges.py evaluates"""
    for name in ("kCols", "kMaxWaves", "kUnroll", "kChunk", "kDelay", "kRing", "kStageRows", "kStageLanes"):
        assert lfe.KC[name] == ae.SGA[name], name
    assert (lfe.WAVE_COLS, lfe.MAX_LEN, lfe.STAGE_ROWS, lfe.STAGE_COLS, lfe.RING) == (1024, 16384, 128, 512, 256)
    shapes = lfe.shape_grid()
    len2s = {s[1] for s in shapes}
    assert {1023, 1024, 1025, 2047, 2048, 2049, 15361, 16384} <= len2s and {0, 1, 15} <= {v % 16 for v in len2s}
    assert {3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 16384} <= {s[0] for s in shapes}


@pytest.mark.parametrize("group", sorted(lfe.hand_groups()))
def test_hand_built_cases_hold_on_the_restatement_and_on_numpy(oracle, group):
    for h in lfe.hand_groups()[group]():
        sc, ends, mv, st = oracle.align(h.a, h.b, h.sm, h.gap_open, h.gap_extend)
        assert sc[0] == h.score and tuple(ends[0]) == h.ends, (h, sc[0], ends[0])
        if h.codes is not None:
            assert st[0] == len(h.codes) and np.array_equal(moves_of(mv[0], st[0]), np.asarray(h.codes, np.int64)), h
        case = ae.Case(h.name, h.a, h.b, h.sm, h.gap_open, h.gap_extend, {})
        score, end, walk, flags = ae.numpy_affine(h.a[0], h.b[0], h.sm, h.gap_open, h.gap_extend, local=True)
        assert score == h.score and end == h.ends[:2] and (int(walk.i[-1]), int(walk.j[-1])) == h.ends[2:], h
        assert np.array_equal(walk.codes, moves_of(mv[0], st[0])), h
        facts = ae.sg_walk_facts(case, score, walk, flags)
        facts.update(ae.path_tie_facts(walk, flags, True))
        for claim in h.claims:
            assert facts[claim], (h, claim)
        if group == "long_runs" and h.gap_open > h.gap_extend:   # one run past a staging block (it may split where extending is no cheaper)
            runs = [(c, L) for c, L, _, _ in ae.te.gap_runs(walk.codes, walk.i, walk.j)]
            assert max(L for _, L in runs) > lfe.STAGE_ROWS, (h, runs)
        if group == "borders":
            assert (h.ends[2] == 0) != (h.ends[3] == 0) or h.ends[2:] == (0, 0)
            assert len(ae.te.staging_exits(walk.i, walk.j, lfe.STAGE_ROWS, lfe.KC["kStageLanes"])) > 2, h


def test_long_runs_cross_the_wave_boundaries_they_claim():
    cases = {h.name: h for h in lfe.long_run_cases()}
    h = cases["long_left/12,1"]
    _, _, walk, _ = ae.numpy_affine(h.a[0], h.b[0], h.sm, 12, 1, local=True)
    left = walk.j[:-1][walk.codes == lfe.LEFT]
    assert left.min() <= lfe.WAVE_COLS < left.max()                       # the run spans column 1024
    h = cases["long_up/12,1"]
    _, _, walk, _ = ae.numpy_affine(h.a[0], h.b[0], h.sm, 12, 1, local=True)
    assert int(np.sum(walk.codes == lfe.UP)) > lfe.RING                   # more rows than the ring holds


def test_shifted_path_ties_keep_their_ties_and_shift_their_results(oracle):
    for shifted, small in lfe.shifted_path_tie_cases():
        c0 = shifted.b.shape[1] - small.b.shape[1]
        assert c0 > 128 and c0 < lfe.WAVE_COLS < c0 + small.b.shape[1]
        got = oracle.align(shifted.a, shifted.b, shifted.sm, *shifted.gaps)
        want = oracle.align(small.a, small.b, small.sm, *small.gaps)
        moved = want[1] + np.where(want[0] > 0, c0, 0)[:, None] * np.array([0, 1, 0, 1], np.int32)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], moved) and np.array_equal(got[3], want[3]), shifted
        for k in range(len(got[0])):
            assert np.array_equal(moves_of(got[2][k], got[3][k]), moves_of(want[2][k], want[3][k])), (shifted, k)
        tally = dict.fromkeys(shifted.claims, 0)
        for k in range(len(shifted.a)):
            _, _, walk, flags = ae.numpy_affine(shifted.a[k], shifted.b[k], shifted.sm, *shifted.gaps, local=True)
            facts = ae.path_tie_facts(walk, flags, True)
            for c in tally:
                tally[c] += bool(facts[c])
            assert len(walk.codes) == 0 or walk.j.max() > 128
        for c, least in shifted.claims.items():
            assert tally[c] >= least, (shifted, c, tally[c])


@pytest.mark.parametrize("len1,len2", [s for s in lfe.shape_grid() if s[1] > lfe.WAVE_COLS and s[0] >= lfe.WAVE_COLS and s[0] < lfe.MAX_LEN])
def test_grid_inputs_reach_the_wave_and_staging_edges(oracle, len1, len2):
    """what test_local_full_affine_gpu.py asserts of its grid inputs, here on the restatement alone"""
    index = lfe.shape_grid().index((len1, len2))
    for p, (sm, go, ge) in enumerate(lfe.grid_params(index)):
        a, b = inputs(12, len1, len2, 100 * p + len1 % 97 + len2 % 89)
        sc, ends, mv, st = oracle.align(a, b, sm, go, ge)
        lfe.assert_grid_edges(sc, ends, st, (len1, len2, p))
