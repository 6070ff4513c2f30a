"""What gives the structured batch of sg_edges.py its teeth (no GPU): through tests/native/sg_xdrop_profile.c -- the reference's
recurrence once more, reporting what it goes through window by window -- the batch is shown to reach the places where the
X-drop sweeps of sg_kernels.hip could be wrong without a result changing on ordinary inputs: cells that survive at exactly
best - 70, windows whose start margin is exactly 12 and exactly 13 (either side of the calm predicate), cells dropped inside
windows, alignments the rule ends, path steps in all 32 band cells and across the seams of the predecessor records' two
halves, best rounds on the seams of the 16-round record pieces and the 32-round move-bit words, and the state the reference
reads past its pads in.  The profile itself is pinned to oracle/sg_oracle.c's sg_oracle_calm_windows, and the hand-worked
scores, lengths and end cells of sg_edges.py to sg_oracle_xdrop.  test_sg_edges_gpu.py runs the same batch on the GPU."""
import numpy as np
import pytest

import sg_edges as se


@pytest.fixture(scope="module")
def profiled(oracle, tmp_path_factory):
    """[(case, score, traceback, profile)] of the batch; computed once"""
    helper = se.SgProfile(tmp_path_factory.mktemp("sg_profile"))
    out = []
    for c in se.batch():
        score, tb = oracle.semiglobal(c.a, c.b)
        tb.setflags(write=False)
        out.append((c, score, tb, helper.profile(c.a, c.b)))
    return out


def test_the_batch_fills_no_wavefront_and_mixes_dead_and_live_alignments(profiled):
    n = len(profiled)
    assert 80 <= n <= 100 and n % 16 != 0
    lengths = np.array([len(tb) for _, _, tb, _ in profiled])
    for per_wavefront in (16, 32, 64):                      # the sweeps' mappings over 4 lanes, 2 lanes, 1 lane
        for lo in range(0, n, per_wavefront):
            part = lengths[lo: lo + per_wavefront]
            assert (part < 200).any() and (part > se.LEN).any(), (per_wavefront, lo)


def test_the_profile_agrees_with_the_committed_restatement(oracle, profiled):
    for c, score, tb, p in profiled:
        windows, calm, dropped = oracle.calm_windows(c.a, c.b, se.WINDOW, 13)
        assert (p.windows, se.SgProfile.calm(p, 13), int(p.dropped[p.margin >= 13].sum())) == (windows, calm, dropped), c.name
        assert dropped == 0, c.name                          # (the claim behind the calm windows, on this batch too)
        assert oracle.calm_windows(c.a, c.b, se.WINDOW, 14)[1] == se.SgProfile.calm(p, 14), c.name
        assert p.score == score and p.best_round == int(tb[-1].sum()), c.name
        assert p.windows == -(-p.rounds // se.WINDOW) and p.rounds <= 2 * se.LEN + 1, c.name


def test_the_batch_reaches_the_threshold_and_both_sides_of_the_calm_margin(profiled):
    by_name = {c.name: p for c, _, _, p in profiled}
    for margin in (12, 13):
        assert any(((p.margin == margin) & ~p.reach & (p.score_at >= 1)).any() for p in by_name.values()), margin
    # ... and among the alignments whose calm windows the GPU test counts: a kernel that called a window with margin 12 calm
    # would exceed that test's upper bound only there
    for margin in (12, 13):
        assert any(((by_name[k].margin == margin) & ~by_name[k].reach & (by_name[k].score_at >= 1)).any() for k in se.COUNTED), margin
    # ... by more windows than the restatement's count holds windows the kernels refuse for a pad in reach: a kernel with a
    # margin of 12 comes out ABOVE the upper bound #(margin >= 13), not merely above its own predicate
    assert any(se.kernel_predicate(by_name[k], 12) > se.SgProfile.calm(by_name[k], 13) for k in se.COUNTED)
    assert all(se.kernel_predicate(by_name[k], 13) <= se.SgProfile.calm(by_name[k], 13) for k in se.COUNTED)
    assert sum(p.at_threshold for p in by_name.values()) > 1000
    assert by_name["stretch70"].at_threshold > 400 and by_name["stretch70_match_mismatch"].at_threshold > 400
    assert sum(p.by_rule for p in by_name.values()) >= 20 and any(not p.by_rule for p in by_name.values())
    assert sum(int((p.dropped_live > 0).sum()) for p in by_name.values()) > 100
    p = by_name["non_base_periodic"]                         # a non-base in reach of six windows in eight
    assert 0 < int((~p.reach & (p.margin >= 14)).sum()) < se.SgProfile.calm(p, 13) < p.windows


def test_the_paths_cover_the_band_and_the_seams_of_the_records(profiled):
    cells = np.zeros(32, np.int64)
    crossings, residues = set(), set()
    for c, _, tb, p in profiled:
        bc = se.band_cells(tb, p.top_y)
        assert bc.min() >= 0 and bc.max() <= 31, c.name
        cells += np.bincount(bc, minlength=32)
        crossings |= set(zip(bc[:-1].tolist(), bc[1:].tolist())) & {(7, 8), (8, 7), (23, 24), (24, 23)}
        residues.add(p.best_round % 32)
    assert (cells > 0).all(), cells                          # the outer half of the records: cells 0 .. 7 and 24 .. 31
    assert crossings == {(7, 8), (8, 7), (23, 24), (24, 23)}
    assert {0, 1, 15, 16, 17, 31} <= residues
    by_name = {c.name: (tb, p) for c, _, tb, p in profiled}
    for s in (17, 24, 30, 31):                               # seq2 = seq1[s:]: the path starts in band cells 0 .. 7
        tb, p = by_name["shift_left%d" % s]
        assert se.band_cells(tb, p.top_y).min() <= 7, s
    assert by_name["acg_acgt"][1].touched_oob == 1
    assert sum(p.touched_oob for _, p in by_name.values()) >= 1


def test_hand_worked_values(profiled):
    checked = 0
    for c, score, tb, _ in profiled:
        if c.hand is None:
            continue
        assert (score, len(tb), tuple(int(v) for v in tb[-1])) == (c.hand["score"], c.hand["length"], c.hand["end"]), c.name
        checked += 1
    assert checked == 23
    by_name = {c.name: (score, tb) for c, score, tb, _ in profiled}
    for name in ("identical", "all_a", "first_base_mismatch", "stretch69", "stretch70", "stretch45", "stretch60"):
        tb = by_name[name][1]                                # "the full path": the diagonal, cell by cell
        assert np.array_equal(tb, np.stack([np.arange(se.LEN + 1)] * 2, axis=1)), name
    for n in se.PREFIXES:
        if n >= 7:                                           # one base deleted in the middle of the prefix: an odd best round
            score, tb = by_name["prefix%d_deleted" % n]
            assert (score, tuple(tb[-1])) == (n - 2, (n, n - 1)), n


def test_move_words_of_a_traceback():
    """sg_edges.move_words against the definition, on a path with all three moves and more than one word"""
    rng = np.random.default_rng(5)
    steps = rng.integers(1, 4, 77)
    tb = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(np.array([[s >> 1, s & 1] for s in steps]), axis=0)])
    words = se.move_words(tb, 4)
    for t, s in enumerate(steps[::-1]):
        assert (int(words[t >> 5]) >> (2 * (t & 31))) & 3 == s
    assert words[3] == 0 and se.same_moves(words, words.copy(), 78)
    other = words.copy()
    other[2] ^= np.uint64(1 << 30)                           # past the last step: unspecified
    assert se.same_moves(other, words, 78)
    other[2] ^= np.uint64(1 << 24)                           # the last step itself
    assert not se.same_moves(other, words, 78)
