"""The X-drop semi-global sweeps (sg_forward_split_kernel<4|2, W>, sg_forward_lane_kernel<W>), the character pre-pass and the
walk on the structured batch of sg_edges.py: cells at exactly best - 70 beside cells one below, windows on either side of the
calm predicate's margin, dead alignments beside live ones in every wavefront, the matrix edges, ties, non-base bytes in
every byte of the pre-pass's words, walks through the outer half of the records, `cap` next to the path length -- under
every mapping, with and without calm windows, against oracle/sg_oracle.c, all by exact equality.  And, one alignment per
launch, the kernels' OWN count of calm windows against what tests/native/sg_xdrop_profile.c says may and must be calm: a
predicate that is too lax or too strict changes no result on these inputs, but it changes that count.
test_sg_edges_cpu.py shows that the batch reaches all this."""
import numpy as np
import pytest

import sg_edges as se

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(oracle):
    """the batch and the oracle's (score, traceback, move words) of every alignment; computed once and left unchanged"""
    a, b = se.arrays()
    out = []
    for c in se.batch():
        score, tb = oracle.semiglobal(c.a, c.b)
        words = se.move_words(tb, 1040)
        tb.setflags(write=False)
        words.setflags(write=False)
        out.append((score, tb, words))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, out


@pytest.fixture(scope="module")
def profiles(tmp_path_factory):
    helper = se.SgProfile(tmp_path_factory.mktemp("sg_profile"))
    return {name: helper.profile(se.batch()[se.index_of(name)].a, se.batch()[se.index_of(name)].b) for name in se.COUNTED}


@pytest.fixture
def switches(gpu):
    """(set_mapping, set_exact); both back to automatic / off afterwards, whatever happened"""
    try:
        yield gpu.semiglobal_set_mapping, gpu.semiglobal_set_exact
    finally:
        gpu.semiglobal_set_mapping(-1)
        gpu.semiglobal_set_exact(False)


def _check_moves(gpu, got, want_rows, order, what):
    scores, moves, lengths = got
    assert moves.shape[1] == gpu.SG_MOVE_WORDS == 1040
    for j, k in enumerate(order):
        score, tb, words = want_rows[k]
        name = se.batch()[k].name
        assert int(scores[j]) == score and int(lengths[j]) == len(tb), what + (name, int(scores[j]), score, int(lengths[j]), len(tb))
        assert se.same_moves(moves[j], words, len(tb)), what + (name, "move words")
        assert np.array_equal(gpu.semiglobal_expand_moves(moves[j], int(lengths[j])), tb), what + (name, "expanded path")


@pytest.mark.parametrize("sweep", se.ALL_MAPPINGS)
def test_moves_entry_on_the_structured_batch(gpu, want, switches, sweep):
    set_mapping, set_exact = switches
    a, b, rows = want
    set_mapping(sweep)
    for exact in (False, True):
        set_exact(exact)
        _check_moves(gpu, gpu.semiglobal_xdrop_moves(a, b), rows, range(len(rows)), (sweep, exact))


@pytest.mark.parametrize("sweep", [41, 21, 11])
def test_results_follow_their_alignments_in_the_reversed_batch(gpu, want, switches, sweep):
    """other neighbours in every wavefront, another alignment shadowed by the spare lanes of the last one"""
    a, b, rows = want
    switches[0](sweep)
    order = list(range(len(rows)))[::-1]
    _check_moves(gpu, gpu.semiglobal_xdrop_moves(a[order], b[order]), rows, order, (sweep, "reversed"))


@pytest.mark.parametrize("sweep", [4, 2, 1])
def test_positions_entry_on_the_structured_batch(gpu, want, switches, sweep):
    a, b, rows = want
    switches[0](sweep)
    scores, tbs, lengths = gpu.semiglobal_xdrop(a, b)
    for k, (score, tb, _) in enumerate(rows):
        name = se.batch()[k].name
        assert int(scores[k]) == score and int(lengths[k]) == len(tb), (sweep, name)
        assert np.array_equal(tbs[k], tb), (sweep, name)


@pytest.mark.parametrize("sweep", [4, 2, 1])
def test_cap_next_to_the_path_length(gpu, want, switches, sweep):
    """exactly min(length, cap) leading positions, full scores and lengths, for paths of 1, 9 and 16385 positions in one call"""
    a, b, rows = want
    switches[0](sweep)
    pick = [se.index_of(name) for name in se.CAP_CASES]
    assert [len(rows[k][1]) for k in pick] == [1, 9, se.LEN + 1]
    caps = sorted({cap for k in pick for cap in se.caps_for(len(rows[k][1]))})
    assert caps == [0, 1, 2, 8, 9, 10, se.LEN, se.LEN + 1, se.LEN + 2]
    for cap in caps:
        guard = 3                                                   # rows of the caller's buffer behind the last alignment's
        tb = np.full((len(pick) + guard, max(cap, 1), 2), -7, np.int32)
        scores = np.zeros(len(pick), np.int32)
        lengths = np.zeros(len(pick), np.uint32)
        x, y = np.ascontiguousarray(a[pick]), np.ascontiguousarray(b[pick])
        rc = gpu.load().swmi_semiglobal_xdrop(x.ctypes.data, y.ctypes.data, len(pick), scores.ctypes.data, tb.ctypes.data, cap, lengths.ctypes.data)
        assert rc == 0, gpu.last_error()
        flat = tb.reshape(-1, 2)
        for j, k in enumerate(pick):
            score, path, _ = rows[k]
            assert int(scores[j]) == score and int(lengths[j]) == len(path), (sweep, cap, j)
            kept = min(len(path), cap)
            assert np.array_equal(flat[j * cap: j * cap + kept], path[:kept]), (sweep, cap, j)
        # (what stands behind a path inside its alignment's `cap` positions is unspecified; behind the last alignment's: nothing)
        assert (flat[len(pick) * cap:] == -7).all(), (sweep, cap)


def _run_one(gpu, a, b, exact):
    """one alignment in a launch of its own: (score, length, move words, windows, calm windows)"""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    d1, d2 = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    d_score = torch.empty(1, dtype=torch.int32, device=dev)
    d_len = torch.empty(1, dtype=torch.int32, device=dev)
    d_moves = torch.zeros(gpu.SG_MOVE_WORDS, dtype=torch.int64, device=dev)
    gpu.semiglobal_set_exact(exact)
    gpu.semiglobal_xdrop_moves_device(d1.data_ptr(), d2.data_ptr(), 1, d_score.data_ptr(), d_moves.data_ptr(), d_len.data_ptr(), st.cuda_stream)
    windows, calm = gpu.semiglobal_window_stats(st.cuda_stream)
    return int(d_score.cpu()[0]), int(d_len.cpu()[0]), d_moves.cpu().numpy().view(np.uint64), windows, calm


@pytest.mark.parametrize("sweep", [41, 21, 11])
def test_calm_window_count_of_one_alignment(gpu, want, profiles, switches, sweep):
    """n = 1 is ONE sweep wavefront (a grid of (n + A - 1) / A blocks of one wavefront, A = 16, 32 or 64 alignments:
    launch_semiglobal) whose spare lanes shadow the alignment, so the launch's counters are the alignment's own.  With
    m = low - (best - 70) at a window's start, as the profile has it, the kernels' predicate is
        low - max(best - 70, 1) >= 13  and  no pad or non-base among the band's characters and the next 8 of either stream,
    so: calm <= #(m >= 13), the restatement's calm windows -- the kernel may be stricter, never laxer;
        calm >= #(m >= 14) - #(windows with a pad or non-base in reach) -- 14: the kernel's threshold is one higher while the score is 0;
    and, reading the predicate as it stands, calm = #(m - [score 0] >= 13 and nothing in reach) exactly."""
    set_mapping, _ = switches
    a, b, rows = want
    set_mapping(sweep)
    assert gpu.semiglobal_kernels_for_batch(1)[0] == {41: "sg_forward_split_kernel<4, 1>", 21: "sg_forward_split_kernel<2, 1>",
                                                      11: "sg_forward_lane_kernel<1>"}[sweep]
    counted = []
    for name in se.COUNTED:
        k, p = se.index_of(name), profiles[name]
        score, tb, words = rows[k]
        s0, l0, m0, windows, calm = _run_one(gpu, a[k], b[k], False)
        s1, l1, m1, windows1, calm1 = _run_one(gpu, a[k], b[k], True)
        upper, lower = se.SgProfile.calm(p, 13), se.SgProfile.calm(p, 14) - int(p.reach.sum())
        exact = se.kernel_predicate(p, 13)
        print("%s mapping %d: windows %d (profile %d), calm %d, bounds [%d, %d], predicate %d" % (name, sweep, windows, p.windows, calm,
                                                                                              lower, upper, exact))
        assert (s0, l0) == (s1, l1) == (score, len(tb)), (name, sweep)
        assert se.same_moves(m0, words, l0) and se.same_moves(m1, words, l1), (name, sweep)
        assert windows == windows1 == p.windows, (name, sweep, windows, windows1, p.windows)
        assert calm1 == 0, (name, sweep)
        assert lower <= exact <= upper, (name, lower, exact, upper)
        if name == "non_base_periodic":
            assert 0 < calm < windows, (name, sweep, calm, windows)
        counted.append((name, calm, lower, upper, exact))
    # (every alignment is run before the counts are judged, so that a failure names all of them)
    assert not [r for r in counted if r[1] > r[3]], ("calmer than the restatement allows (name, calm, lower, upper, predicate)", sweep, counted)
    assert not [r for r in counted if r[1] < r[2]], ("less calm than the restatement demands (name, calm, lower, upper, predicate)", sweep, counted)
    assert not [r for r in counted if r[1] != r[4]], ("not the predicate as the kernels state it (name, calm, lower, upper, predicate)", sweep, counted)
