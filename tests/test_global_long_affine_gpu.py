"""The long global / fit / overlap aligner with affine gaps (swmi_global_long_affine*) on the GPU, every field bit-exact against
the C restatement tests/native/global_full_affine_oracle.c, compiled unchanged (it takes any lengths).  The kernel sweeps len2
in stripes of 16384 columns and carries the last column's H and F from one stripe to the next; the shapes sit at the stripe's
and the wavefront's edges, the planted pairs' paths cross them, and the hand-built pairs put a gap across the boundary.
Moves are compared up to `steps`; words past it are unspecified."""
import numpy as np
import pytest
import torch

from conftest import match_matrix
from global_full_affine_support import (ALL_MASKS, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullAffineOracle, assert_same,
                                        moves_of, path_from)
from global_long_support import AFFINE_PARAMS, LEN1S, LEN2S, MASKS, MAX_LEN, STRIPE, crosses, planted_batch
from local_support import random_matrix

pytestmark = pytest.mark.gpu

DIAG, UP, LEFT = 3, 2, 1


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullAffineOracle(tmp_path_factory.mktemp("global_long_affine_oracle"))


def _both(gpu, oracle, a, b, sm, go, ge, mask, what):
    """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
    want = oracle.align(a, b, sm, go, ge, mask)
    assert_same(gpu.global_long.global_long_affine(a, b, sm, go, ge, mask), want, what)
    sc, ends, mv, st = gpu.global_long.global_long_affine(a, b, sm, go, ge, mask, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    return want


def _one(gpu, a, b, sm, go, ge, mask, traceback=True):
    """One pair through the host entry: (score, ends[4], codes of the walk or None)."""
    sc, ends, mv, st = gpu.global_long.global_long_affine(a[None], b[None], sm, go, ge, mask, traceback=traceback)
    return int(sc[0]), [int(x) for x in ends[0]], moves_of(mv[0], st[0]) if traceback else None


# ---- 1. stripe edges on len2 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1", LEN1S)
@pytest.mark.parametrize("len2", LEN2S)
def test_stripe_edges(gpu, oracle, len2, len1):
    """Every (len2, len1) of the grid under GLOBAL, FIT, OVERLAP and each single flag, the parameter sets rotating over the
    masks and the shapes; three planted pairs and a random one.  Some path of the case crosses column 16384, and where
    len2 > 32768 some path crosses column 32768 (asserted on the restatement's results)."""
    a, b = planted_batch(len1, len2, 1000 * LEN2S.index(len2) + len1 + 7)
    over1 = over2 = False
    for mi, mask in enumerate(MASKS):
        sm, go, ge = AFFINE_PARAMS[(mi + LEN1S.index(len1) + LEN2S.index(len2)) % len(AFFINE_PARAMS)]
        want = _both(gpu, oracle, a, b, sm, go, ge, mask, (len1, len2, mask, go, ge))
        over1 |= bool(crosses(want[1], STRIPE).any())
        over2 |= bool(crosses(want[1], 2 * STRIPE).any())
    assert over1
    assert over2 or len2 <= 2 * STRIPE


# ---- 2. long len1, one stripe; both long ----------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(16385, 17), (65536, 1025), (40000, 1024)])
def test_long_seq1_one_stripe(gpu, oracle, len1, len2):
    rng = np.random.default_rng(len1 + 1)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    b[0] = a[0, len1 // 2: len1 // 2 + len2]
    for mask, (sm, go, ge) in zip((GLOBAL, FIT, OVERLAP, END1), AFFINE_PARAMS):
        if max(int(np.abs(sm.astype(np.int64)).max()), go, ge) * (len1 + len2) > 1 << 23:
            sm, go, ge = match_matrix(5, -4), 6, 2
        _both(gpu, oracle, a, b, sm, go, ge, mask, (len1, len2, mask))


def test_both_long_overlap(gpu, oracle):
    """(20000, 40000): seq1's tail is a noisy copy of the stretch of seq2 that starts in stripe 0 and ends in stripe 2, with a
    5-base deletion."""
    rng = np.random.default_rng(15)
    a = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 40000), dtype=np.uint8)
    src = a[0, 1000:]
    noisy = np.where(rng.random(len(src)) < 0.1, rng.integers(0, 4, len(src)), src).astype(np.uint8)
    noisy = np.concatenate([noisy[:7000], noisy[7005:], rng.integers(0, 4, 5, dtype=np.uint8)])
    b[0, 15000:15000 + len(noisy)] = noisy
    want = oracle.align(a, b, match_matrix(5, -4), 6, 2, OVERLAP)
    assert crosses(want[1], STRIPE).all() and crosses(want[1], 2 * STRIPE).all()
    assert_same(gpu.global_long.global_long_affine(a, b, match_matrix(5, -4), 6, 2, OVERLAP), want, "both long")


# ---- 3. 65536 x 65536, expected values worked out here --------------------------------------------------------------------

@pytest.mark.parametrize("match,go,ge", [(1, 3, 1), (64, 64, 64)])
def test_full_size_identical_sequences(gpu, match, go, ge):
    """Identical sequences under GLOBAL: the diagonal scores 65536 match and any other path holds two gaps and fewer matches,
    so the score is 65536 match, the walk 65536 diagonal steps from (65536, 65536) to (0, 0).  P = 64: 64 * 131072 = 2^23."""
    a = np.random.default_rng(19).integers(0, 4, (1, MAX_LEN), dtype=np.uint8)
    sc, ends, mv, st = gpu.global_long.global_long_affine(a, a, match_matrix(match, -match), go, ge, GLOBAL)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, 0, 0] and int(st[0]) == MAX_LEN
    assert np.all(moves_of(mv[0], st[0]) == DIAG)
    sc, ends, _, _ = gpu.global_long.global_long_affine(a, a, match_matrix(match, -match), go, ge, GLOBAL, traceback=False)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, -1, -1]


# ---- 4. hand-built, expected values worked out here -----------------------------------------------------------------------

def test_left_run_across_the_stripe_boundary(gpu):
    """seq2 = seq1 with 200 foreign bases inserted after base 100, the insert over columns 16285 .. 16484, behind a prefix
    that seq1 lacks (FIT frees it).  seq1 holds only 0 / 1, the rest only 2 / 3.  One gap of 200: 200 * 5 - (9 + 199 * 1);
    F runs through the carry for 100 columns."""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 2, 200, dtype=np.uint8)
    b = np.concatenate([rng.integers(2, 4, 16184, dtype=np.uint8), s[:100], rng.integers(2, 4, 200, dtype=np.uint8), s[100:],
                        rng.integers(2, 4, 300, dtype=np.uint8)])
    score, ends, codes = _one(gpu, s, b, match_matrix(5, -4), 9, 1, FIT)
    assert score == 1000 - 208 and ends == [200, 16584, 0, 16184]
    assert list(codes) == [DIAG] * 100 + [LEFT] * 200 + [DIAG] * 100


def test_up_run_across_row_256_in_stripe_1(gpu):
    """seq1 = 200 bases, 120 foreign ones, 200 bases; seq2 holds the 400 from column 17001 on.  Under FIT: 200 diagonals, one
    gap of 120 up moves over rows 201 .. 320, 200 diagonals: 400 * 5 - (9 + 119)."""
    rng = np.random.default_rng(4)
    s = rng.integers(0, 2, 400, dtype=np.uint8)
    a = np.concatenate([s[:200], rng.integers(2, 4, 120, dtype=np.uint8), s[200:]])
    b = np.concatenate([rng.integers(2, 4, 17000, dtype=np.uint8), s, rng.integers(2, 4, 50, dtype=np.uint8)])
    score, ends, codes = _one(gpu, a, b, match_matrix(5, -4), 9, 1, FIT)
    assert score == 2000 - 128 and ends == [520, 17400, 0, 17000]
    assert list(codes) == [DIAG] * 200 + [UP] * 120 + [DIAG] * 200


@pytest.mark.parametrize("first", [16384, 16385])
@pytest.mark.parametrize("go,ge", [(7, 2), (2, 7)])
def test_gap_that_opens_at_the_boundary(gpu, first, go, ge):
    """A 3-base insert in seq2 whose first column is 16384 -- the gap opens in stripe 0 and extends into stripe 1, F carried
    across -- or 16385, where it opens in stripe 1 from the carried H.  40 diagonals, 3 left moves, 40 diagonals under FIT.
    With open > extend it is one gap, open + 2 extend; with open < extend the recurrences reopen, 3 open."""
    rng = np.random.default_rng(first)
    s = rng.integers(0, 2, 80, dtype=np.uint8)
    b = np.concatenate([rng.integers(2, 4, first - 41, dtype=np.uint8), s[:40], rng.integers(2, 4, 3, dtype=np.uint8), s[40:],
                        rng.integers(2, 4, 64, dtype=np.uint8)])
    score, ends, codes = _one(gpu, s, b, match_matrix(5, -4), go, ge, FIT)
    assert score == 400 - (go + 2 * min(go, ge)) and ends == [80, first + 42, 0, first - 41]
    assert list(codes) == [DIAG] * 40 + [LEFT] * 3 + [DIAG] * 40


@pytest.mark.parametrize("go,ge", [(4, 2), (0, 0)])
def test_end2_tie_between_stripes_goes_to_the_earlier_column(gpu, go, ge):
    """seq2 holds seq1 twice, ending at column 10000 (stripe 0) and at column 30000 (stripe 1), in a background that seq1
    lacks: under FIT both last-row cells hold 60 * 3 and nothing exceeds it, so the end cell is (60, 10000) -- also with free
    gaps, where 180 fills the last row right of it."""
    s = np.random.default_rng(6).integers(0, 2, 60, dtype=np.uint8)
    b = np.full(40000, 3, np.uint8)
    b[9940:10000] = s
    b[29940:30000] = s
    score, ends, codes = _one(gpu, s, b, match_matrix(3, -3), go, ge, FIT)
    assert score == 180 and ends == [60, 10000, 0, 9940] and list(codes) == [DIAG] * 60
    score, ends, _ = _one(gpu, s, b, match_matrix(3, -3), go, ge, FIT, traceback=False)
    assert score == 180 and ends[:2] == [60, 10000]


@pytest.mark.parametrize("len2", [16385, 17409])
def test_end1_best_row_in_a_last_stripe_of_one_column(gpu, len2):
    """The last column is the only valid one of the last stripe (16385) or of its last wavefront (17409).  seq1 = 50 bases
    that end a seq2 of foreign bases, then 30 foreign bases: with END1 | BEGIN2 the best cell of the last column is row 50."""
    s = np.random.default_rng(len2).integers(0, 2, 50, dtype=np.uint8)
    a = np.concatenate([s, np.full(30, 2, np.uint8)])
    b = np.full(len2, 3, np.uint8)
    b[len2 - 50:] = s
    score, ends, codes = _one(gpu, a, b, match_matrix(4, -5), 5, 3, END1 | BEGIN2)
    assert score == 200 and ends == [50, len2, 0, len2 - 50] and list(codes) == [DIAG] * 50


def test_walk_whose_staging_blocks_straddle_the_boundary(gpu, oracle):
    """A 3000-base noisy copy across column 16384 under FIT: the walk crosses the boundary inside a staging block of 128 rows x
    512 columns and takes more than 20 blocks."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 4, (1, 3000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b[0, 14900:17900] = np.where(rng.random(3000) < 0.1, rng.integers(0, 4, 3000), a[0])
    want = oracle.align(a, b, match_matrix(5, -4), 6, 2, FIT)
    assert crosses(want[1], STRIPE).all() and int(want[3][0]) > 2 * 1024
    assert_same(gpu.global_long.global_long_affine(a, b, match_matrix(5, -4), 6, 2, FIT), want, "straddle")


def test_border_end_cells_under_overlap(gpu):
    """All-mismatch pairs under OVERLAP: every inner cell is negative and the border holds 0, so the end cell is the first
    border end cell in row-major order, (0, len2), with an empty walk."""
    for len1, len2 in ((40, 16385), (300, 33000)):
        a, b = np.zeros(len1, np.uint8), np.ones(len2, np.uint8)
        score, ends, codes = _one(gpu, a, b, match_matrix(2, -3), 2, 1, OVERLAP)
        assert score == 0 and ends == [0, len2, 0, len2] and len(codes) == 0
    a, b = np.zeros(40, np.uint8), np.ones(16385, np.uint8)
    score, ends, codes = _one(gpu, a, b, match_matrix(2, -3), 2, 1, END2 | 1)
    assert score == 0 and ends == [40, 0, 40, 0] and len(codes) == 0


def test_bytes_0_to_255(gpu, oracle):
    """Bases are taken modulo 4: a batch of arbitrary bytes equals the batch of their low two bits."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (2, 129), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 17409), dtype=np.uint8)
    b[0, 16300:16429] = a[0]
    want = oracle.align(a & 3, b & 3, random_matrix(), 11, 2, FIT)
    assert_same(gpu.global_long.global_long_affine(a, b, random_matrix(), 11, 2, FIT), want, "bytes")


# ---- 5. ties to the existing entries --------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(300, 16384), (16384, 300), (1000, 5000)])
def test_equals_the_fixed_entry_where_both_reach(gpu, len1, len2):
    rng = np.random.default_rng(len1 + len2 + 1)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, len2 - w:] = np.where(rng.random(w) < 0.1, rng.integers(0, 4, w), a[0, len1 - w:])
    for mask in ALL_MASKS:
        sm, go, ge = AFFINE_PARAMS[mask % len(AFFINE_PARAMS)]
        assert_same(gpu.global_long.global_long_affine(a, b, sm, go, ge, mask),
                    gpu.global_affine.global_full_affine(a, b, sm, go, ge, mask), (len1, len2, mask))


def test_open_equal_to_extend_is_the_linear_entry(gpu):
    """(257, 32769): with gap_open == gap_extend == g every field equals swmi_global_long's with gap g, under every mask."""
    a, b = planted_batch(257, 32769, 55)
    for mask in ALL_MASKS:
        assert_same(gpu.global_long.global_long_affine(a, b, match_matrix(5, -4), 3, 3, mask),
                    gpu.global_long.global_long(a, b, match_matrix(5, -4), 3, mask), mask)


# ---- 6. the host entry across alignments, and the expander ----------------------------------------------------------------

def test_host_entry_and_expand_moves(gpu, oracle):
    """n = 5 of (129, 32769), host to host with a traceback; expand_moves rebuilds each path from its start cell to its end."""
    a4, b4 = planted_batch(129, 32769, 78)
    a, b = np.concatenate([a4, a4[:1]]), np.concatenate([b4, b4[1:2]])
    want = oracle.align(a, b, match_matrix(5, -4), 6, 2, FIT)
    got = gpu.global_long.global_long_affine(a, b, match_matrix(5, -4), 6, 2, FIT)
    assert_same(got, want, "host n = 5")
    sc, ends, mv, st = got
    for k in range(5):
        pos = gpu.global_long.expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1])
        assert tuple(pos[0]) == (int(ends[k, 2]), int(ends[k, 3])) and tuple(pos[-1]) == (int(ends[k, 0]), int(ends[k, 1]))
        assert np.array_equal(pos, path_from(mv[k], st[k], ends[k, 0], ends[k, 1]))


def test_device_entry_on_resident_buffers(gpu, oracle):
    """The _device entry on torch buffers, traceback and ends-only, at a shape with a carry (len2 > 16384)."""
    a, b = planted_batch(64, 16400, 32)
    n, mw = 4, gpu.global_long.move_words(64, 16400)
    sm = match_matrix(1, -1)
    want = oracle.align(a, b, sm, 3, 1, OVERLAP)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    ends = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu.global_long.global_long_affine_device(da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, 3, 1, OVERLAP, sc.data_ptr(),
                                              ends.data_ptr(), mv.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32)), want, "device")
    gpu.global_long.global_long_affine_device(da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, 3, 1, OVERLAP, sc.data_ptr(),
                                              ends.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), None, None), want, "device ends-only", traceback=False)
    gpu.global_long.global_long_affine_release_workspaces()
