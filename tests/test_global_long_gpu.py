"""The long global / fit / overlap aligner (swmi_global_long*) on the GPU, every field bit-exact against the C restatement
tests/native/global_full_oracle.c, compiled unchanged (it takes any lengths).  The kernel sweeps len2 in stripes of 16384
columns (16 wavefronts of 1024); the shapes sit at the stripe's and the wavefront's edges, and the planted pairs' paths cross
them.  Moves are compared up to `steps`; words past it are unspecified."""
import numpy as np
import pytest
import torch

from conftest import match_matrix
from global_full_support import ALL_MASKS, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP, GlobalFullOracle, assert_same, moves_of, path_from
from global_long_support import LEN1S, LEN2S, LINEAR_PARAMS, MASKS, MAX_LEN, STRIPE, crosses, planted_batch
from local_support import random_matrix

pytestmark = pytest.mark.gpu

DIAG, UP, LEFT = 3, 2, 1
K111 = match_matrix(1, -1)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return GlobalFullOracle(tmp_path_factory.mktemp("global_long_oracle"))


def _both(gpu, oracle, a, b, sm, gap, mask, what):
    """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
    want = oracle.align(a, b, sm, gap, mask)
    assert_same(gpu.global_long.global_long(a, b, sm, gap, mask), want, what)
    sc, ends, mv, st = gpu.global_long.global_long(a, b, sm, gap, mask, traceback=False)
    assert mv is None and st is None
    assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
    return want


def _one(gpu, a, b, sm, gap, mask, traceback=True):
    """One pair through the host entry: (score, ends[4], codes of the walk or None)."""
    sc, ends, mv, st = gpu.global_long.global_long(a[None], b[None], sm, gap, mask, traceback=traceback)
    return int(sc[0]), [int(x) for x in ends[0]], moves_of(mv[0], st[0]) if traceback else None


# ---- 1. stripe edges on len2 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1", LEN1S)
@pytest.mark.parametrize("len2", LEN2S)
def test_stripe_edges(gpu, oracle, len2, len1):
    """Every (len2, len1) of the grid under GLOBAL, FIT, OVERLAP and each single flag, the parameter sets rotating over the
    masks and the shapes; three planted pairs and a random one.  Some path of the case crosses column 16384, and where
    len2 > 32768 some path crosses column 32768 (asserted on the restatement's results)."""
    a, b = planted_batch(len1, len2, 1000 * LEN2S.index(len2) + len1)
    over1 = over2 = False
    for mi, mask in enumerate(MASKS):
        sm, gap = LINEAR_PARAMS[(mi + LEN1S.index(len1) + LEN2S.index(len2)) % len(LINEAR_PARAMS)]
        want = _both(gpu, oracle, a, b, sm, gap, mask, (len1, len2, mask, gap))
        over1 |= bool(crosses(want[1], STRIPE).any())
        over2 |= bool(crosses(want[1], 2 * STRIPE).any())
    assert over1
    assert over2 or len2 <= 2 * STRIPE


# ---- 2. long len1, one stripe; both long ----------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(16385, 17), (65536, 1025), (40000, 1024)])
def test_long_seq1_one_stripe(gpu, oracle, len1, len2):
    rng = np.random.default_rng(len1)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    b[0] = a[0, len1 // 2: len1 // 2 + len2]
    for mask, (sm, gap) in zip((GLOBAL, FIT, OVERLAP, END1), LINEAR_PARAMS):
        if max(int(np.abs(sm.astype(np.int64)).max()), gap) * (len1 + len2) > 1 << 23:
            sm, gap = match_matrix(5, -4), 3
        _both(gpu, oracle, a, b, sm, gap, mask, (len1, len2, mask))


def test_both_long_overlap(gpu, oracle):
    """(20000, 40000): seq1's tail is a noisy copy of the stretch of seq2 that starts in stripe 0 and ends in stripe 2."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 40000), dtype=np.uint8)
    src = a[0, 1000:]
    noisy = np.where(rng.random(len(src)) < 0.1, rng.integers(0, 4, len(src)), src).astype(np.uint8)
    noisy = np.concatenate([noisy[:7000], noisy[7005:], rng.integers(0, 4, 5, dtype=np.uint8)])
    b[0, 15000:15000 + len(noisy)] = noisy
    want = oracle.align(a, b, match_matrix(5, -4), 3, OVERLAP)
    assert crosses(want[1], STRIPE).all() and crosses(want[1], 2 * STRIPE).all()
    assert_same(gpu.global_long.global_long(a, b, match_matrix(5, -4), 3, OVERLAP), want, "both long")


# ---- 3. 65536 x 65536, expected values worked out here --------------------------------------------------------------------

@pytest.mark.parametrize("match,gap", [(1, 1), (64, 64)])
def test_full_size_identical_sequences(gpu, match, gap):
    """Identical sequences under GLOBAL: the diagonal scores 65536 match and any other path loses at least 2 gap + a match, so
    the score is 65536 match, the walk 65536 diagonal steps from (65536, 65536) to (0, 0).  P = 64: 64 * 131072 = 2^23."""
    a = np.random.default_rng(9).integers(0, 4, (1, MAX_LEN), dtype=np.uint8)
    sc, ends, mv, st = gpu.global_long.global_long(a, a, match_matrix(match, -match), gap, GLOBAL)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, 0, 0] and int(st[0]) == MAX_LEN
    assert np.all(moves_of(mv[0], st[0]) == DIAG)
    sc, ends, _, _ = gpu.global_long.global_long(a, a, match_matrix(match, -match), gap, GLOBAL, traceback=False)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, -1, -1]


# ---- 4. hand-built, expected values worked out here -----------------------------------------------------------------------

def _homopolymers(len1, len2):
    """seq1 all 0, seq2 all 1: every pair of bases mismatches."""
    return np.zeros(len1, np.uint8), np.ones(len2, np.uint8)


def test_left_run_across_the_stripe_boundary(gpu):
    """seq2 = seq1 with 200 foreign bases inserted after base 100, so that the insert covers columns 16285 .. 16484 of a seq2
    whose first 16184 bases seq1 lacks (FIT frees them): matches 5, mismatches -4, gap 1.  seq1 holds only 0 / 1, the insert
    and the prefix only 2 / 3, so no diagonal can enter them; the path is 100 diagonals, 200 left moves across column 16384,
    100 diagonals, and scores 200 * 5 - 200."""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 2, 200, dtype=np.uint8)
    pre = rng.integers(2, 4, 16184, dtype=np.uint8)
    ins = rng.integers(2, 4, 200, dtype=np.uint8)
    tail = rng.integers(2, 4, 300, dtype=np.uint8)
    b = np.concatenate([pre, s[:100], ins, s[100:], tail])
    score, ends, codes = _one(gpu, s, b, match_matrix(5, -4), 1, FIT)
    assert score == 800 and ends == [200, 16584, 0, 16184]
    assert list(codes) == [DIAG] * 100 + [LEFT] * 200 + [DIAG] * 100


def test_up_run_across_row_256_in_stripe_1(gpu):
    """seq1 = 200 bases, 120 foreign ones, 200 bases; seq2 holds the 400 without the foreign ones from column 17001 on
    (stripe 1, behind a prefix that seq1 lacks): under FIT the path is 200 diagonals, 120 up moves over rows 201 .. 320,
    200 diagonals: 400 * 5 - 120."""
    rng = np.random.default_rng(4)
    s = rng.integers(0, 2, 400, dtype=np.uint8)
    a = np.concatenate([s[:200], rng.integers(2, 4, 120, dtype=np.uint8), s[200:]])
    b = np.concatenate([rng.integers(2, 4, 17000, dtype=np.uint8), s, rng.integers(2, 4, 50, dtype=np.uint8)])
    score, ends, codes = _one(gpu, a, b, match_matrix(5, -4), 1, FIT)
    assert score == 2000 - 120 and ends == [520, 17400, 0, 17000]
    assert list(codes) == [DIAG] * 200 + [UP] * 120 + [DIAG] * 200


@pytest.mark.parametrize("first", [16384, 16385])
def test_gap_that_opens_at_the_boundary(gpu, first):
    """A 3-base insert in seq2 whose first column is 16384 (it extends into stripe 1) or 16385 (it opens there): 40 diagonals,
    3 left moves, 40 diagonals under FIT, 80 * 5 - 3 * 2."""
    rng = np.random.default_rng(first)
    s = rng.integers(0, 2, 80, dtype=np.uint8)
    b = np.concatenate([rng.integers(2, 4, first - 41, dtype=np.uint8), s[:40], rng.integers(2, 4, 3, dtype=np.uint8), s[40:],
                        rng.integers(2, 4, 64, dtype=np.uint8)])
    score, ends, codes = _one(gpu, s, b, match_matrix(5, -4), 2, FIT)
    assert score == 394 and ends == [80, first + 42, 0, first - 41]
    assert list(codes) == [DIAG] * 40 + [LEFT] * 3 + [DIAG] * 40


@pytest.mark.parametrize("gap", [2, 0])
def test_end2_tie_between_stripes_goes_to_the_earlier_column(gpu, gap):
    """seq2 holds seq1 twice, ending at column 10000 (stripe 0) and at column 30000 (stripe 1), in a background that seq1
    lacks: under FIT both last-row cells hold 60 * 3 and nothing exceeds it, so the end cell is (60, 10000); with gap 0 the
    value 180 also fills the last row right of column 10000 and the first such cell still wins."""
    s = np.random.default_rng(6).integers(0, 2, 60, dtype=np.uint8)
    b = np.full(40000, 3, np.uint8)
    b[9940:10000] = s
    b[29940:30000] = s
    score, ends, codes = _one(gpu, s, b, match_matrix(3, -3), gap, FIT)
    assert score == 180 and ends == [60, 10000, 0, 9940] and list(codes) == [DIAG] * 60
    score, ends, _ = _one(gpu, s, b, match_matrix(3, -3), gap, FIT, traceback=False)
    assert score == 180 and ends[:2] == [60, 10000]


@pytest.mark.parametrize("len2", [16385, 17409])
def test_end1_best_row_in_a_last_stripe_of_one_column(gpu, len2):
    """The last column is the only valid one of the last stripe (16385) or of its last wavefront (17409).  seq1 = 50 bases
    that end a seq2 of foreign bases, then 30 foreign bases: with END1 | BEGIN2 the best cell of the last column is row 50
    (50 * 4), and the rows below lose a gap each."""
    s = np.random.default_rng(len2).integers(0, 2, 50, dtype=np.uint8)
    a = np.concatenate([s, np.full(30, 2, np.uint8)])
    b = np.full(len2, 3, np.uint8)
    b[len2 - 50:] = s
    score, ends, codes = _one(gpu, a, b, match_matrix(4, -5), 3, END1 | BEGIN2)
    assert score == 200 and ends == [50, len2, 0, len2 - 50] and list(codes) == [DIAG] * 50


def test_walk_whose_staging_blocks_straddle_the_boundary(gpu, oracle):
    """A 3000-base noisy copy across column 16384 under FIT: the walk crosses the boundary inside a staging block of 128 rows x
    1024 columns and takes more than 20 blocks."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 4, (1, 3000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b[0, 14900:17900] = np.where(rng.random(3000) < 0.1, rng.integers(0, 4, 3000), a[0])
    want = oracle.align(a, b, match_matrix(5, -4), 3, FIT)
    assert crosses(want[1], STRIPE).all() and int(want[3][0]) > 2 * 1024
    assert_same(gpu.global_long.global_long(a, b, match_matrix(5, -4), 3, FIT), want, "straddle")


def test_border_end_cells_under_overlap(gpu):
    """All-mismatch pairs under OVERLAP: every inner cell is negative and the border holds 0, so the end cell is the first
    border end cell in row-major order, (0, len2), with an empty walk; with seq1 longer it is still (0, len2)."""
    for len1, len2 in ((40, 16385), (300, 33000)):
        a, b = _homopolymers(len1, len2)
        score, ends, codes = _one(gpu, a, b, match_matrix(2, -3), 1, OVERLAP)
        assert score == 0 and ends == [0, len2, 0, len2] and len(codes) == 0
    # only seq2's end free: (len1, 0) is the one border end cell, reached by nothing but itself
    a, b = _homopolymers(40, 16385)
    score, ends, codes = _one(gpu, a, b, match_matrix(2, -3), 1, END2 | 1)
    assert score == 0 and ends == [40, 0, 40, 0] and len(codes) == 0


def test_bytes_0_to_255(gpu, oracle):
    """Bases are taken modulo 4: a batch of arbitrary bytes equals the batch of their low two bits."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (2, 129), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 17409), dtype=np.uint8)
    b[0, 16300:16429] = a[0]
    want = oracle.align(a & 3, b & 3, random_matrix(), 7, FIT)
    assert_same(gpu.global_long.global_long(a, b, random_matrix(), 7, FIT), want, "bytes")


# ---- 5. ties to the fixed-length entry ------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(300, 16384), (16384, 300), (1000, 5000)])
def test_equals_the_fixed_entry_where_both_reach(gpu, len1, len2):
    rng = np.random.default_rng(len1 + len2)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, len2 - w:] = np.where(rng.random(w) < 0.1, rng.integers(0, 4, w), a[0, len1 - w:])
    for mask in ALL_MASKS:
        sm, gap = LINEAR_PARAMS[mask % len(LINEAR_PARAMS)]
        assert_same(gpu.global_long.global_long(a, b, sm, gap, mask), gpu.global_full(a, b, sm, gap, mask), (len1, len2, mask))


# ---- 6. the host entry across alignments, and the expander ----------------------------------------------------------------

def test_host_entry_and_expand_moves(gpu, oracle):
    """n = 5 of (129, 32769), host to host with a traceback; expand_moves rebuilds each path from its start cell to its end
    cell, and the path equals the one the moves spell in numpy."""
    a4, b4 = planted_batch(129, 32769, 77)
    a, b = np.concatenate([a4, a4[:1]]), np.concatenate([b4, b4[1:2]])
    want = oracle.align(a, b, match_matrix(5, -4), 3, FIT)
    got = gpu.global_long.global_long(a, b, match_matrix(5, -4), 3, FIT)
    assert_same(got, want, "host n = 5")
    sc, ends, mv, st = got
    for k in range(5):
        pos = gpu.global_long.expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1])
        assert pos.shape == (int(st[k]) + 1, 2)
        assert tuple(pos[0]) == (int(ends[k, 2]), int(ends[k, 3])) and tuple(pos[-1]) == (int(ends[k, 0]), int(ends[k, 1]))
        assert np.array_equal(pos, path_from(mv[k], st[k], ends[k, 0], ends[k, 1]))


def test_device_entry_on_resident_buffers(gpu, oracle):
    """The _device entry on torch buffers, traceback and ends-only, at a shape with a carry (len2 > 16384)."""
    a, b = planted_batch(64, 16400, 31)
    n, mw = 4, gpu.global_long.move_words(64, 16400)
    want = oracle.align(a, b, K111, 1, OVERLAP)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    ends = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu.global_long.global_long_device(da.data_ptr(), 64, db.data_ptr(), 16400, n, K111, 1, OVERLAP, sc.data_ptr(), ends.data_ptr(),
                                       mv.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32)), want, "device")
    gpu.global_long.global_long_device(da.data_ptr(), 64, db.data_ptr(), 16400, n, K111, 1, OVERLAP, sc.data_ptr(), ends.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), None, None), want, "device ends-only", traceback=False)
    gpu.global_long.global_long_release_workspaces()


# ---- 7. the C++ overloads -------------------------------------------------------------------------------------------------

def _checksum(path):
    s = 0
    for i, j in path:
        s = (s * 1000003 + int(i) * 32771 + int(j)) & 0xFFFFFFFFFFFFFFFF
    return s


def test_cpp_overloads(gpu, oracle, tmp_path):
    """NeedlemanWunsch_long_mi355x, its batch form in pieces of 2, and the affine pair at open == extend (the linear results),
    on five pairs of (129, 17409): score, path length, end cell and a checksum of every path against the restatement."""
    import os
    import shutil
    import subprocess

    from conftest import PKG, ROOT
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "compat_global_long")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_global_long.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a4, b4 = planted_batch(129, 17409, 91)
    a, b = np.concatenate([a4, a4[:1]]), np.concatenate([b4, b4[1:2]])
    sm = random_matrix()
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.array([5, 129, 17409, 3], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(5):
            fh.write(a[k].tobytes() + b[k].tobytes())
    sc, ends, mv, st = oracle.align(a, b, sm, 3, FIT)
    for extra in ([], ["3"]):
        run = subprocess.run([exe, str(data), str(FIT), "2"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert run.returncode == 0, run.stderr
        lines = run.stdout.strip().splitlines()
        assert lines[-2:] == ["single 0", "ragged 1"], lines[-2:]
        rows = [tuple(map(int, line.split())) for line in lines[:-2]]
        assert len(rows) == 5
        for k in range(5):
            path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
            assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), _checksum(path)), (extra, k)
