"""Helpers of the long semi-global aligners' tests (test_semiglobal_long_gpu.py, test_semiglobal_long_affine_gpu.py): one body per
check with the family as an argument.  The shapes at the kernels' stripe edges and the parameter sets are the long global
aligners' (global_long_support.py), by import; the definitions stay the two C restatements tests/native/sgfull_oracle.c and
sgfull_affine_oracle.c, which take any lengths and are compiled unchanged.

A semi-global path starts at (0, 0) and pays for its leading gap, so with a short seq1 and a positive gap the best cell sits near
the origin and no path looks at a later stripe.  The pairs here are built so that they do: gaps that cost nothing per extra column,
or a seq1 as long as the columns it has to reach.  Every check asserts, on the restatement's result, the situation it was built
for."""
import numpy as np

from global_long_support import AFFINE_PARAMS, LEN1S, LEN2S, LINEAR_PARAMS, MAX_LEN, STRIPE, plant, planted_batch  # noqa: F401
from sgfull_affine_support import SgAffineOracle
from sgfull_support import SgFullOracle, move_words, moves_to_path  # noqa: F401

DIAG, UP, LEFT = 3, 2, 1


def moves_of(moves_row, count):
    """The first `count` move codes of a row, in walking order."""
    t = np.arange(int(count))
    return ((np.asarray(moves_row, np.uint64)[t // 32] >> (2 * (t % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)


def assert_same(got, want, what, traceback=True):
    """Every field of two results equal; moves up to `lengths - 1` only (words past the last move are unspecified)."""
    sc, ends, mv, ln = got
    wsc, wends, wmv, wln = want
    assert np.array_equal(sc, wsc), (what, np.flatnonzero(sc != wsc)[:8], sc[:8], wsc[:8])
    assert ends.shape == wends.shape and np.array_equal(ends, wends), (what, np.flatnonzero((ends != wends).any(axis=1))[:8])
    if not traceback:
        return
    assert np.array_equal(ln, wln), (what, np.flatnonzero(ln != wln)[:8])
    for k in range(len(sc)):
        full, part = divmod(int(ln[k]) - 1, 32)
        assert np.array_equal(mv[k, :full], wmv[k, :full]), (what, k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (mv[k, full] & mask) == (wmv[k, full] & mask), (what, k)


def mm(match, mismatch):
    sm = np.full((4, 4), mismatch, np.int8)
    np.fill_diagonal(sm, match)
    return sm.reshape(16)


def quiet_pair(len1, len2, ends_at, seed):
    """seq1 over {0, 1}, seq2 over {2, 3} but for one exact copy of seq1 that ends on column `ends_at`: the copy holds the only
    matches of the pair."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, len1, dtype=np.uint8)
    b = rng.integers(2, 4, len2, dtype=np.uint8)
    b[ends_at - len1:ends_at] = a
    return a, b


def quiet_batch(len1, len2, seed):
    """Quiet pairs (quiet_pair) whose copy lies across column 16384 (pair 0) and, where len2 > 32768, across column 32768 (pair
    1), clipped into seq2 as global_long_support.plant clips; then planted_batch's four pairs.  Returns (seq1s, seq2s, the
    boundary of each quiet pair)."""
    rng = np.random.default_rng(seed + 1)
    bounds = [STRIPE] + ([2 * STRIPE] if len2 > 2 * STRIPE else [])
    a = rng.integers(0, 2, (len(bounds), len1), dtype=np.uint8)
    b = rng.integers(2, 4, (len(bounds), len2), dtype=np.uint8)
    for k, bound in enumerate(bounds):
        plant(b[k], a[k], bound)
    a4, b4 = planted_batch(len1, len2, seed)
    return np.concatenate([a, a4]), np.concatenate([b, b4]), bounds


def insertion_pair():
    """(16500, 16700): seq2 is seq1 with 100 random bases inserted behind column 16335 (they fill columns 16336 .. 16435, across
    the first stripe boundary), 5 % mismatches and a random tail of 100.  The inserted bases are drawn from {2, 3} and seq1's
    rows within 128 of row 16335 from {0, 1}: no inserted base can pair with a base of seq1 as a match, so a path that takes the
    insertion as ONE gap can neither break the run on a chance match nor slide it (with four letters everywhere a linear-gap
    walk, diagonal first on a tie, breaks it into a dozen pieces)."""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 4, 16500, dtype=np.uint8)
    a[16335 - 128:16335 + 128] &= 1
    noisy = np.where(rng.random(16500) < 0.05, rng.integers(0, 4, 16500), a).astype(np.uint8)
    b = np.concatenate([noisy[:16335], rng.integers(2, 4, 100, dtype=np.uint8), noisy[16335:], rng.integers(0, 4, 100, dtype=np.uint8)])
    assert len(b) == 16700
    return a[None], b[None]


def both_long_pair():
    """(33000, 33000): seq2 is a copy of seq1 with 10 % mismatches."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 33000, dtype=np.uint8)
    b = np.where(rng.random(33000) < 0.10, rng.integers(0, 4, 33000), a).astype(np.uint8)
    return a[None], b[None]


def left_runs(codes, end_j):
    """(first column, last column) of every maximal run of left moves of a walk that starts in column end_j."""
    codes = np.asarray(codes)
    col = int(end_j) - np.concatenate([[0], np.cumsum(codes != UP)])[:-1]        # the column each move leaves
    runs, t = [], 0
    while t < len(codes):
        if codes[t] == LEFT:
            u = t
            while u + 1 < len(codes) and codes[u + 1] == LEFT:
                u += 1
            runs.append((int(col[u]), int(col[t])))
            t = u + 1
        else:
            t += 1
    return runs


_PAIRS = {"insertion": insertion_pair, "both_long": both_long_pair}
_pair_cache = {}
_want_cache = {}


def pair(name):
    if name not in _pair_cache:
        _pair_cache[name] = _PAIRS[name]()
    return _pair_cache[name]


# ---- what the linear and the affine test files share: one body per check, the family as an argument -----------------------

class Family:
    """The linear (gaps = (gap,)) or the affine (gaps = (open, extend)) long semi-global aligner: its Python entries, its
    fixed-length twin, its restatement and its parameter sets."""

    def __init__(self, affine):
        self.affine = affine
        self.params = [(sm, (go, ge)) for sm, go, ge in AFFINE_PARAMS] if affine else [(sm, (g,)) for sm, g in LINEAR_PARAMS]
        self.free = self.params[4]                 # gaps cost nothing per extra column: (2, -3, 0) / (2, -3, 4, 0)
        self.name = "semiglobal_long_affine" if affine else "semiglobal_long"

    def oracle(self, tmpdir):
        return (SgAffineOracle if self.affine else SgFullOracle)(tmpdir)

    def align(self, gpu, a, b, sm, gaps, traceback=True):
        return getattr(gpu.semiglobal_long, self.name)(a, b, sm, *gaps, traceback=traceback)

    def fixed(self, gpu, a, b, sm, gaps):
        return (gpu.semiglobal_full_affine if self.affine else gpu.semiglobal_full)(a, b, sm, *gaps)

    def device(self, gpu, *args, **kw):
        return getattr(gpu.semiglobal_long, self.name + "_device")(*args, **kw)

    def release(self, gpu):
        getattr(gpu.semiglobal_long, self.name + "_release_workspaces")()

    def gaps(self, gap):
        """The gap of a hand-built linear case for this family: affine with open == extend is the linear recurrence."""
        return (gap, gap) if self.affine else (gap,)

    def want(self, oracle, name, sm, gaps):
        """The restatement's result on a named pair, computed once per family and parameter set."""
        key = (self.affine, name, bytes(np.asarray(sm, np.int8)), tuple(gaps))
        if key not in _want_cache:
            a, b = pair(name)
            _want_cache[key] = oracle.align(a, b, sm, *gaps)
        return _want_cache[key]

    def against(self, gpu, a, b, sm, gaps, want, what):
        """The host entry with traceback and ends-only against a result of the restatement."""
        assert_same(self.align(gpu, a, b, sm, gaps), want, what)
        sc, ends, mv, ln = self.align(gpu, a, b, sm, gaps, traceback=False)
        assert mv is None and ln is None
        assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)

    def both(self, gpu, oracle, a, b, sm, gaps, what):
        want = oracle.align(a, b, sm, *gaps)
        self.against(gpu, a, b, sm, gaps, want, what)
        return want

    def one(self, gpu, oracle, a, b, sm, gaps, what):
        """One pair, traceback and ends-only, bit-exact against the restatement: (score, best cell, positions, the walk's codes)
        of the restatement, for the caller's hand-worked values."""
        sc, ends, mv, ln = self.both(gpu, oracle, a[None], b[None], sm, gaps, what)
        return int(sc[0]), [int(x) for x in ends[0]], int(ln[0]), list(moves_of(mv[0], int(ln[0]) - 1))


# 1.
def check_stripe_edges(fam, gpu, oracle, len2, len1):
    """One (len2, len1) of the grid.  Under the free-extension set the quiet pairs' best cell is the end of the copy, beyond the
    pair's boundary, and the path runs back through every earlier stripe -- with one exception, worked by hand: the affine
    family at len1 = 1, where the one match (2) does not pay for opening the leading gap (4), so nothing is above 0 and the
    answer is (0, 0).  Under one positive-gap set (rotating over the shapes, all inside the domain: 127 * (257 + 65536) < 2^23)
    the leading gap never pays, the quiet pairs' best cell lies in stripe 0, and nothing from a later stripe may beat it."""
    a, b, bounds = quiet_batch(len1, len2, 1000 * LEN2S.index(len2) + len1)
    sm, gaps = fam.free
    want = fam.both(gpu, oracle, a, b, sm, gaps, (len1, len2, gaps))
    pays = 2 * len1 > (gaps[0] if fam.affine else 0)
    for k, bound in enumerate(bounds):
        if pays:
            assert int(want[1][k, 1]) > bound and int(want[1][k, 0]) == len1, (k, want[1][k])
            assert int(want[0][k]) == 2 * len1 - (gaps[0] if fam.affine else 0) and int(want[3][k]) > bound
        else:
            assert int(want[0][k]) == 0 and want[1][k].tolist() == [0, 0] and int(want[3][k]) == 1
    sm, gaps = fam.params[(LEN1S.index(len1) + LEN2S.index(len2)) % 4]
    assert gaps[0] > 0 and 127 * (len1 + len2) < 1 << 23
    want = fam.both(gpu, oracle, a, b, sm, gaps, (len1, len2, gaps))
    for k in range(len(bounds)):
        assert int(want[1][k, 1]) <= STRIPE, (k, want[1][k])


# 2.
def insertion_sets(fam):
    """Linear: (5, -4, 3) and (1, -1, 1).  Affine: open > extend, extend 0, and open < extend."""
    return [fam.params[0], fam.params[4], fam.params[1]] if fam.affine else [fam.params[1], fam.params[0]]


def check_positive_gap_across_the_boundary(fam, gpu, oracle, which):
    """The insertion pair: the best cell lies on the last rows, 100 columns further right, and the path holds a run of at
    least 100 left moves that starts right of column 16384 and ends left of it."""
    sm, gaps = insertion_sets(fam)[which]
    a, b = pair("insertion")
    want = fam.want(oracle, "insertion", sm, gaps)
    sc, ends, mv, ln = want
    assert int(ends[0, 0]) >= 16400 and int(ends[0, 1]) >= int(ends[0, 0]) + 90 and int(sc[0]) > 0, (sc, ends)
    codes = moves_of(mv[0], int(ln[0]) - 1)
    assert int((codes == LEFT).sum()) - int((codes == UP).sum()) == int(ends[0, 1]) - int(ends[0, 0])
    runs = left_runs(codes, ends[0, 1])
    assert any(hi - lo + 1 >= 100 and lo <= STRIPE < hi for lo, hi in runs), runs
    fam.against(gpu, a, b, sm, gaps, want, ("insertion", gaps))


# 3.
def both_long_set(fam):
    return fam.params[0] if fam.affine else fam.params[1]


def check_both_beyond_32768(fam, gpu, oracle):
    sm, gaps = both_long_set(fam)
    a, b = pair("both_long")
    want = fam.want(oracle, "both_long", sm, gaps)
    assert int(want[1][0, 1]) > 2 * STRIPE and int(want[1][0, 0]) > 2 * STRIPE and int(want[0][0]) > 0
    fam.against(gpu, a, b, sm, gaps, want, ("both long", gaps))


# 4.
def check_long_seq1(fam, gpu, oracle, len1, len2):
    """One stripe, a long seq1: the carry is never touched.  The extreme set is left out: 127 * (65536 + 1025) > 2^23."""
    rng = np.random.default_rng(len1)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    b[0] = a[0, len1 // 2: len1 // 2 + len2]
    assert len2 <= STRIPE
    for x in (0, 1, 3, 4):
        sm, gaps = fam.params[x]
        fam.both(gpu, oracle, a, b, sm, gaps, (len1, len2, gaps))


# 5. hand-built cases: the values are worked out in the docstrings, and the restatement has to give them too
def tie_pair():
    """seq1 = 0^60 2^80 1^60; seq2 all 3 with 1^60 at columns 9941 .. 10000 and 0^60 at 29941 .. 30000, 40000 long."""
    a = np.concatenate([np.zeros(60, np.uint8), np.full(80, 2, np.uint8), np.ones(60, np.uint8)])
    b = np.full(40000, 3, np.uint8)
    b[9940:10000] = 1
    b[29940:30000] = 0
    return a, b


def check_tie_between_stripes(fam, gpu, oracle):
    """At gap 0 both runs score 60 * 2: 1^60 ends on (200, 10000) in stripe 0, 0^60 on (60, 30000) in stripe 1.  The first cell
    in row-major order is the one in row 60, in the LATER stripe; "the earlier stripe wins" would answer (200, 10000).  That
    H(200, 10000) is 120 as well comes from the restatement on seq2[:10000]."""
    a, b = tie_pair()
    sm, gaps = mm(2, -3), fam.gaps(0)
    early = oracle.align(a[None], b[None, :10000], sm, *gaps)
    assert int(early[0][0]) == 120 and early[1][0].tolist() == [200, 10000]
    score, ends, positions, codes = fam.one(gpu, oracle, a, b, sm, gaps, "tie between stripes")
    assert score == 120 and ends == [60, 30000] and positions == 30001
    assert codes[:60] == [DIAG] * 60 and codes[60:] == [LEFT] * 29940


def check_tie_on_one_row(fam, gpu, oracle):
    """The same pair: at gap 0 H(60, j) = 120 for every j >= 30000, in stripe 1 and in stripe 2 (worked out here in numpy on rows
    0 .. 60, whose cells left of column 29941 hold 0); the earliest column wins."""
    a, b = tie_pair()
    s = np.where(a[:60, None] == b[None, :], 2, -3)
    h = np.zeros(len(b) + 1, np.int64)
    for i in range(60):
        t = np.concatenate([[0], np.maximum(h[:-1] + s[i], h[1:])])
        h = np.maximum.accumulate(t)
    assert np.all(h[30000:] == 120) and np.all(h[:30000] < 120) and len(b) > 2 * STRIPE
    score, ends, positions, _ = fam.one(gpu, oracle, a, b, mm(2, -3), fam.gaps(0), "tie on one row")
    assert score == 120 and ends == [60, 30000] and positions == 30001


def check_best_cell_on_column(fam, gpu, oracle, column, len2=17000):
    """A quiet pair at gap 0 whose copy of 80 ends on `column`: 16384 is stripe 0's carried column, 16385 stripe 1's first, and
    len2 itself the one valid column of the last stripe."""
    a, b = quiet_pair(80, len2, column, column)
    score, ends, positions, codes = fam.one(gpu, oracle, a, b, mm(2, -3), fam.gaps(0), ("best cell on", column))
    assert score == 160 and ends == [80, column] and positions == column + 1
    assert codes == [DIAG] * 80 + [LEFT] * (column - 80)


def check_forced_walk_along_row_0(fam, gpu, oracle):
    """len1 = 1, len2 = 65536, seq1's base only at column 32768, gap 0: (1, 32768) with 32769 positions, one diagonal and then
    32767 forced left moves along row 0, across two stripe boundaries."""
    a = np.zeros(1, np.uint8)
    b = np.ones(MAX_LEN, np.uint8)
    b[2 * STRIPE - 1] = 0
    score, ends, positions, codes = fam.one(gpu, oracle, a, b, mm(2, -3), fam.gaps(0), "forced walk")
    assert score == 2 and ends == [1, 2 * STRIPE] and positions == 2 * STRIPE + 1
    assert codes == [DIAG] + [LEFT] * (2 * STRIPE - 1)


def check_all_mismatch(fam, gpu, oracle):
    """(300, 20000), seq1 all 0 and seq2 all 1: nothing is above 0, so the score is 0 at (0, 0) and the path is that one cell."""
    a, b = np.zeros(300, np.uint8), np.ones(20000, np.uint8)
    for gap in (1, 0):
        score, ends, positions, codes = fam.one(gpu, oracle, a, b, mm(2, -3), fam.gaps(gap), ("all mismatch", gap))
        assert score == 0 and ends == [0, 0] and positions == 1 and codes == []


def check_walk_straddles_the_boundary(fam, gpu, oracle):
    """The insertion pair: its path crosses column 16384 on rows near 16335, inside one staging block of 128 rows whose lanes
    lie on both sides of the boundary."""
    sm, gaps = insertion_sets(fam)[0]
    a, b = pair("insertion")
    want = fam.want(oracle, "insertion", sm, gaps)
    path = moves_to_path(want[2][0], want[3][0], want[1][0, 0], want[1][0, 1])
    rows = path[(path[:, 1] >= STRIPE - 8) & (path[:, 1] <= STRIPE + 8), 0]
    assert len(rows) >= 17 and rows.max() - rows.min() < 128
    assert_same(fam.align(gpu, a, b, sm, gaps), want, "straddle")


def check_bytes_0_to_255(fam, gpu, oracle):
    """Bases are taken modulo 4: a batch of arbitrary bytes equals the batch of their low two bits."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (2, 129), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 17409), dtype=np.uint8)
    b[0, 16300:16429] = a[0]
    for sm, gaps in (fam.free, fam.params[3]):
        want = oracle.align(a & 3, b & 3, sm, *gaps)
        assert_same(fam.align(gpu, a, b, sm, gaps), want, "bytes")
    assert int(want[0].max()) >= 0


# 6.
def check_full_size(fam, gpu, match, gap):
    """65536 x 65536 in closed form.  Identical sequences: the diagonal scores 65536 match at (65536, 65536), 65537 positions,
    every move diagonal (any gap costs 2 gap and saves nothing); ends-only the same score and cell.  seq1 all 0 against seq2
    all 1: nothing is above 0, so score 0 at (0, 0) and one position, while the last cells reach the most negative keys."""
    sm, gaps = mm(match, -match), fam.gaps(gap)
    a = np.random.default_rng(9).integers(0, 4, (1, MAX_LEN), dtype=np.uint8)
    sc, ends, mv, ln = fam.align(gpu, a, a, sm, gaps)
    assert int(sc[0]) == match * MAX_LEN and ends[0].tolist() == [MAX_LEN, MAX_LEN] and int(ln[0]) == MAX_LEN + 1
    assert np.all(moves_of(mv[0], MAX_LEN) == DIAG)
    sc, ends, _, _ = fam.align(gpu, a, a, sm, gaps, traceback=False)
    assert int(sc[0]) == match * MAX_LEN and ends[0].tolist() == [MAX_LEN, MAX_LEN]
    a, b = np.zeros((1, MAX_LEN), np.uint8), np.ones((1, MAX_LEN), np.uint8)
    sc, ends, mv, ln = fam.align(gpu, a, b, sm, gaps)
    assert int(sc[0]) == 0 and ends[0].tolist() == [0, 0] and int(ln[0]) == 1
    sc, ends, _, _ = fam.align(gpu, a, b, sm, gaps, traceback=False)
    assert int(sc[0]) == 0 and ends[0].tolist() == [0, 0]


# 7.
def check_equals_fixed(fam, gpu, len1, len2):
    rng = np.random.default_rng(len1 + len2)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, :w] = np.where(rng.random(w) < 0.1, rng.integers(0, 4, w), a[0, :w])
    for sm, gaps in fam.params:
        assert_same(fam.align(gpu, a, b, sm, gaps), fam.fixed(gpu, a, b, sm, gaps), (len1, len2, gaps))


def check_global_witness(fam, gpu, oracle, name, sm, gaps):
    """A second witness from another kernel (DESIGN section 20's property): the long GLOBAL aligner on seq1[:end_i], seq2[:end_j]
    gives the same score, where (end_i, end_j) and the score are the restatement's on a pair of check 2 or 3."""
    a, b = pair(name)
    want = fam.want(oracle, name, sm, gaps)
    ei, ej = int(want[1][0, 0]), int(want[1][0, 1])
    assert ei > STRIPE and ej > STRIPE
    entry = gpu.global_long.global_long_affine if fam.affine else gpu.global_long.global_long
    sc = entry(a[:, :ei], b[:, :ej], sm, *gaps, 0, traceback=False)[0]
    assert int(sc[0]) == int(want[0][0])


# 8.
def check_host_entry_and_expand(fam, gpu, oracle):
    """n = 5 of (129, 32769), host to host with a traceback under the free-extension set; expand_moves rebuilds each path from
    (0, 0) to the best cell, and it equals the positions that the restatement's moves spell in Python."""
    a, b, _ = quiet_batch(129, 32769, 77)
    a, b = a[:5], b[:5]
    sm, gaps = fam.free
    want = oracle.align(a, b, sm, *gaps)
    got = fam.align(gpu, a, b, sm, gaps)
    assert_same(got, want, "host n = 5")
    sc, ends, mv, ln = got
    assert int(ends[0, 1]) > STRIPE
    for k in range(5):
        pos = gpu.semiglobal_long.expand_moves(mv[k], ln[k])
        assert pos.shape == (int(ln[k]), 2) and tuple(pos[0]) == (0, 0) and tuple(pos[-1]) == (int(ends[k, 0]), int(ends[k, 1]))
        assert np.array_equal(pos, moves_to_path(want[2][k], want[3][k], want[1][k, 0], want[1][k, 1]))


def check_device_entry(fam, gpu, oracle):
    """The _device entry on torch buffers, traceback and ends-only, at a shape with a carry (len2 > 16384); then release."""
    import torch
    a, b, _ = quiet_batch(64, 16400, 31)
    a, b = np.ascontiguousarray(a[:4]), np.ascontiguousarray(b[:4])
    sm, gaps = fam.free
    n, mw = 4, gpu.semiglobal_long.move_words(64, 16400)
    want = oracle.align(a, b, sm, *gaps)
    assert int(want[1][0, 1]) > STRIPE
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    ends = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda")
    ln = torch.zeros(n, dtype=torch.int32, device="cuda")
    fam.device(gpu, da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, *gaps, sc.data_ptr(), ends.data_ptr(), mv.data_ptr(), ln.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32)), want, "device")
    sc.zero_()
    ends.zero_()
    fam.device(gpu, da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, *gaps, sc.data_ptr(), ends.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), None, None), want, "device ends-only", traceback=False)
    fam.release(gpu)


def checksum(path):
    s = 0
    for i, j in path:
        s = (s * 1000003 + int(i) * 32771 + int(j)) & 0xFFFFFFFFFFFFFFFF
    return s


def check_cpp_overloads(fam, gpu, oracle, tmp_path):
    """tests/native/compat_semiglobal_long.cpp on five pairs of (129, 17409) at gap 0, where the quiet pair's path crosses the
    boundary: SemiGlobal_long_mi355x one by one and its batch form in pieces of 2 (with a fourth argument: the affine pair at
    open == extend == that gap): score, path length, best cell and a checksum of every path against the restatement."""
    import os
    import shutil
    import subprocess

    from conftest import PKG, ROOT
    assert shutil.which("g++") is not None, "g++ not available"
    exe = str(tmp_path / "compat_semiglobal_long")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_semiglobal_long.cpp"), "-o", exe, "-L", lib, "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a, b, _ = quiet_batch(129, 17409, 91)
    a, b = a[:5], b[:5]
    sm = mm(2, -3)
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.array([5, 129, 17409, 0], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(5):
            fh.write(a[k].tobytes() + b[k].tobytes())
    sc, ends, mv, ln = oracle.align(a, b, sm, *fam.gaps(0))
    assert int(ends[0, 1]) > STRIPE
    run = subprocess.run([exe, str(data), "2"] + (["0"] if fam.affine else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "single 0", lines[-1]
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == 5
    for k in range(5):
        path = moves_to_path(mv[k], ln[k], ends[k, 0], ends[k, 1])
        assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), checksum(path)), k
