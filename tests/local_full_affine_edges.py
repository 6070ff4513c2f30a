"""Hand-built inputs for the any-length affine local aligner (csrc/local_full_affine_kernels.hip), each
with the fields worked out here, and the length grid derived from the kernel's constants.  Shared by
test_local_full_affine_edges_cpu.py (every expected field and every claimed edge checked through the C restatement and the
numpy tables, no device) and test_local_full_affine_gpu.py (every field bit-exact on the GPU).

Background of most cases: seq1 all 0, seq2 all 1, so nothing matches but what a case plants with bases 2 and 3."""
import numpy as np

import affine_edges as ae
import table_edges as te
from conftest import match_matrix
from local_support import random_matrix

KC = te.kernel_constants("local_full_affine_kernels.hip")
COLS = KC["kCols"]                                       # 16 columns per lane
WAVE_COLS = te.WAVE * COLS                               # 1024 columns per wavefront
MAX_LEN = WAVE_COLS * KC["kMaxWaves"]                    # 16384
STAGE_ROWS = KC["kStageRows"]                            # 128
STAGE_COLS = KC["kStageLanes"] * COLS                    # 512
RING = KC["kRing"]                                       # 256
DIAG, UP, LEFT = 3, 2, 1
K111 = match_matrix(1, -1)
K54 = match_matrix(5, -4)
K23 = match_matrix(2, -3)
K10 = match_matrix(10, -10)


class Hand:
    """One alignment with what it must give: score, ends = (end_i, end_j, start_i, start_j) and, where the path is pinned,
    its walking-order move codes (None: only the restatement decides the moves).  claims: predicates of affine_edges that
    the numpy tables must confirm for it (CPU test)."""

    def __init__(self, name, a, b, sm, gap_open, gap_extend, score, ends, codes=None, claims=()):
        self.name, self.sm, self.gap_open, self.gap_extend = name, np.asarray(sm, np.int8), int(gap_open), int(gap_extend)
        self.a, self.b = np.ascontiguousarray(a, np.uint8).reshape(1, -1), np.ascontiguousarray(b, np.uint8).reshape(1, -1)
        self.score, self.ends, self.codes, self.claims = int(score), tuple(int(x) for x in ends), codes, tuple(claims)

    @property
    def shape(self):
        return self.a.shape[1], self.b.shape[1]

    def __repr__(self):
        return "%s %dx%d open=%d extend=%d" % (self.name, self.a.shape[1], self.b.shape[1], self.gap_open, self.gap_extend)


def _background(len1, len2):
    return np.zeros(len1, np.uint8), np.ones(len2, np.uint8)


# ---- the length grid -----------------------------------------------------------------------------------------------------

def shape_grid():
    """[(len1, len2)]: len2 at the wavefront edges W * 1024 - 1 / W * 1024 / W * 1024 + 1 for W = 1, 2, one valid column in
    the last of kMaxWaves wavefronts and all of them full (len2 mod 16 in 15 / 0 / 1 along the way); len1 around the trip,
    the chunk, lane 63's delay, the staging block, the ring and the longest sequence; and shapes past one wavefront and
    several staging blocks both ways."""
    w, last = WAVE_COLS, WAVE_COLS * (KC["kMaxWaves"] - 1) + 1
    u, c, s, r = KC["kUnroll"], KC["kChunk"], STAGE_ROWS, RING
    return [(1, 1), (1, MAX_LEN), (MAX_LEN, 1), (2, 3),
            (u - 1, w - 1), (u, w), (u + 1, w + 1),
            (c - 1, 2 * w), (c, 2 * w + 1), (c + 1, last), (te.WAVE, MAX_LEN),
            (te.WAVE - 1, 2 * w - 1), (te.WAVE + 1, w + COLS + 1), (s - 1, w + COLS), (s, w - 1), (s + 1, 2 * w + 1),
            (r - 1, w + 1), (r, 2 * w), (r + 1, w),
            (1500, 2100), (2 * w, 2 * w + 1), (1100, last), (MAX_LEN, MAX_LEN)]


def grid_params(index):
    """extend < open, open < extend with an asymmetric matrix, one of (0, 0), (5, 0), (0, 5) in turn, and every PARAMS
    matrix with a gap pair of its own"""
    from local_support import PARAMS
    go, ge = ae.ZERO_GAPS[index % 3]
    sets = [(K23, 11, 1), (random_matrix(3), 3, 7), (K54, go, ge)]
    gaps = [(15, 2), (3, 1), (4, 0), (127, 3), (5, 5)]
    return sets + [(match_matrix(m, x), o, e) for (m, x, _), (o, e) in zip(PARAMS, gaps)]


def assert_grid_edges(sc, ends, st, what):
    """what the grid's inputs (local_full_affine_support.inputs: every third pair planted, every seventh a homopolymer) must
    give at shapes past one wavefront both ways: a planted path that crosses a multiple of 1024 columns, and a path longer
    than a staging block is wide"""
    planted = [k for k in range(0, len(sc), 3) if k % 7 != 1]
    crossing = [k for k in planted if int(ends[k, 3]) // WAVE_COLS < int(ends[k, 1]) // WAVE_COLS]
    assert crossing, (what, ends[planted])
    assert int(st.max()) > STAGE_COLS, what


# ---- the floor -----------------------------------------------------------------------------------------------------------

def floor_cases():
    """A match (+1), a mismatch (-1), then 40 matches: the cell after the mismatch holds 0 and its diagonal candidate is 0
    too.  The floor wins: the path starts at that cell.  c0 = 1022 puts the tie cell in column 1024, the last of wave 0.
    Then tie_floor_gap: with open = 0 the cell above a start cell holds 0, so E = 0 where H = 0 (and F likewise)."""
    out = []
    L = 40
    P = np.random.default_rng(5).integers(2, 4, L).astype(np.uint8)
    for r0, c0 in ((0, 0), (7, 1020), (200, 3070), (30, WAVE_COLS - 2)):
        a, b = _background(r0 + L + 30, c0 + L + 50)
        a[r0:r0 + 2 + L] = np.concatenate([[2, 0], P])
        b[c0:c0 + 2 + L] = np.concatenate([[2, 1], P])
        for go, ge in ((3, 1), (1, 1)):
            out.append(Hand("floor_diag/%d,%d/%d,%d" % (r0, c0, go, ge), a, b, K111, go, ge, L,
                            (r0 + 2 + L, c0 + 2 + L, r0 + 2, c0 + 2), [DIAG] * L, ("tie_floor_diag",)))
    # a block of 20 matches (homopolymer 2 on 2) at open = 0: its score 100 first at the block's far corner (later cells of
    # that row and below only repeat it), the walk's 20 diagonals end on (r0, c0), where H = 0 = E = F
    L = 20
    for r0, c0, ge in ((50, 100, 0), (50, 1500, 5), (3, WAVE_COLS, 0)):
        a, b = _background(r0 + L + 40, c0 + L + 60)
        a[r0:r0 + L] = 2
        b[c0:c0 + L] = 2
        out.append(Hand("floor_gap/%d,%d/0,%d" % (r0, c0, ge), a, b, K54, 0, ge, 5 * L, (r0 + L, c0 + L, r0, c0), [DIAG] * L,
                        ("tie_floor_gap",)))
    return out


# ---- carried state and long runs ------------------------------------------------------------------------------------------

def _run_pair(rng, x, r, y, up):
    """seq1 = 2 + X + R + Y, seq2 = 3 + X + Y (up = True: an up run of r inside E) or the other way round (a left run inside
    F); X and Y of {0, 1}, R of {2, 3} but X's last base wherever the walk enters a staging block inside the run (every row
    = len1 mod 16, every column = 0 mod 16: a superset), where the diagonal then ties with the gap and H's own code says
    diagonal.  The leading 2 / 3 mismatch, so the walk stops on a stop code at (1, 1)."""
    X, Y, R = te._lo(rng, x), te._lo(rng, y), te._hi(rng, r)
    at = 2 + x + np.arange(r - 1)                         # the row (column) of R[t], 1-based
    R[:-1][(at - ((2 + x + r + y - 1) if up else 0)) % COLS == 0] = X[-1]
    long_, short = np.concatenate([[2], X, R, Y]), np.concatenate([[3], X, Y])
    return (long_, short) if up else (short, long_)


CARRIED_F_RUNS = ((700, 520, 600, 10), (1800, 600, 400, 10), (2300, 2100, 1300, 10))


def carried_cases(f_runs=CARRIED_F_RUNS):
    """f_runs: the (x, r, y, open) of the left runs (a caller whose seq2 is shorter than 1 + x + r + y passes its own).
    (2, -3), extend 1: the score 2 (x + y) - (open + (r - 1)) pins the path to one gap run (2 x and 2 y > open + r, so each side pays
    for the gap; a lone match inside R cannot pay for a second gap), the walk passes through the run's cells in state E / F
    whatever their H codes say, returns to H where the gap opened and goes on diagonally to (1, 1)."""
    out = []
    rng = np.random.default_rng(18100)
    for x, r, y, go in ((300, 129, 500, 8), (300, 300, 500, 8), (1100, 1300, 700, 8)):
        a, b = _run_pair(rng, x, r, y, True)
        out.append(Hand("carried_E/r=%d" % r, a, b, K23, go, 1, 2 * (x + y) - (go + r - 1), (1 + x + r + y, 1 + x + y, 1, 1),
                        [DIAG] * y + [UP] * r + [DIAG] * x, ("carried_E_decides", "exit_top_in_E", "one_gap_run", "E_run_over_128")))
    for x, r, y, go in f_runs:
        a, b = _run_pair(rng, x, r, y, False)
        out.append(Hand("carried_F/r=%d/x=%d" % (r, x), a, b, K23, go, 1, 2 * (x + y) - (go + r - 1), (1 + x + y, 1 + x + r + y, 1, 1),
                        [DIAG] * y + [LEFT] * r + [DIAG] * x,
                        ("carried_F_decides", "exit_left_in_F", "one_gap_run", "F_extends_across_wave")))
    return out


def long_run_cases(waves=KC["kMaxWaves"]):
    """waves: the wave count whose last boundary the last case crosses (the kernel's own by default).
    seq1 = X + Y, seq2 = X + R + Y, |X| = |Y| = 900 and |R| = 300 random over four letters, (5, -4).  All 1800 bases of
    seq1 match, and seq2's 300 more cost at least one gap of 300, so for extend <= open the score is
    5 * 1800 - (open + 299 extend), first reached at (1800, 2100): (12, 1) -> 8689, (6, 6) -> 7200, (12, 0) -> 8988; the same
    with the sequences swapped (an up run of 300 rows, more than the ring's 256; end cell (2100, 1800)).  At (0, 3) one-base
    gaps are free and the same input scores 9000.  R lies in columns 901 .. 1200, across column 1024.  The last case puts the
    run across column 15360, the last wave boundary."""
    out = []
    rng = np.random.default_rng(18200)
    X, Y, R = (rng.integers(0, 4, n, dtype=np.uint8) for n in (900, 900, 300))
    a, b = np.concatenate([X, Y]), np.concatenate([X, R, Y])
    for go, ge, score in ((12, 1, 8689), (6, 6, 7200), (12, 0, 8988), (0, 3, 9000)):
        assert go < ge or score == 5 * 1800 - (go + 299 * ge)
        out.append(Hand("long_left/%d,%d" % (go, ge), a, b, K54, go, ge, score, (1800, 2100, 0, 0), None))
        out.append(Hand("long_up/%d,%d" % (go, ge), b, a, K54, go, ge, score, (2100, 1800, 0, 0), None))
    last = WAVE_COLS * (waves - 1)
    x, r, y = last - 150, 300, 450
    X, Y, R = te._lo(rng, x), te._lo(rng, y), te._hi(rng, r)
    out.append(Hand("long_left/last_wave", np.concatenate([X, Y]), np.concatenate([X, R, Y]), K23, 12, 1, 2 * (x + y) - (12 + r - 1),
                    (x + y, x + r + y, 0, 0), [DIAG] * y + [LEFT] * r + [DIAG] * x,
                    ("F_across_last_wave_of_16" if waves == KC["kMaxWaves"] else "F_extends_across_wave", "one_gap_run")))
    return out


def border_cases():
    """Walks that end on column 0 and on row 0 after more than one staging block, by a gap run that opens beside the border.
    seq1 = 3^p 2 3^r Y against seq2 = 2 Y under (10, -10), open 6, extend 0: the 2s match in column 1 (H = 10), E = 4 down
    the whole of column 1 from there, and Y (of {0, 1}) adds 10 y: the score 4 + 10 y is above Y's own 10 y.  The walk: y
    diagonals, r up moves inside E in column 1, back to H where E opened at (p + 2, 1), one diagonal to (p, 0)."""
    out = []
    rng = np.random.default_rng(18300)
    for p in (0, 7):
        for r, y, up in ((300, 200, True), (600, 200, False)):
            Y = te._lo(rng, y)
            long_ = np.concatenate([np.full(p, 3), [2], np.full(r, 3), Y]).astype(np.uint8)
            short = np.concatenate([[2], Y]).astype(np.uint8)
            codes = [DIAG] * y + [UP if up else LEFT] * r + [DIAG]
            if up:
                out.append(Hand("border/col0/p=%d" % p, long_, short, K10, 6, 0, 4 + 10 * y, (p + 1 + r + y, 1 + y, p, 0), codes))
            else:
                out.append(Hand("border/row0/p=%d" % p, short, long_, K10, 6, 0, 4 + 10 * y, (1 + y, p + 1 + r + y, 0, p), codes))
    return out


# ---- best-cell ties and padded columns ------------------------------------------------------------------------------------

def best_cell_cases(waves=KC["kMaxWaves"], handover_waves=(1,)):
    """waves: the wave count whose last wavefront holds the one valid column of the second last_column case; handover_waves:
    the wave edges 1024 w / 1024 w + 1 of the hand-over cases."""
    out = []
    L = 20
    # two blocks of 20 matches, one in wavefront 0 (bases 2) and one in wavefront 1 (bases 3), rows and columns disjoint:
    # both corners hold 20, and the one in the smaller row is first in row-major order
    for rows0, rows1 in ((70, 30), (30, 70)):
        a, b = _background(120, 1600)
        a[rows0:rows0 + L] = 2
        b[100:100 + L] = 2
        a[rows1:rows1 + L] = 3
        b[1500:1500 + L] = 3
        r, c = (rows1, 1500) if rows1 < rows0 else (rows0, 100)
        out.append(Hand("two_waves/%d,%d" % (rows0, rows1), a, b, K111, 3, 1, L, (r + L, c + L, r, c), [DIAG] * L))
        if rows1 < rows0:                               # at open 0 the first block's 100 spreads right and down, not to the left
            out.append(Hand("two_waves/open0/%d,%d" % (rows0, rows1), a, b, K54, 0, 2, 5 * L, (r + L, c + L, r, c), [DIAG] * L))
    # open 0: the block's corner at column 1024 (lane 63 of wave 0) hands its score to column 1025 (lane 0 of wave 1)
    for edge in (WAVE_COLS * w for w in handover_waves):
        a, b = _background(90, edge + 276)
        a[50:50 + L] = 2
        b[edge - L:edge] = 2
        for ge in (0, 4):
            out.append(Hand("columns_%d_%d/0,%d" % (edge, edge + 1, ge), a, b, K54, 0, ge, 5 * L, (50 + L, edge, 50, edge - L), [DIAG] * L))
    # the end cell in the last valid column; the columns right of it are padding and, at open 0, hold its score too
    for len2 in (WAVE_COLS + 1, WAVE_COLS * (waves - 1) + 1):
        a, b = _background(60, len2)
        a[30:30 + L] = 2
        b[len2 - L:] = 2
        for sm, go, ge, match in ((K111, 2, 1, 1), (K54, 0, 0, 5), (K54, 0, 3, 5)):
            out.append(Hand("last_column/%d/%d,%d" % (len2, go, ge), a, b, sm, go, ge, match * L, (30 + L, len2, 30, len2 - L), [DIAG] * L))
    return out


# ---- path ties beyond column 128 ------------------------------------------------------------------------------------------

def shifted_path_tie_cases(c0=WAVE_COLS - 64):
    """affine_edges.local_path_tie_cases (pairs of 128 x 128 over {0, 1}, selected so that every tie between two candidates
    on a cell of the path occurs) with c0 columns of bases {2, 3} in front of seq2.  Every score of a base of {0, 1} against
    one of {2, 3} is <= 0 in those matrices, so columns 1 .. c0 hold H = 0 and column c0 acts as column 0 does (F(i, c0 + 1)
    = -open): the table right of it is the small pair's, shifted by c0 -- columns 961 .. 1088, across the wave edge.
    [(affine_edges.Case with the shifted seq2, c0)]"""
    rng = np.random.default_rng(18400)
    out = []
    for case in ae.local_path_tie_cases():
        s = case.sm.reshape(4, 4)
        assert s[:2, 2:].max() <= 0
        junk = rng.integers(2, 4, (len(case.b), c0), dtype=np.uint8)
        out.append((ae.Case(case.name + "/shifted", case.a, np.concatenate([junk, case.b], axis=1), case.sm, case.gap_open,
                            case.gap_extend, dict(case.claims)), case))
    return out


def hand_groups():
    return {"floor": floor_cases, "carried": carried_cases, "long_runs": long_run_cases, "borders": border_cases,
            "best_cell": best_cell_cases}
