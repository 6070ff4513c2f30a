"""Inputs that reach the edges of the two AFFINE table aligners' mappings, the predicates that say which edge an alignment
reaches, and a whole-table numpy formulation of Gotoh's recurrences to evaluate them with.  The affine counterpart of
table_edges.py, whose helpers it reuses with the affine kernels' constants; shared by test_affine_edges_cpu.py (every claimed
edge checked through the C restatements and numpy, no device), test_affine_edges_gpu.py (every field bit-exact on the GPU)
and fuzz_parity.py.

    swmi_local_align_affine*       csrc/local_affine_kernels.hip, DESIGN.md section 14: the mapping of local_kernels.hip,
                                   F handed from lane to lane by a second row_shr:1, tie order in a 2-bit field of the key
    swmi_semiglobal_full_affine*   csrc/sgfull_affine_kernels.hip, DESIGN.md section 16: the mapping of sgfull_kernels.hip,
                                   (H, F) pairs through the LDS ring, tie order in tag bits, a walk that carries its state
                                   (H / E / F) across staging blocks of 128 rows x 512 columns

What is new against the linear aligners, and so what the predicates of this file look for: a walk that leaves a staging
block inside an E or F run (the state register is carried) or on the very move on which the gap opened (the state is H
again in the next block); an F run that extends across a wave boundary (the ring's second word) or a lane boundary (the
second DPP move); cells of the path where two candidates are equal, so that only the tag order decides the move; the pad
column with open = 0; the bounds the keys' shifts are argued from.  Every generator is deterministic."""
import functools

import numpy as np

import table_edges as te
from conftest import match_matrix
from local_support import random_matrix

SGA = te.kernel_constants("sgfull_affine_kernels.hip")
LOCA = te.kernel_constants("local_affine_kernels.hip")
WAVE = te.WAVE
COLS = SGA["kCols"]                                        # 16 columns per lane
WAVE_COLS = WAVE * COLS                                    # 1024 columns per wavefront
MAX_LEN = WAVE_COLS * SGA["kMaxWaves"]                     # 16384
STAGE_ROWS = SGA["kStageRows"]                             # 128
STAGE_LANES = SGA["kStageLanes"]                           # 32: half the linear kernel's
STAGE_COLS = STAGE_LANES * COLS                            # 512
LOC_COLS = LOCA["kCols"]                                   # 8 columns per lane
LOC_SEQ2 = LOCA["kLanes"] * LOC_COLS                       # 128
NEG = -(1 << 30)                                           # E on row 0, F on column 0


class Case:
    """One batch of one shape for one aligner and (sm, gap_open, gap_extend), and the edges its generator claims for it:
    {predicate name: the least number of its alignments that must meet it}.  linear_gap: the gap at which the LINEAR
    aligner computes the same thing (open = extend), or None."""

    def __init__(self, name, a, b, sm, gap_open, gap_extend, claims, score=None):
        self.name, self.a, self.b, self.sm = name, np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8), np.asarray(sm, np.int8)
        self.gap_open, self.gap_extend, self.claims = int(gap_open), int(gap_extend), claims
        self.score = score                                 # the score every alignment must have, worked out by hand

    @property
    def shape(self):
        return self.a.shape[1], self.b.shape[1]

    @property
    def gaps(self):
        return self.gap_open, self.gap_extend

    @property
    def linear_gap(self):
        return self.gap_open if self.gap_open == self.gap_extend else None

    def __repr__(self):
        return "%s %dx%d n=%d open=%d extend=%d sm=%s" % (self.name, self.a.shape[1], self.b.shape[1], len(self.a), self.gap_open,
                                                          self.gap_extend, self.sm.tolist())


# ---- whole tables in numpy -----------------------------------------------------------------------------------------------

def _rows(a, b, sm, go, ge, local):
    """(i, H, E, F, D) for i = 0 .. len1: int64 rows of len2 + 1 entries, D the diagonal candidate, NEG where a table has
    no value (E on row 0, F and D on column 0).  E comes straight from the row above.  F needs the row's own H:
        open >= extend: an F that opens from an H which is itself an F never beats extending that F, so
                        F(i,j) = max over k < j of P(i,k) - open - (j-1-k) extend, P = max(D, E[, 0]) and P(i,0) = H(i,0):
                        a running maximum of P(i,k) + k extend;
        open <  extend: H(i,j-1) >= F(i,j-1), so opening always wins: F(i,j) = H(i,j-1) - open and
                        H(i,j) = max over k <= j of P(i,k) - (j-k) open, a running maximum of P(i,k) + k open."""
    S = te._score_rows(a, b, sm)
    len1, len2 = S.shape
    j = np.arange(len2 + 1, dtype=np.int64)
    none = np.full(len2 + 1, NEG, np.int64)
    H = np.zeros(len2 + 1, np.int64)
    if not local:
        H[1:] = -(go + (j[1:] - 1) * ge)
    E = none
    yield 0, H, E, none, none
    for i in range(1, len1 + 1):
        En = none.copy()
        np.maximum(H[1:] - go, E[1:] - ge, out=En[1:])
        D = none.copy()
        D[1:] = H[:-1] + S[i - 1]
        P = np.maximum(D, En)
        if local:
            np.maximum(P, 0, out=P)
        P[0] = 0 if local else -(go + (i - 1) * ge)
        F = none.copy()
        if go >= ge:
            run = np.maximum.accumulate(P + j * ge)
            F[1:] = run[:-1] - go - (j[1:] - 1) * ge
            Hn = np.maximum(P, F)
        else:
            Hn = np.maximum.accumulate(P + j * go) - j * go
            F[1:] = Hn[:-1] - go
        H, E = Hn, En
        yield i, H, E, F, D


def affine_tables(a, b, sm, gap_open, gap_extend, local=False):
    """H, E, F, D of Gotoh's recurrences, each (len1 + 1) x (len2 + 1) int32 (every value lies within +-2^23; NEG = -2^30
    where a table has no value), computed a row at a time (_rows)."""
    out = [np.empty((len(a) + 1, len(b) + 1), np.int32) for _ in range(4)]
    for i, H, E, F, D in _rows(a, b, sm, int(gap_open), int(gap_extend), local):
        for t, row in zip(out, (H, E, F, D)):
            t[i] = np.maximum(row, NEG)
    return tuple(out)


# what a cell's candidates are equal to: one byte per cell is all the walk and every path predicate need
DIAG, H_IS_E, H_IS_F, E_OPEN, E_EXT, F_OPEN, F_EXT, FLOOR = (1 << k for k in range(8))


def affine_flags(a, b, sm, gap_open, gap_extend, local=False, keep_h=False):
    """(flags[(len1 + 1) x (len2 + 1)] uint8, (score, i, j) of the best cell): which candidates each cell's H, E and F
    equal -- H's diagonal term, E and F (and 0, local); E's and F's open and extend terms -- and the first cell in row-major
    order strictly above every earlier one, from 0 at (0, 0).  A quarter of the memory of one table.  keep_h: the H table
    (int32) as a third result."""
    go, ge = int(gap_open), int(gap_extend)
    flags = np.zeros((len(a) + 1, len(b) + 1), np.uint8)
    table = np.empty(flags.shape, np.int32) if keep_h else None
    best = (0, 0, 0)
    Hp = Ep = None
    for i, H, E, F, D in _rows(a, b, sm, go, ge, local):
        if keep_h:
            table[i] = H
        if i:
            conds = [H[1:] == D[1:], H[1:] == E[1:], H[1:] == F[1:], E[1:] == Hp[1:] - go, (E[1:] == Ep[1:] - ge) & (Ep[1:] > NEG),
                     F[1:] == H[:-1] - go, (F[1:] == F[:-1] - ge) & (F[:-1] > NEG)] + ([H[1:] == 0] if local else [])
            f = flags[i, 1:]
            for bit, cond in enumerate(conds):             # DIAG, H_IS_E, ... in the order of their bits
                f |= cond.view(np.uint8) << bit
            m = int(H[1:].max())
            if m > best[0]:
                best = (m, i, 1 + int(np.argmax(H[1:])))
        Hp, Ep = H, E
    return (flags, best, table) if keep_h else (flags, best)


class Walk:
    """The walk back from the best cell over affine_flags: codes[t] the move taken at step t (3 / 2 / 1 = diagonal / up /
    left), (i[t], j[t]) the cell it was taken from, arrived[t] the state the walk reached that cell in (0 / 1 / 2 = H / E /
    F), state[t] the state the move was made in and after[t] the state after it (0 where the gap opened on this move);
    (i[-1], j[-1]) the cell the walk ends on and arrived[-1] the state it reached it in.  The semi-global walk is forced
    along row 0 and column 0 (state H); the local one stops at H = 0 reached in state H."""

    def __init__(self, end_i, end_j, steps):
        """steps: [(state the move is made in, state after it)]"""
        made = np.array([s for s, _ in steps], np.int64)
        self.state, self.after = made, np.array([x for _, x in steps], np.int64)
        self.codes = 3 - made                               # H: diagonal (3), E: up (2), F: left (1)
        self.i = end_i - np.concatenate([[0], np.cumsum(made != 2)])
        self.j = end_j - np.concatenate([[0], np.cumsum(made != 1)])
        self.arrived = np.concatenate([[0], self.after])

    @classmethod
    def from_flags(cls, flags, end_i, end_j, local):
        i, j, state = int(end_i), int(end_j), 0
        steps = []
        while i > 0 and j > 0:
            f = int(flags[i, j])
            if state == 0:
                if local and f & FLOOR:
                    break
                state = 0 if f & DIAG else 1 if f & H_IS_E else 2
            made = state
            if state == 0:
                i, j = i - 1, j - 1
            elif state == 1:
                state = 0 if f & E_OPEN else 1
                i -= 1
            else:
                state = 0 if f & F_OPEN else 2
                j -= 1
            steps.append((made, state))
        walk = cls(end_i, end_j, steps)
        if not local:                                       # forced: up along column 0, left along row 0, no state
            n = len(walk.codes)
            walk.codes = np.concatenate([walk.codes, np.full(i, 2), np.full(j, 1)]).astype(np.int64)
            walk.i = np.concatenate([walk.i, np.arange(i - 1, -1, -1), np.zeros(j, np.int64)]).astype(np.int64)
            walk.j = np.concatenate([walk.j, np.full(i, j), np.arange(j - 1, -1, -1)]).astype(np.int64)
            zeros = np.zeros(len(walk.codes) - n, np.int64)
            walk.state, walk.after, walk.arrived = (np.concatenate([x, zeros]) for x in (walk.state, walk.after, walk.arrived))
        return walk

    def words(self, n_words):
        """the moves packed as the aligners return them: 2 bits per move, 32 per uint64 word, walking order"""
        out = np.zeros(n_words, np.uint64)
        for t0 in range(0, len(self.codes), 32):
            c = self.codes[t0:t0 + 32].astype(np.uint64)
            out[t0 // 32] = np.bitwise_or.reduce(c << (2 * np.arange(len(c), dtype=np.uint64)))
        return out


def numpy_affine(a, b, sm, gap_open, gap_extend, local=False, keep_h=False):
    """(score, (end_i, end_j), Walk, flags[, H]) of one alignment from the numpy tables"""
    flags, (score, bi, bj), *table = affine_flags(a, b, sm, gap_open, gap_extend, local, keep_h)
    return (score, (bi, bj), Walk.from_flags(flags, bi, bj, local), flags) + tuple(table)


# ---- predicates ----------------------------------------------------------------------------------------------------------

SG_TIE_CLAIMS = ("tie_two_waves", "first_in_later_wave", "tie_two_lanes_one_wave", "first_in_later_lane", "same_lane_later_row")
LOCAL_TIE_CLAIMS = ("tie_two_lanes", "first_in_later_lane", "same_lane_earlier_col_later_row", "same_column_later_row")
PATH_TIES = ("tie_diag_E", "tie_diag_F", "tie_E_F_above_diag", "tie_E_open_extend", "tie_F_open_extend")
FLOOR_TIES = ("tie_floor_diag", "tie_floor_gap")


def _longest(mask):
    """the longest run of True"""
    if not mask.any():
        return 0
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max())


def path_tie_facts(walk, flags, local=False):
    """Ties between candidates on cells of the path, each in the state the walk is in there, so that the tag order alone
    decides the move: the diagonal equal to E or to F where the walk arrives in state H (the diagonal wins), E equal to F
    above the diagonal (E wins), E's or F's open candidate equal to its extend candidate where the walk is inside that gap
    (opening wins) -- counted only where the cell the gap opened from does not itself continue the same gap, so that the
    other order would give other moves; local: H = 0 reached in state H with a candidate at 0 as well (the floor wins)."""
    out = dict.fromkeys(PATH_TIES + (FLOOR_TIES if local else ()), False)
    i, j = walk.i, walk.j
    n = len(walk.codes)
    f = flags[i[:n], j[:n]].astype(np.int64)
    in_h = walk.arrived[:n] == 0
    out["tie_diag_E"] = bool(np.any(in_h & (f & DIAG > 0) & (f & H_IS_E > 0)))
    out["tie_diag_F"] = bool(np.any(in_h & (f & DIAG > 0) & (f & H_IS_F > 0)))
    out["tie_E_F_above_diag"] = bool(np.any(in_h & (f & DIAG == 0) & (f & H_IS_E > 0) & (f & H_IS_F > 0)))
    # the cell the gap opens from, (i - 1, j) or (i, j - 1), reached in state H: what it does next
    nxt = flags[i[1:n + 1], j[1:n + 1]].astype(np.int64)
    inside = (i[1:n + 1] > 0) & (j[1:n + 1] > 0)
    stops = (nxt & FLOOR > 0) if local else np.zeros(n, bool)
    goes_up = ~stops & (nxt & DIAG == 0) & (nxt & H_IS_E > 0)
    goes_left = ~stops & (nxt & DIAG == 0) & (nxt & H_IS_E == 0) & (nxt & H_IS_F > 0)
    out["tie_E_open_extend"] = bool(np.any((walk.state == 1) & (f & E_OPEN > 0) & (f & E_EXT > 0) & inside & ~goes_up))
    out["tie_F_open_extend"] = bool(np.any((walk.state == 2) & (f & F_OPEN > 0) & (f & F_EXT > 0) & inside & ~goes_left))
    if local and i[-1] > 0 and j[-1] > 0 and walk.arrived[-1] == 0:
        last = int(flags[i[-1], j[-1]])
        if last & FLOOR:
            out["tie_floor_diag"] = bool(last & DIAG)
            out["tie_floor_gap"] = bool(last & (H_IS_E | H_IS_F))
    return out


def sg_walk_facts(case, score, walk, flags=None):
    """The walk-shape predicates of one affine semi-global alignment: those of table_edges.py for the affine staging block,
    and the ones that need the walk's state.  carried_E_decides / carried_F_decides (they need the flags): the walk enters
    a block inside E or F on a cell whose H would go another way (the diagonal ties with the gap there, and wins), so that
    a walk which forgot its state at the block's edge would turn off the run."""
    c, i, j = walk.codes, walk.i, walk.j
    out = te.sg_walk_facts(score, c, i, j, STAGE_ROWS, STAGE_LANES)
    exits = te.staging_exits(i, j, STAGE_ROWS, STAGE_LANES, steps=True)
    left_moves = walk.state == 2

    def other_way(t, gap_bit):           # H's own choice on cell t (diagonal, E, F in that order) is not this gap
        f = int(flags[i[t], j[t]]) if flags is not None and i[t] > 0 and j[t] > 0 else gap_bit
        return bool(f & DIAG) or (gap_bit == H_IS_F and bool(f & H_IS_E)) or not f & gap_bit
    out.update({
        "exit_top_in_E": any(kind == "top" and walk.after[t - 1] == 1 for kind, _, t in exits),
        "exit_left_in_F": any(kind == "left" and walk.after[t - 1] == 2 for kind, _, t in exits),
        "exit_top_on_open": any(kind == "top" and walk.state[t - 1] == 1 and walk.after[t - 1] == 0 for kind, _, t in exits),
        "exit_left_on_open": any(kind == "left" and walk.state[t - 1] == 2 and walk.after[t - 1] == 0 for kind, _, t in exits),
        "exit_corner": any(kind == "corner" for kind, _, _ in exits),
        "carried_E_decides": any(kind == "top" and walk.after[t - 1] == 1 and other_way(t, H_IS_E) for kind, _, t in exits),
        "carried_F_decides": any(kind == "left" and walk.after[t - 1] == 2 and other_way(t, H_IS_F) for kind, _, t in exits),
        # the move from column 1024 k + 1 to 1024 k inside F: F(i, 1024 k + 1) is F(i, 1024 k) - extend, the ring's second word
        "F_extends_across_wave": case.gap_extend < case.gap_open and bool(np.any(
            left_moves & (walk.after == 2) & (j[:-1] % WAVE_COLS == 1) & (j[:-1] > 1))),
        "F_across_last_wave_of_16": case.gap_extend < case.gap_open and bool(np.any(
            left_moves & (walk.after == 2) & (j[:-1] == WAVE_COLS * (SGA["kMaxWaves"] - 1) + 1))),
        "E_run_over_128": _longest(walk.after == 1) >= STAGE_ROWS,
        "one_gap_run": len(te.gap_runs(c, i, j)) == 1,
        "end_at_len2_open0": case.gap_open == 0 and score > 0 and int(j[0]) == case.shape[1] and case.shape[1] % COLS != 0,
    })
    return out


def local_walk_facts(case, score, walk):
    c, i, j = walk.codes, walk.i, walk.j
    return {
        "up_run_over_128": any(code == 2 and L > 128 for code, L, _, _ in te.gap_runs(c, i, j)),
        "E_run_over_128": _longest(walk.after == 1) >= 128,
        # the move from column 8 l + 1 to 8 l inside F: lane l's F(i, 8 l + 1) extends lane l - 1's F(i, 8 l)
        "F_extends_across_lane": case.gap_extend < case.gap_open and bool(np.any(
            (walk.state == 2) & (walk.after == 2) & (j[:len(c)] % LOC_COLS == 1) & (j[:len(c)] > 1))),
        "one_left_run_over_8": [code == 1 and L > LOC_COLS for code, L, _, _ in te.gap_runs(c, i, j)] == [True],
    }


def facts_of(case, k, local):
    """(facts, score, (end_i, end_j), Walk) of alignment k of a case, every predicate the case claims evaluated on the
    numpy tables"""
    best_ties = any(c in (LOCAL_TIE_CLAIMS if local else SG_TIE_CLAIMS) for c in case.claims)
    score, end, walk, flags, *table = numpy_affine(case.a[k], case.b[k], case.sm, case.gap_open, case.gap_extend, local, keep_h=best_ties)
    facts = local_walk_facts(case, score, walk) if local else sg_walk_facts(case, score, walk, flags)
    if any(c in PATH_TIES + FLOOR_TIES for c in case.claims):
        facts.update(path_tie_facts(walk, flags, local))
    if best_ties:
        facts.update(te.local_tie_facts(table[0]) if local else te.sg_tie_facts(table[0]))
    return facts, score, end, walk


def claim_counts(case, local):
    """({claim: number of alignments of the case that meet it}, [(score, end, Walk)] per alignment)"""
    counts = dict.fromkeys(case.claims, 0)
    results = []
    for k in range(len(case.a)):
        facts, score, end, walk = facts_of(case, k, local)
        for c in counts:
            counts[c] += bool(facts[c])
        results.append((score, end, walk))
    return counts, results


# ---- shape grids ---------------------------------------------------------------------------------------------------------

SGA_LEN1 = te.sg_len1_grid(SGA)
SGA_LEN2 = te.sg_len2_grid(SGA)
LOCA_LEN1 = te.local_len1_grid(LOCA)
LOCA_N = te.local_n_grid(LOCA)
ZERO_GAPS = [(0, 0), (5, 0), (0, 5)]


def sg_shape_grid():
    """the grid of table_edges.sg_shape_grid derived from the affine kernel's constants"""
    return te.sg_shape_grid(SGA_LEN1, SGA_LEN2)


def local_shape_grid():
    return te.local_shape_grid(LOCA_LEN1, LOCA_N)


def grid_params(index):
    """The three parameter sets of grid shape number `index`: extend < open, open < extend with a random matrix, and one of
    (0, 0), (5, 0), (0, 5) in turn."""
    go, ge = ZERO_GAPS[index % 3]
    return [("(2,-3,11,1)", match_matrix(2, -3), 11, 1), ("random,3,7", random_matrix(3), 3, 7),
            ("(5,-4,%d,%d)" % (go, ge), match_matrix(5, -4), go, ge)]


# ---- generators: semi-global ---------------------------------------------------------------------------------------------

RUN_SM = match_matrix(2, -3)


def sg_run_cases():
    """One interior gap run of exactly |R|: seq2 = X + R + Y against seq1 = X + Y (a left run, inside F) and the other way
    round (an up run, inside E); X and Y of {0, 1}, copied exactly, R of {2, 3}, (2, -3), extend 1.  |Y| >= |R| / 2 + 300
    makes the detour pay, so the score is 2 (|X| + |Y|) - (open + (|R| - 1) extend), which pins the run to a single gap.
    |X| places the left runs (columns |X| + 1 .. |X| + |R|) across j = 1024 k for several k; every run is longer than a
    staging block is wide (512) or high (128), so the walk leaves a block inside it.  The walk enters the next block at a
    column 16 g (left runs) or a row len1 - 128 m (up runs: every block before was left through the top); R holds X's last
    base at every such column (row), where the diagonal then equals F (E): H of the cell the walk enters on would take
    the diagonal, and only the carried state keeps the walk in the run.  A lone match cannot pay for a second gap, so the
    score identity stands."""
    cases = []
    rng = np.random.default_rng(11100)
    last = WAVE_COLS * (SGA["kMaxWaves"] - 1)
    #   |R|   len1   the |X| of each alignment (the first: 700, with the shortest |Y| the score identity allows at len1)
    for r, len1, xs in ((520, 700 + 560, (700,)), (520, 3460, (700, 1800, 2900)), (600, 2100, (700, 1500)),
                        (1100, 1850, (700, 1000)), (2100, 2350, (700, 1000)), (520, last - 300 + 560, (last - 300,))):
        rows1, rows2 = [], []
        for x in xs:
            assert len1 - x >= r // 2 + 300 and (x + r) // WAVE_COLS > x // WAVE_COLS
            X, Y = te._lo(rng, x), te._lo(rng, len1 - x)
            R = te._hi(rng, r)
            R[:-1][(x + 1 + np.arange(r - 1)) % COLS == 0] = X[-1]          # not R's last base: the gap could then end a base earlier
            rows1.append(np.concatenate([X, Y]))
            rows2.append(np.concatenate([X, R, Y]))
        claims = {"one_gap_run": len(xs), "F_extends_across_wave": len(xs), "exit_left_in_F": len(xs), "carried_F_decides": len(xs)}
        if xs[0] == last - 300:
            claims["F_across_last_wave_of_16"] = 1
        cases.append(Case("insertion%d/len1=%d" % (r, len1), np.stack(rows1), np.stack(rows2), RUN_SM, 10, 1, claims,
                          score=2 * len1 - (10 + (r - 1))))
    for r, len2, xs in ((129, 1500, (300, 1100)), (300, 1600, (300, 1100)), (1300, 2100, (300, 1100))):
        rows1, rows2 = [], []
        for x in xs:
            assert len2 - x >= r // 2 + 300
            X, Y = te._lo(rng, x), te._lo(rng, len2 - x)
            R = te._hi(rng, r)
            R[:-1][(x + 1 + np.arange(r - 1) - (len2 + r)) % COLS == 0] = X[-1]
            rows1.append(np.concatenate([X, R, Y]))
            rows2.append(np.concatenate([X, Y]))
        cases.append(Case("deletion%d/len2=%d" % (r, len2), np.stack(rows1), np.stack(rows2), RUN_SM, 8, 1,
                          {"one_gap_run": len(xs), "E_run_over_128": len(xs), "exit_top_in_E": len(xs), "carried_E_decides": len(xs)},
                          score=2 * len2 - (8 + (r - 1))))
    return cases


def sg_extend0_cases():
    """extend = 0: F never decays, so one value travels along a row across every wave boundary of a 16-wave alignment.
    seq2 = junk + X + R + Y against seq1 = X + Y: the border costs `open` whatever its length, the left run of |R| crosses
    the last wave boundary, and the walk then runs along row 0 to column 0."""
    rng = np.random.default_rng(11200)
    last = WAVE_COLS * (SGA["kMaxWaves"] - 1)
    x, r, y = 200, 520, 400
    X, Y = te._lo(rng, x), te._lo(rng, y)
    a = np.concatenate([X, Y])[None]
    b = np.concatenate([te._hi(rng, last - 300 - x), X, te._hi(rng, r), Y])[None]
    return [Case("extend0/16waves", a, b, RUN_SM, 9, 0, {"F_extends_across_wave": 1, "F_across_last_wave_of_16": 1, "exit_left_in_F": 1})]


def sg_staircase_cases():
    """the staircases of table_edges.py (several gaps of 100..200 both ways) with affine parameters: the walk turns corners
    between E, F and H and leaves blocks through the top, inside an up gap where extending is cheaper than opening and on
    an opening move where it is not (open = extend: opening wins every tie)"""
    out = []
    for case, (go, ge) in zip(te.sg_staircase_cases(), ((6, 1), (12, 0), (2, 2))):
        n = len(case.a) // 2                                # half of them: the numpy tables of 7000 x 7000 take seconds each
        claims = {"staircase": n, "block_exit_top": n, "block_across_waves": n}
        claims.update({"exit_top_in_E": n} if ge < go else {"exit_top_on_open": n})
        out.append(Case(case.name, case.a[:n], case.b[:n], RUN_SM, go, ge, claims))
    return out


CORNER_GAPS = [(1, 1), (6, 1), (0, 3)]


def sg_corner_cases():
    """A walk that leaves a staging block through its corner: the best cell (x + 127, x + L + 127), 127 diagonal moves back
    to row x, the block's top row, a left run of L to column x + 1 = 16 g_lo + 1, the block's first (x = 1 mod 16,
    L in 16 (kStageLanes - 1) - (kStageRows - 1) .. + 15 = 369 .. 384), then a diagonal move out of both edges at once, in
    state H again since the run's last move opened the gap."""
    lo = COLS * (STAGE_LANES - 1) - (STAGE_ROWS - 1)
    cases = []
    rng = np.random.default_rng(12300)
    for x, L in ((17, lo + 15), (33, lo), (1025, lo + 8), (2049, lo + 11)):
        X, Y = te._lo(rng, x), te._lo(rng, STAGE_ROWS - 1)
        a = np.concatenate([X, Y])[None]
        b = np.concatenate([X, te._hi(rng, L), Y])[None]
        for go, ge in CORNER_GAPS:
            cases.append(Case("corner/x=%d/L=%d" % (x, L), a, b, match_matrix(10, -10), go, ge, {"exit_corner": 1}))
    return cases


def sg_open_exit_cases():
    """The move that leaves a staging block is the one on which the gap opened, so the next block starts in state H.
    Left: x = 16 g, d = 50 diagonal moves from the best cell (x + d, x + L + d), then a left run of L = 450
    (d - 1 + L in 496 .. 511) whose last move goes from column 16 g + 1, the block's first, to 16 g.  Up: d diagonal moves,
    then an up run of L = 128 - d or 256 - d rows whose last move leaves through the block's top row."""
    cases = []
    rng = np.random.default_rng(12400)
    d = 50
    L = COLS * (STAGE_LANES - 1) + 4 - d
    assert COLS * (STAGE_LANES - 1) <= d - 1 + L < COLS * STAGE_LANES
    for x in (160, 1040):
        X, Y = te._lo(rng, x), te._lo(rng, d)
        cases.append(Case("open_exit/left/x=%d" % x, np.concatenate([X, Y])[None], np.concatenate([X, te._hi(rng, L), Y])[None],
                          match_matrix(10, -10), 6, 1, {"exit_left_on_open": 1, "one_gap_run": 1}))
    for x, L in ((160, STAGE_ROWS - d), (1040, 2 * STAGE_ROWS - d)):
        X, Y = te._lo(rng, x), te._lo(rng, d)
        cases.append(Case("open_exit/up/x=%d/L=%d" % (x, L), np.concatenate([X, te._hi(rng, L), Y])[None], np.concatenate([X, Y])[None],
                          match_matrix(10, -10), 6, 1, {"exit_top_on_open": 1, "one_gap_run": 1}))
    return cases


def sg_wave_edge_end_cases():
    """the best cell at j = 1024 k and 1024 k + 1 (table_edges.py), with affine parameters"""
    return [Case(c.name, c.a, c.b, c.sm, 7, 2, {"end_at_wave_edge": 2}) for c in te.sg_wave_edge_end_cases()]


@functools.lru_cache(maxsize=None)          # selected by whole tables: seconds, and nobody changes a case
def sg_best_tie_cases():
    """Ties of the maximum H that only the reduction order decides: the cases of table_edges.sg_tie_cases at open = extend
    = their gap (0 for the constructed ones), where the affine aligner is the linear one."""
    return [Case(c.name, c.a, c.b, c.sm, c.gap, c.gap, dict(c.claims)) for c in te.sg_tie_cases()]


PATH_TIE_GAPS = [(1, 0), (1, 1), (2, 1), (0, 1)]


def _select(rng, make, facts_of_pair, want, per_claim, batch):
    """pairs drawn by make(rng) and kept where they add to a claim of `want` that is still short; at most 40 rounds"""
    chosen, got = [], dict.fromkeys(want, 0)
    for _ in range(40):
        for _ in range(batch):
            a, b = make(rng)
            facts = facts_of_pair(a, b)
            if any(facts[c] and got[c] < per_claim for c in want):
                chosen.append((a, b))
                for c in want:
                    got[c] += bool(facts[c])
        if all(v >= per_claim for v in got.values()):
            break
    return chosen


def _path_tie_cases(local, seed, len1, len2, per_claim):
    cases = []
    rng = np.random.default_rng(seed)
    for t, (go, ge) in enumerate(PATH_TIE_GAPS):
        name, sm = te.TIE_MATRICES[t % len(te.TIE_MATRICES)]
        # with open < extend opening wins strictly: E's and F's two candidates are never equal
        want = tuple(c for c in PATH_TIES + (FLOOR_TIES if local else ()) if go >= ge or not c.endswith("open_extend"))

        def facts(a, b):
            _, _, walk, flags = numpy_affine(a, b, sm, go, ge, local)
            return path_tie_facts(walk, flags, local)
        chosen = _select(rng, lambda r: (r.integers(0, 2, len1, dtype=np.uint8), r.integers(0, 2, len2, dtype=np.uint8)), facts, want,
                         per_claim, 16)
        cases.append(Case("%spath_ties/%s/%d,%d" % ("local_" if local else "", name, go, ge), np.stack([c[0] for c in chosen]),
                          np.stack([c[1] for c in chosen]), sm, go, ge, {c: per_claim for c in want}))
    return cases


@functools.lru_cache(maxsize=None)          # selected by whole tables: seconds, and nobody changes a case
def sg_path_tie_cases(per_claim=4):
    """Random pairs over {0, 1}, 60 x 80, matrices in {-1, 0, 1}, selected by the numpy predicates until every path tie is
    met by per_claim alignments."""
    return _path_tie_cases(False, 14400, 60, 80, per_claim)


def sg_pad_cases():
    """open = 0, len2 % 16 != 0 and the best cell in column len2: the pad column beside it holds exactly the best value
    (F opens from it at no cost).  The inputs of table_edges.sg_pad_cases at extend 0 and 3, and len2 = 1024 (W - 1) + 1
    (one valid column in the last wave, 63 whole lanes of padding) at (0, 0)."""
    cases = []
    keep = [0, 2, 4, 1]                                     # the three exact copies of each case and one noisy one
    for c in te.sg_pad_cases():
        for ge in (0, 3):
            cases.append(Case(c.name, c.a[keep], c.b[keep], c.sm, 0, ge, {"end_at_len2_open0": 3}))
    rng = np.random.default_rng(15500)
    len2 = WAVE_COLS * 2 + 1
    B = rng.integers(0, 4, (4, len2), dtype=np.uint8)
    a = np.concatenate([B, rng.integers(0, 4, (4, 40), dtype=np.uint8)], axis=1)
    cases.append(Case("pad/one_column_in_last_wave/len2=%d" % len2, a, B, match_matrix(1, -1), 0, 0, {"end_at_len2_open0": 4}))
    return cases


_PLUS = np.full(16, 127, np.int8)
_MINUS = np.full(16, -128, np.int8)
_BOTH = np.where(np.eye(4, dtype=bool), 127, -128).astype(np.int8).reshape(16)
EXTREME_PARAMS = [("all+127/0,0", _PLUS, 0, 0), ("all-128/127,127", _MINUS, 127, 127), ("all-128/127,0", _MINUS, 127, 0),
                  ("all-128/0,127", _MINUS, 0, 127), ("diag+127,off-128/127,0", _BOTH, 127, 0), ("diag+127,off-128/0,127", _BOTH, 0, 127)]


def sg_extreme_cases():
    """16384 x 16384 at the bounds the keys' shifts are argued from, on an identical, a shifted and a random pair"""
    a, b = te._pair_kinds(3, MAX_LEN, MAX_LEN, 18800)
    return [Case("extreme/" + name, a, b, sm, go, ge, {}) for name, sm, go, ge in EXTREME_PARAMS]


# ---- generators: local ---------------------------------------------------------------------------------------------------

def local_run_cases():
    """seq1 lacks r bases of the 128-mer (one left run of r, inside F, across r / 8 lane boundaries), or carries the 128-mer
    with more than 128 bases of {2, 3} inserted (an up run inside E, the inputs of table_edges.local_insertion_cases).
    The 128-mer's r bases are all 2 and seq1 is 3 around its two flanks of {0, 1}, so nothing but flank on flank matches:
    the score is 20 (128 - r) - (open + (r - 1) extend)."""
    cases = []
    rng = np.random.default_rng(16600)
    for r, (go, ge) in ((9, (10, 1)), (17, (10, 1)), (60, (10, 1)), (100, (10, 1)), (100, (3, 0))):
        b = rng.integers(0, 2, (6, LOC_SEQ2), dtype=np.uint8)
        a = np.full((6, 300), 3, np.uint8)
        for k in range(6):
            cut = int(rng.integers(10, LOC_SEQ2 - r - 10 + 1))
            b[k, cut:cut + r] = 2
            src = np.concatenate([b[k, :cut], b[k, cut + r:]])
            at = int(rng.integers(0, 300 - len(src) + 1))
            a[k, at:at + len(src)] = src
        cases.append(Case("local_deletion%d" % r, a, b, match_matrix(20, -20), go, ge, {"one_left_run_over_8": 6, "F_extends_across_lane": 6},
                          score=20 * (LOC_SEQ2 - r) - (go + (r - 1) * ge)))
    for c in te.local_insertion_cases():
        cases.append(Case(c.name, c.a, c.b, c.sm, 10, 1, {"up_run_over_128": 6, "E_run_over_128": 6}))
    return cases


@functools.lru_cache(maxsize=None)          # selected by whole tables: seconds, and nobody changes a case
def local_best_tie_cases():
    return [Case(c.name, c.a, c.b, c.sm, c.gap, c.gap, dict(c.claims)) for c in te.local_tie_cases()]


@functools.lru_cache(maxsize=None)          # selected by whole tables: seconds, and nobody changes a case
def local_path_tie_cases(per_claim=4):
    """the same for the local aligner, 128 x 128 (gaps both ways), with the two ties of the zero floor"""
    return _path_tie_cases(True, 17700, LOC_SEQ2, LOC_SEQ2, per_claim)


def local_extreme_cases():
    """len1 = 16384 with the extreme parameter sets"""
    a, b = te._pair_kinds(6, te.LOC_MAX_LEN, LOC_SEQ2, 19900)
    return [Case("local_extreme/" + name, a, b, sm, go, ge, {}) for name, sm, go, ge in EXTREME_PARAMS]


SG_GROUPS = {"runs": sg_run_cases, "extend0": sg_extend0_cases, "staircases": sg_staircase_cases, "corners": sg_corner_cases,
             "open_exits": sg_open_exit_cases, "wave_edge_ends": sg_wave_edge_end_cases, "best_ties": sg_best_tie_cases,
             "path_ties": sg_path_tie_cases, "pad": sg_pad_cases}
LOCAL_GROUPS = {"runs": local_run_cases, "best_ties": local_best_tie_cases, "path_ties": local_path_tie_cases}


# ---- comparisons ---------------------------------------------------------------------------------------------------------

def sg_result_of(results, move_words):
    """[(score, end, Walk)] as the (scores, ends, moves, lengths) an aligner returns"""
    n = len(results)
    sc = np.array([r[0] for r in results], np.int32)
    ends = np.array([r[1] for r in results], np.int32).reshape(n, 2)
    moves = np.stack([r[2].words(move_words) for r in results])
    return sc, ends, moves, np.array([len(r[2].codes) + 1 for r in results], np.uint32)


def local_result_of(results, move_words):
    n = len(results)
    sc = np.array([r[0] for r in results], np.int32)
    ends = np.array([r[1] + (int(r[2].i[-1]), int(r[2].j[-1])) for r in results], np.int32).reshape(n, 4)
    moves = np.stack([r[2].words(move_words) for r in results])
    return sc, ends, moves, np.array([len(r[2].codes) for r in results], np.uint32)
