"""Hand-built inputs for the wide-alphabet aligners (libswmi_wide.so, libswmi_wide_long.so, libswmi_wide_profile.so; DESIGN.md
sections 29, 30 and 32), deterministic and without a device.  Shared by test_wide_edges_cpu.py (the inputs mean what they claim,
on the C restatements alone) and test_wide_edges_gpu.py (every field bit-exact on the GPU).

The wide kernels are the 4-letter affine sweep with one thing changed: where a cell's score comes from.  So this file has two
halves.

    relabelling   a 4-letter hand case (local_full_affine_edges.py, global_full_affine_edges.py, the shifted path ties) becomes a
                  32-letter one: seq1's bases go through an injective map rows: 4 -> 32, seq2's through a different one, cols;
                  sm32[rows[x] * 32 + cols[y]] = sm4[x * 4 + y]; every other entry is a FILLER that a correct kernel never reads;
                  random bits 5 - 7 on every byte.  The table of substitution scores is the 4-letter one cell for cell, so the
                  score, the ends and every move are the 4-letter case's.  With rows != cols a transposed lookup lands on the
                  filler, with letters >= 16 a dropped bit 4 does, and a filler of +127 is a trap that the local kind's zero floor
                  cannot hide.
    census        alignments with closed-form results in which ONE profile byte decides the score and the end cell: every letter
                  row at every column position of lanes 0, 31 and 63 of each of the four waves, every (seq1 letter, seq2 letter)
                  pair, the values >= 64, 127 and -128 (the sign extension of the cell's v_bfe_i32)."""
import functools

import numpy as np

import global_full_affine_edges as gfe
import local_full_affine_edges as lfe
import table_edges as te
from wide_support import BEGIN2, END2, GLOBAL, LOCAL, move_offsets, moves_of

WK = te.kernel_constants("wide_long_internal.h")          # includes wide_internal.h
MAX_WAVES = WK["kWideMaxWaves"]                            # 4
MAX_LEN1, MAX_LEN2 = WK["kWideMaxLen1"], WK["kWideMaxLen2"]    # 16384, 4096
LONG_MAX_LEN = WK["kWideLongMaxLen"]                       # 65536
COLS, WAVE_COLS = lfe.COLS, lfe.WAVE_COLS                  # 16, 1024: the sweep is the 4-letter kernels'
LETTERS = 32
DIAG, UP, LEFT = 3, 2, 1

# (rows, cols, filler)
RELABELLINGS = (((0, 1, 2, 3), (0, 1, 2, 3), 127),
                ((31, 0, 16, 15), (7, 24, 8, 23), 127),
                ((28, 29, 30, 31), (3, 2, 1, 0), -128))


class WCase:
    """n alignments over FOUR letters under one kind, mask, 4 x 4 matrix and gap pair, before relabelling.  a, b: lists of 1-D
    uint8 arrays; pinned: per alignment (score, ends, walking-order move codes or None), or None where only the 4-letter
    restatement says what the result is (the selected path-tie pairs)."""

    def __init__(self, name, kind, mask, a, b, sm4, gap_open, gap_extend, pinned=None, claims=()):
        self.name, self.kind, self.mask = name, kind, int(mask)
        self.a, self.b = [np.ascontiguousarray(x, np.uint8) for x in a], [np.ascontiguousarray(x, np.uint8) for x in b]
        self.sm4, self.gap_open, self.gap_extend = np.asarray(sm4, np.int8).reshape(16), int(gap_open), int(gap_extend)
        self.pinned, self.claims = pinned, tuple(claims)
        assert max(len(x) for x in self.a) <= LONG_MAX_LEN and max(len(x) for x in self.b) <= LONG_MAX_LEN

    @property
    def key(self):
        """what one call shares"""
        return self.kind, self.mask, self.sm4.tobytes(), self.gap_open, self.gap_extend

    @property
    def fits_wide(self):
        return max(len(x) for x in self.a) <= MAX_LEN1 and max(len(x) for x in self.b) <= MAX_LEN2

    def __repr__(self):
        return "%s kind=%d mask=%d n=%d %dx%d open=%d extend=%d" % (self.name, self.kind, self.mask, len(self.a), len(self.a[0]), len(self.b[0]),
                                                                    self.gap_open, self.gap_extend)


def _of_hand(h):
    return WCase(h.name, LOCAL, 0, [h.a[0]], [h.b[0]], h.sm, h.gap_open, h.gap_extend, [(h.score, h.ends, h.codes)], h.claims)


def _of_global_hand(h):
    return WCase(h.name, GLOBAL, h.mask, [h.a[0]], [h.b[0]], h.sm, h.gap_open, h.gap_extend, [(h.score, h.ends, h.codes)])


def _of_tie_case(case):
    return WCase(case.name, LOCAL, 0, list(case.a), list(case.b), case.sm, case.gap_open, case.gap_extend, None, tuple(case.claims))


# ---- a. relabelling ---------------------------------------------------------------------------------------------------------

def relabel_matrix(sm4, rows, cols, filler):
    sm32 = np.full((LETTERS, LETTERS), filler, np.int8)
    sm32[np.ix_(np.asarray(rows), np.asarray(cols))] = np.asarray(sm4, np.int8).reshape(4, 4)
    return sm32.reshape(-1)


def relabel(case, rows, cols, filler, junk_seed):
    """(a32, b32, sm32) of a WCase: lists of uint8 arrays over 32 letters with random bits 5 - 7, and the flat 32 x 32 matrix."""
    assert len(set(rows)) == 4 and len(set(cols)) == 4
    rng = np.random.default_rng(junk_seed)
    rmap, cmap = np.asarray(rows, np.uint8), np.asarray(cols, np.uint8)

    def through(seqs, letter):
        return [(letter[x & 3] | (rng.integers(0, 8, len(x), dtype=np.uint8) << 5)).astype(np.uint8) for x in seqs]
    return through(case.a, rmap), through(case.b, cmap), relabel_matrix(case.sm4, rows, cols, filler)


# ---- b. the local kind's hand families --------------------------------------------------------------------------------------
# local_full_affine_edges.py's groups.  Three of its generators build cases from the 4-letter kernel's 16 wavefronts, which do not
# fit 4096 columns; they take the wide wave count instead (and the one left run of 2100 a shorter one across column 2048).

WIDE_CARRIED_F_RUNS = lfe.CARRIED_F_RUNS[:2] + ((1300, 1400, 1350, 10),)
TIE_C0 = WAVE_COLS - 64


@functools.lru_cache(maxsize=None)
def local_families():
    """{family: [WCase]}, every case inside the wide domain (len1 <= 16384, len2 <= 4096)."""
    edges = tuple(range(1, MAX_WAVES))                      # the hand-over at 1024 / 1025, 2048 / 2049 and 3072 / 3073
    out = {"floor": lfe.floor_cases(), "carried": lfe.carried_cases(f_runs=WIDE_CARRIED_F_RUNS), "long_runs": lfe.long_run_cases(waves=MAX_WAVES),
           "borders": lfe.border_cases(), "best_cell": lfe.best_cell_cases(waves=MAX_WAVES, handover_waves=edges)}
    out = {name: [_of_hand(h) for h in hands] for name, hands in out.items()}
    out["path_ties"] = [_of_tie_case(shifted) for shifted, _ in lfe.shifted_path_tie_cases(c0=TIE_C0)]
    assert all(c.fits_wide for cases in out.values() for c in cases)
    return out


def replaced_hands():
    """The names of local_full_affine_edges.hand_groups()'s cases that do not fit the wide domain: each has a counterpart above."""
    return sorted(h.name for make in lfe.hand_groups().values() for h in make() if h.shape[0] > MAX_LEN1 or h.shape[1] > MAX_LEN2)


# ---- c. the global kind's hand families -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def global_families():
    return {"global_" + name: [_of_global_hand(h) for h in hands] for name, hands in gfe.hand_groups().items()}


def families():
    return dict(local_families(), **global_families())


# ---- the long library: stripe edges at 4096 -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_families():
    """For libswmi_wide_long.so, whose stripes are 1024 or 4096 columns wide: the shifted path ties across column 4096, the end
    cell in column 4097 with 1023 columns of padding beside it, and the hand-over from column 4096 to 4097."""
    best = [h for h in lfe.best_cell_cases(waves=MAX_WAVES + 1, handover_waves=(MAX_WAVES,)) if h.shape[1] > MAX_LEN2]
    assert sorted({h.shape[1] for h in best}) == [MAX_LEN2 + 1, MAX_LEN2 + 276]
    return {"long_best_cell": [_of_hand(h) for h in best],
            "long_path_ties": [_of_tie_case(shifted) for shifted, _ in lfe.shifted_path_tie_cases(c0=MAX_LEN2 - 64)]}


# ---- calls --------------------------------------------------------------------------------------------------------------------

def calls_of(cases, relabelling, neighbours=None):
    """[(kind, mask, a32, b32, sm32, gap_open, gap_extend, [(case, index of its first alignment)])]: the cases that share kind,
    mask, matrix and gaps in ONE ragged call under one relabelling (so that wave counts 1 - 4 run side by side), with
    `neighbours` = (a32, b32), alignments of the caller's over all 32 letters, between and around them."""
    rows, cols, filler = relabelling
    groups = {}
    for case in cases:
        groups.setdefault(case.key, []).append(case)
    out = []
    for g, group in enumerate(groups.values()):
        a32, b32, where = [], [], []
        for k, case in enumerate(group):
            if neighbours is not None:
                t = (g + k) % len(neighbours[0])
                a32.append(neighbours[0][t])
                b32.append(neighbours[1][t])
            x, y, sm32 = relabel(case, rows, cols, filler, junk_seed=1000 * g + k)
            where.append((case, len(a32)))
            a32 += x
            b32 += y
        if neighbours is not None:
            a32 += list(neighbours[0])
            b32 += list(neighbours[1])
        c = group[0]
        out.append((c.kind, c.mask, a32, b32, sm32, c.gap_open, c.gap_extend, where))
    return out


def fixed_as_ragged(a, b, r, traceback=True):
    """A fixed-shape 4-letter restatement's (scores, ends, moves[n, words], steps) in the wide results' ragged layout."""
    if not traceback:
        return r[0], r[1], None, None, None
    mo = move_offsets(a, b)
    moves = np.zeros(int(mo[-1]) + 2, np.uint64)
    for k in range(len(a)):
        moves[int(mo[k]):int(mo[k]) + r[2].shape[1]] = r[2][k]
    return r[0], r[1], moves, mo, r[3]


def result_slice(result, first, n):
    """Alignments first .. first + n - 1 of a ragged result as a ragged result of their own."""
    sc, ends, moves, mo, steps = result
    if moves is None:
        return sc[first:first + n], ends[first:first + n], None, None, None
    lo = int(mo[first])
    return sc[first:first + n], ends[first:first + n], moves[lo:], mo[first:first + n + 1] - mo[first], steps[first:first + n]


def assert_pinned(result, first, pinned, what, traceback=True):
    """The hand-worked fields of alignments first .. of a ragged result."""
    sc, ends, _, _, steps = result
    for k, (score, want_ends, codes) in enumerate(pinned, first):
        want_ends = tuple(want_ends) if traceback else (want_ends[0], want_ends[1], -1, -1)
        assert int(sc[k]) == score and tuple(int(x) for x in ends[k]) == want_ends, (what, k, int(sc[k]), ends[k], score, want_ends)
        if traceback and codes is not None:
            assert int(steps[k]) == len(codes) and moves_of(result, k) == list(codes), (what, k, "codes")


# ---- d. the profile census ---------------------------------------------------------------------------------------------------

CENSUS_LANES = (0, te.WAVE // 2 - 1, te.WAVE - 1)           # 0, 31, 63
CENSUS_ROWS = (1, 2, 4, 5, 8, 9, 32, 33, 129)                # trip and chunk edges, lane 63's delay, past a staging block
CENSUS_GAPS = (127, 127)
SHIFTS = tuple(range(LETTERS))


def census_columns():
    """All 16 column positions of lanes 0, 31 and 63 of each wave, 1-based: 192 columns."""
    return [WAVE_COLS * w + COLS * lane + jj + 1 for w in range(MAX_WAVES) for lane in CENSUS_LANES for jj in range(COLS)]


def census_matrix(shift, value=None):
    """M_s[p, (p + s) % 32] = 1 + 3 p (or `value`), -3 elsewhere."""
    sm = np.full((LETTERS, LETTERS), -3, np.int8)
    p = np.arange(LETTERS)
    sm[p, (p + shift) % LETTERS] = 1 + 3 * p if value is None else value
    return sm.reshape(-1)


def _census_letters(p, shift, t):
    """(q, z, y): seq2's letter at the census column, seq2's background letter z != q, seq1's background letter y with
    M_s[y, z] = M_s[y, q] = -3."""
    q = (p + shift) % LETTERS
    z = (q + 1 + t % (LETTERS - 1)) % LETTERS
    y = next(v for v in ((p + 1 + u) % LETTERS for u in range(LETTERS)) if v != p and (v + shift) % LETTERS != z)
    return q, z, y


class Census:
    """One call: sm (flat 32 x 32), a, b (lists over 32 letters with junk bits), kind, mask, and per alignment the closed form
    (score, ends, codes) and what it probes, (column, p, q, row, len2)."""

    def __init__(self, name, kind, mask, sm):
        self.name, self.kind, self.mask, self.sm = name, kind, mask, sm
        self.a, self.b, self.pinned, self.probes = [], [], [], []

    def add(self, rng, seq1, seq2, pinned, probe):
        for seqs, x in ((self.a, seq1), (self.b, seq2)):
            x = np.asarray(x, np.uint8)
            seqs.append((x | (rng.integers(0, 8, len(x), dtype=np.uint8) << 5)).astype(np.uint8))
        self.pinned.append(pinned)
        self.probes.append(probe)


def _len2_for(c, t):
    """c is the last valid column in every other alignment; else 1 .. 29 columns (padding to a correct kernel's neighbours) follow"""
    return c if t % 2 == 0 else min(MAX_LEN2, c + 1 + t % 29)


@functools.lru_cache(maxsize=None)
def census_calls(kind):
    """One Census per shift s (32 calls, one matrix each).  The 192 columns are dealt out to the shifts, six each, by a fixed
    permutation, and each column meets all 32 row letters p in its shift's call: every (column, p) and every (p, q) occurs.
    LOCAL: seq1 = r - 1 background letters then p, r cycling through CENSUS_ROWS; the one positive cell is (r, c): score
    1 + 3 p, ends (r, c, r - 1, c - 1), one diagonal move.  GLOBAL under BEGIN2 | END2: r = 1, the same score and end cell."""
    columns = np.random.default_rng(29100).permutation(census_columns())
    per = len(columns) // len(SHIFTS)
    out = []
    t = 0
    for s in SHIFTS:
        rng = np.random.default_rng(29200 + s)
        cen = Census("census/%s/shift=%d" % ("local" if kind == LOCAL else "global", s), kind, 0 if kind == LOCAL else BEGIN2 | END2, census_matrix(s))
        for c in (int(x) for x in columns[per * s:per * (s + 1)]):
            for p in range(LETTERS):
                t += 1
                r = CENSUS_ROWS[t % len(CENSUS_ROWS)] if kind == LOCAL else 1
                len2 = _len2_for(c, t // len(CENSUS_ROWS))
                q, z, y = _census_letters(p, s, t)
                seq2 = np.full(len2, z, np.uint8)
                seq2[c - 1] = q
                cen.add(rng, [y] * (r - 1) + [p], seq2, (1 + 3 * p, (r, c, r - 1, c - 1), [DIAG]), (c, p, q, r, len2))
        out.append(cen)
    return out


EXTREME_SHIFT = 11


@functools.lru_cache(maxsize=None)
def extreme_census_calls():
    """The second matrix family: `value` in place of 1 + 3 p, for the two values whose sign the cell's extraction must keep.
    LOCAL, 127: the census's alignments of one shift.  GLOBAL under mask 0, 127 and -128: square alignments r = c = len2 of
    CENSUS_ROWS, the special pair in the corner; with gaps (127, 127) a path off the main diagonal pays 254 for its two gap
    moves, more than any cell can cost, so the score is -3 (r - 1) + value along r diagonals, ends (r, r, 0, 0)."""
    s = EXTREME_SHIFT
    rng = np.random.default_rng(29300)
    local = Census("census/local/127", LOCAL, 0, census_matrix(s, 127))
    src = census_calls(LOCAL)[s]
    for x, y, (_, ends, codes), probe in zip(src.a, src.b, src.pinned, src.probes):
        local.add(rng, x & 31, y & 31, (127, ends, codes), probe)
    out = [local]
    for value in (127, -128):
        cen = Census("census/global/%d" % value, GLOBAL, 0, census_matrix(s, value))
        for t, r in enumerate(CENSUS_ROWS):
            for p in range(LETTERS):
                q, z, y = _census_letters(p, s, t + p)
                cen.add(rng, [y] * (r - 1) + [p], [z] * (r - 1) + [q], (-3 * (r - 1) + value, (r, r, 0, 0), [DIAG] * r), (r, p, q, r, r))
        out.append(cen)
    return out


def census_coverage():
    """What the census must reach (asserted by the CPU test): ({(column, p)}, {(p, q)}, {deciding values})."""
    cells, pairs, values = set(), set(), set()
    for cen in census_calls(LOCAL) + census_calls(GLOBAL) + extreme_census_calls():
        sm = cen.sm.reshape(LETTERS, LETTERS)
        for c, p, q, r, len2 in cen.probes:
            cells.add((c, p))
            pairs.add((p, q))
            values.add(int(sm[p, q]))
    return cells, pairs, values


# ---- e. the same census as position-specific profiles --------------------------------------------------------------------------

PROFILE_LEN2S = (1, 16, 17, 1024, 1025, 3073, 4096)
PROFILE_BACKGROUND = 0                                       # the letter that no column rewards


def profile_census_columns(len2):
    """Up to 31 of the census's columns inside len2, column 1 and the last valid column among them, spread over what lies
    between; column k of them rewards letter 1 + (5 k + len2) % 31: distinct letters, never the background.  {column: letter}"""
    inside = sorted({c for c in census_columns() if c <= len2} | {1, len2})
    if len(inside) > LETTERS - 1:
        pick = np.unique(np.round(np.linspace(0, len(inside) - 1, LETTERS - 1)).astype(int))
        inside = [inside[k] for k in pick]
    assert inside[0] == 1 and inside[-1] == len2 and len(inside) <= LETTERS - 1
    return {c: 1 + (5 * k + len2) % (LETTERS - 1) for k, c in enumerate(inside)}


def census_profile(len2):
    """(len2, 32) int8: -3 everywhere, profile[c - 1, p] = 1 + 3 p for the (c, p) of profile_census_columns."""
    prof = np.full((len2, LETTERS), -3, np.int8)
    for c, p in profile_census_columns(len2).items():
        prof[c - 1, p] = 1 + 3 * p
    return prof


@functools.lru_cache(maxsize=None)
def profile_census(len2, kind):
    """(profile, sequences, pinned, mask): LOCAL: [background] * (r - 1) + [p] for every letter p and every r of CENSUS_ROWS;
    a letter that a column rewards gives score 1 + 3 p with ends (r, c, r - 1, c - 1) and one diagonal move, any other letter
    score 0 with no move.  GLOBAL under BEGIN2 | END2: [p] alone: the same score and end cell, or -3 from (0, 0) to (1, 1) where
    no column rewards p (the first of the last row's equal cells)."""
    rng = np.random.default_rng(29400 + len2)
    column_of = {p: c for c, p in profile_census_columns(len2).items()}
    seqs, pinned = [], []
    for r in (CENSUS_ROWS if kind == LOCAL else (1,)):
        for p in range(LETTERS):
            x = np.asarray([PROFILE_BACKGROUND] * (r - 1) + [p], np.uint8)
            seqs.append((x | (rng.integers(0, 8, r, dtype=np.uint8) << 5)).astype(np.uint8))
            if p in column_of:
                c = column_of[p]
                pinned.append((1 + 3 * p, (r, c, r - 1, c - 1), [DIAG]))
            else:
                pinned.append((0, (0, 0, 0, 0), []) if kind == LOCAL else (-3, (1, 1, 0, 0), [DIAG]))
    return census_profile(len2), seqs, pinned, 0 if kind == LOCAL else BEGIN2 | END2


# ---- the traps ---------------------------------------------------------------------------------------------------------------

FAULTS = ("transposed", "letters_masked_with_15", "seq2_shifted_by_one", "filler_changed")


def with_fault(fault, a32, b32, sm32, relabelling=None):
    """The inputs a restatement must be given to compute what a kernel with that one fault would: (a, b, sm)."""
    if fault == "transposed":
        return a32, b32, np.ascontiguousarray(np.asarray(sm32).reshape(LETTERS, LETTERS).T).reshape(-1)
    if fault == "letters_masked_with_15":
        return [x & 15 for x in a32], [y & 15 for y in b32], sm32
    if fault == "seq2_shifted_by_one":
        return a32, [np.roll(y, -1) for y in b32], sm32
    assert fault == "filler_changed" and relabelling is not None
    rows, cols, filler = relabelling
    keep = np.zeros((LETTERS, LETTERS), bool)
    keep[np.ix_(np.asarray(rows), np.asarray(cols))] = True
    other = np.int8(-128 if filler == 127 else 127)
    return a32, b32, np.where(keep, np.asarray(sm32).reshape(LETTERS, LETTERS), other).astype(np.int8).reshape(-1)


def differs(got, want):
    """Does any field (score, end, step count, move) of two ragged results differ?"""
    if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4])):
        return True
    return any(moves_of(got, k) != moves_of(want, k) for k in range(len(got[0])))

