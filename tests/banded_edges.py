"""Constructed inputs for the banded affine scorer (swmi_score_banded_affine) and the edge each one claims.

Convention of oracle/sw_oracle.c: seq1 indexes rows i, seq2 columns j (1-based), diagonal d = j - i, band LO <= d <= HI.
Importable without a device.  test_banded_edges_cpu.py proves every claim made here through the C oracle and through the
two numpy formulations below (neither shares code with the oracle), test_banded_edges_gpu.py sends every case through every
kernel body.  A Case carries `want`: the score of each pair worked out by hand (-1 where no hand value exists and the
oracle's value is taken), and `below`: a bound the oracle's score must stay strictly under (-1: none) -- the score the pair
would have if the diagonal it sits on were inside the band."""
import numpy as np

from conftest import match_matrix
from local_affine_support import AFFINE_GAPS
from local_support import random_matrix

LO, HI = -64, 63                                          # the band of the scorer: 128 diagonals
NEIGHBOUR_BANDS = [(-63, 63), (-65, 63), (-64, 62), (-64, 64)]    # each bound off by one, one at a time
NEG = -(1 << 29)

# len % 4 in {0, 1, 2, 3} (the int32 kernel's trips of four), len % 16 in {0, 1, 15, ...} (the packed kernel's trips of 16),
# both ends of the domain 64 .. 1792
LENGTHS = [64, 65, 66, 67, 79, 80, 81, 128, 333, 334, 1024, 1057, 1791, 1792]
assert {l % 4 for l in LENGTHS} == {0, 1, 2, 3} and {0, 1, 15} <= {l % 16 for l in LENGTHS}
# Only the packed body exists up to len 229 (127 * 229 + 18 * 128 + 254 + 64 < 0x7C00), the plain int32 cell from len 259 on
# (127 * 259 >= 2^15): the int32 bodies are reached at these
BODY_LENGTHS = [333, 334, 1024, 1057, 1791, 1792]
assert {l % 4 for l in BODY_LENGTHS} == {0, 1, 2, 3}
# A shifted copy needs len - |s| matches to stand clear of what random diagonals give: not at 64 .. 81 (|s| up to 66)
SHIFT_LENGTHS = [128] + BODY_LENGTHS
SHIFT_SKIPPED = [64, 65, 66, 67, 79, 80, 81]
# A gap run of up to 65 in the middle needs two halves that are each longer than the run
GAP_LENGTHS = BODY_LENGTHS
GAP_SKIPPED = [64, 65, 66, 67, 79, 80, 81, 128]
# ... and with gaps that cost next to nothing, (0, 0) and (1, 4), free gaps through random sequence drown the signal of
# a cut run below len 1024 (at len 256 the four cases no longer separate the band from its neighbours)
FREE_GAP_LENGTHS = [1024, 1057, 1791, 1792]
# A corner block of 8 one diagonal outside the band at the far end starts at column len - 65 - 7 >= 1
CORNER_LENGTHS = [79, 80, 81, 128] + BODY_LENGTHS
CORNER_SKIPPED = [64, 65, 66, 67]
for _used, _skipped in ((SHIFT_LENGTHS, SHIFT_SKIPPED), (GAP_LENGTHS, GAP_SKIPPED), (CORNER_LENGTHS, CORNER_SKIPPED)):
    assert sorted(_used + _skipped) == LENGTHS

SHIFTS = [-66, -65, -64, -63, -62, 62, 63, 64, 65]
SHIFT_GAPS = [(127, 127), (126, 127)]                     # priced out; open >= extend and open < extend: both kernel bodies
GAP_RUNS = [62, 63, 64, 65]
GAP_SETS = [(5, 1), (20, 0), (0, 0), (1, 4)]
HAND_GAP_SETS = [(5, 1), (20, 0)]                         # the gap sets whose joined score is claimed by hand
BLOCK = np.array([2, 2, 3, 2, 3, 3, 3, 2], np.uint8)      # aperiodic: it matches itself in full on one diagonal only

KERNELS = ["sw_banded_affine_pk_kernel<1>", "sw_banded_affine_pk_kernel<0>", "sw_banded_affine_kernel<1,1>",
           "sw_banded_affine_kernel<0,1>", "sw_banded_affine_kernel<1,0>", "sw_banded_affine_kernel<0,0>"]
BODIES = ["pk", "i16", "i32"]
kBandedTrip = 16
PK_LIMIT = 0x7C00


# ---- two formulations of the recurrence, the band bounds as parameters ---------------------------------------------------

def numpy_banded_gotoh(a, b, sm, gap_open, gap_ext, lo=LO, hi=HI):
    """Independent restatement: anti-diagonal-free, row by row with explicit band mask, int64 arrays."""
    n = len(a)
    sm = np.asarray(sm, np.int64).reshape(4, 4)
    H = np.zeros((n + 1, n + 1), np.int64)
    E = np.full((n + 1, n + 1), NEG, np.int64)
    F = np.full((n + 1, n + 1), NEG, np.int64)
    best = 0
    for i in range(1, n + 1):
        first, last = max(1, i + lo), min(n, i + hi)
        for j in range(first, last + 1):
            E[i, j] = max(E[i, j - 1] - gap_ext, H[i, j - 1] - gap_open)
            F[i, j] = max(F[i - 1, j] - gap_ext, H[i - 1, j] - gap_open)
            H[i, j] = max(0, H[i - 1, j - 1] + sm[a[i - 1] & 3, b[j - 1] & 3], E[i, j], F[i, j])
            best = max(best, H[i, j])
    return int(best)


def band_scores(a, b, sm, gap_open, gap_ext, lo=LO, hi=HI):
    """The same recurrence for a whole batch (a, b: n x len), one anti-diagonal i + j = s at a time over the hi - lo + 1
    diagonals: entry k of every state vector is diagonal lo + k, the cell to the left is entry k - 1 and the cell above entry
    k + 1 of anti-diagonal s - 1, the diagonal predecessor entry k of s - 2.  Cells outside the band or the matrix (and the
    entries of the other parity) hold H = 0, E = F = NEG."""
    a = np.atleast_2d(np.asarray(a)).astype(np.int64) & 3
    b = np.atleast_2d(np.asarray(b)).astype(np.int64) & 3
    n, length = a.shape
    S = np.asarray(sm, np.int64).reshape(4, 4)
    go, ge = int(gap_open), int(gap_ext)
    d = np.arange(lo, hi + 1, dtype=np.int64)
    width = len(d)
    zero = np.zeros((n, width), np.int64)
    none = np.full((n, width), NEG, np.int64)
    H1, H2, E1, F1 = zero, zero, none, none
    best = np.zeros(n, np.int64)
    pad0 = np.zeros((n, 1), np.int64)
    padn = np.full((n, 1), NEG, np.int64)
    for s in range(2, 2 * length + 1):
        i2, j2 = s - d, s + d                              # twice the row and the column
        valid = (i2 % 2 == 0) & (i2 >= 2) & (i2 <= 2 * length) & (j2 >= 2) & (j2 <= 2 * length)
        if not valid.any():
            H1, H2, E1, F1 = zero, H1, none, none
            continue
        i = np.clip(i2 // 2, 1, length) - 1
        j = np.clip(j2 // 2, 1, length) - 1
        E = np.maximum(np.hstack([padn, E1[:, :-1]]) - ge, np.hstack([pad0, H1[:, :-1]]) - go)
        F = np.maximum(np.hstack([F1[:, 1:], padn]) - ge, np.hstack([H1[:, 1:], pad0]) - go)
        H = np.maximum(np.maximum(H2 + S[a[:, i], b[:, j]], 0), np.maximum(E, F))
        H = np.where(valid, H, 0)
        E = np.where(valid, E, NEG)
        F = np.where(valid, F, NEG)
        np.maximum(best, H.max(axis=1), out=best)
        H1, H2, E1, F1 = H, H1, E, F
    return best.astype(np.int32)


# ---- which kernel body a parameter set runs (the host's rule, restated; the GPU file asserts it by name) ----------------

def body_of(length, sm, gap_open, gap_ext):
    """'pk' / 'i16' / 'i32' by the formula of DESIGN.md 9: the packed kernel while
    len * max(s, 0) + (kBandedTrip + 2) * max(0, -min s) + open + extend + 64 < 0x7C00, the 16-bit maxes while len * max(s, 0)
    < 2^15, else the plain int32 cell."""
    top, bias = max(0, int(np.max(sm))), max(0, -int(np.min(sm)))
    if length * top + (kBandedTrip + 2) * bias + gap_open + gap_ext + 64 < PK_LIMIT:
        return "pk"
    return "i16" if length * top < 32768 else "i32"


def kernel_name(length, sm, gap_open, gap_ext):
    body = body_of(length, sm, gap_open, gap_ext)
    oge = int(gap_open >= gap_ext)
    return "sw_banded_affine_pk_kernel<%d>" % oge if body == "pk" else "sw_banded_affine_kernel<%d,%d>" % (oge, body == "i16")


def match_for(length, body, base):
    """The match score that makes a matrix run `body` at this length: `base` in the packed kernel, the largest one below
    2^15 / len for the 16-bit maxes, the smallest one from 2^15 / len on for the plain cell (the generators assert with
    body_of that the whole parameter set does select the body)."""
    m = {"pk": base, "i16": min(127, 32767 // length), "i32": -(-32768 // length)}[body]
    assert 0 < m <= 127, (length, body)
    return m


# ---- cases -----------------------------------------------------------------------------------------------------------------

class Case:
    """n pairs of one length for one (sm, open, extend); labels[k] names the edge pair k claims."""

    def __init__(self, family, name, a, b, sm, gap_open, gap_ext, labels, want=None, below=None):
        self.family, self.name = family, name
        self.a, self.b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
        self.sm, self.gap_open, self.gap_ext = np.asarray(sm, np.int8), int(gap_open), int(gap_ext)
        self.labels = list(labels)
        n = len(self.a)
        self.want = np.full(n, -1, np.int64) if want is None else np.asarray(want, np.int64)
        self.below = np.full(n, -1, np.int64) if below is None else np.asarray(below, np.int64)
        assert len(self.labels) == n == len(self.b) == len(self.want) == len(self.below)

    @property
    def length(self):
        return self.a.shape[1]

    @property
    def kernel(self):
        return kernel_name(self.length, self.sm, self.gap_open, self.gap_ext)

    def what(self, k=None):
        s = "%s len=%d (%d,%d) sm=(%d,%d) %s" % (self.name, self.length, self.gap_open, self.gap_ext, int(self.sm[0]), int(self.sm[1]),
                                                 self.kernel)
        return s if k is None else "%s: %s" % (s, self.labels[k])

    def __repr__(self):
        return self.what()


def shifted_pair(rng, length, s):
    """b[j] = a[j - s], the rest random: the copy lies on diagonal d = s, from one border of the matrix to the other."""
    a = rng.integers(0, 4, length, dtype=np.uint8)
    b = rng.integers(0, 4, length, dtype=np.uint8)
    if s >= 0:
        b[s:] = a[:length - s]
    else:
        b[:length + s] = a[-s:]
    return a, b


def shift_case(length, match, mismatch, gap_open, gap_ext, seed=0):
    """One pair per shift of SHIFTS.  Claim: match * (len - |s|) for LO <= s <= HI -- the copy's diagonal runs from border
    to border and every cell on it matches, no path has more diagonal steps than a border-to-border diagonal leaves rows or
    columns for, and gaps and mismatches only cost; outside the band whatever the random diagonals give, below that."""
    assert length in SHIFT_LENGTHS, "a shifted copy needs len - 66 matches to stand clear of noise: not at %s" % SHIFT_SKIPPED
    rng = np.random.default_rng(7000 + 16 * length + seed)
    pairs = [shifted_pair(rng, length, s) for s in SHIFTS]
    full = np.array([match * (length - abs(s)) for s in SHIFTS])
    inside = np.array([LO <= s <= HI for s in SHIFTS])
    return Case("shift", "shift", [p[0] for p in pairs], [p[1] for p in pairs], match_matrix(match, mismatch), gap_open, gap_ext,
                ["shift %+d" % s for s in SHIFTS], np.where(inside, full, -1), np.where(inside, -1, full))


def gap_run_pair(rng, length, g, insert):
    """a, and b = a with g random bases inserted at len / 2 (the path jumps to d = +g) or g bases deleted there (d = -g)."""
    a = rng.integers(0, 4, length, dtype=np.uint8)
    h = length // 2
    fill = rng.integers(0, 4, g, dtype=np.uint8)
    b = np.concatenate([a[:h], fill, a[h:]])[:length] if insert else np.concatenate([a[:h], a[h + g:], fill])
    return a, b


def gap_run_case(length, match, mismatch, gap_open, gap_ext, seed=0, hand=None):
    """One pair per g of GAP_RUNS, inserted and deleted.  The joined score is match * (len - g) - (open + (g - 1) * extend).
    hand (default: (open, extend) in HAND_GAP_SETS with match 2, mismatch -3): the joined score is claimed exactly where the
    landing diagonal is in the band; where it is not, the run is cut and the score stays below the joined one."""
    assert length in GAP_LENGTHS, "a run of 65 needs two longer halves: not at %s" % GAP_SKIPPED
    hand = (gap_open, gap_ext) in HAND_GAP_SETS if hand is None else hand
    if not hand:
        assert length in FREE_GAP_LENGTHS, "free gaps through random sequence drown a cut run below len 1024"
    rng = np.random.default_rng(9000 + 16 * length + seed)
    pairs, labels, want, below = [], [], [], []
    for insert in (True, False):
        for g in GAP_RUNS:
            pairs.append(gap_run_pair(rng, length, g, insert))
            labels.append("%s %d (%d,%d)" % ("insert" if insert else "delete", g, gap_open, gap_ext))
            joined = match * (length - g) - (gap_open + (g - 1) * gap_ext)
            inside = LO <= (g if insert else -g) <= HI
            want.append(joined if inside and hand else -1)
            below.append(-1 if inside else joined)
    return Case("gap_run", "gap_run", [p[0] for p in pairs], [p[1] for p in pairs], match_matrix(match, mismatch), gap_open, gap_ext,
                labels, want, below)


def corner_placements(length):
    """(label, first row, first column, in band) of the block of 8: its diagonal run starts or ends at a corner of the band,
    or one cell outside it."""
    n = length
    ends = lambda i, j: (i - 7, j - 7)
    out = [("corner (1,1)", 1, 1), ("corner (1,64)", 1, 64), ("corner (65,1)", 65, 1),
           ("corner (len,len)",) + ends(n, n), ("corner (len-63,len)",) + ends(n - 63, n), ("corner (len,len-64)",) + ends(n, n - 64),
           ("outside (1,65)", 1, 65), ("outside (66,1)", 66, 1),
           ("outside (len-64,len)",) + ends(n - 64, n), ("outside (len,len-65)",) + ends(n, n - 65)]
    return [(label, r, c, LO <= c - r <= HI) for label, r, c in out]


def corner_case(length, match, mismatch, gap_open, gap_ext):
    """a all 0, b all 1 (every cell a mismatch) but for BLOCK in both.  Claim: 8 * match where the block's diagonal is in
    the band (a strongly negative mismatch and priced-out gaps leave nothing else), strictly less one diagonal outside."""
    assert length in CORNER_LENGTHS, "the far outside corner starts at column len - 72: not at %s" % CORNER_SKIPPED
    a = np.zeros((10, length), np.uint8)
    b = np.ones((10, length), np.uint8)
    labels, want, below = [], [], []
    for k, (label, r, c, inside) in enumerate(corner_placements(length)):
        assert 1 <= r and r + 7 <= length and 1 <= c and c + 7 <= length, (label, length)
        a[k, r - 1:r + 7] = BLOCK
        b[k, c - 1:c + 7] = BLOCK
        labels.append(label)
        want.append(8 * match if inside else -1)
        below.append(-1 if inside else 8 * match)
    hand = mismatch < 0 and min(gap_open, gap_ext) > 0
    return Case("corner", "corner", a, b, match_matrix(match, mismatch), gap_open, gap_ext, labels, want if hand else None, below)


def related(rng, n, length, sub=0.08, indel=0.02):
    """noisy copies with substitutions and short indels (the generator of test_banded_affine.py)"""
    a = rng.integers(0, 4, (n, length), dtype=np.uint8)
    b = np.zeros_like(a)
    for k in range(n):
        out, i = [], 0
        while len(out) < length:
            r = rng.random()
            if r < indel:
                out.append(rng.integers(0, 4))
            elif r < 2 * indel:
                i += 1
            else:
                out.append(a[k, i % length] if rng.random() > sub else rng.integers(0, 4))
                i += 1
        b[k] = out[:length]
    return a, b


# ---- every family in every body ------------------------------------------------------------------------------------------

# (body, open, extend) of the priced-out families; open >= extend and open < extend select the two instantiations of a body
def _priced_out(length):
    return [(body, go, ge) for body in BODIES if body == "pk" or length in BODY_LENGTHS for go, ge in SHIFT_GAPS]


def shift_cases(lengths=SHIFT_LENGTHS):
    """(2, -3) with gaps priced out in the packed body; in the others the match that selects the body, mismatch -3/2 of it"""
    out = []
    for length in lengths:
        for body, go, ge in _priced_out(length):
            m = match_for(length, body, 2)
            mm = -3 if body == "pk" else max(-128, -(3 * m + 1) // 2)
            assert body_of(length, match_matrix(m, mm), go, ge) == body
            out.append(shift_case(length, m, mm, go, ge))
    return out


def body_gap_set(gaps, match):
    """(open, extend) of GAP_SETS scaled with the match score (GAP_SETS are priced for match 2), each at most 127: a gap
    that did not grow with the match would let free gaps through random sequence outscore the run"""
    k = match // 2
    return tuple(min(127, g * k) for g in gaps)


def gap_run_cases(lengths=GAP_LENGTHS):
    """(2, -3) with every gap set of GAP_SETS in the packed body; in the int32 bodies the match that selects the body,
    mismatch -3/2 of it and the gap set scaled likewise (body_gap_set).  Hand values for (5, 1) and (20, 0) and their
    multiples; (0, 0) and (1, 4) from len 1024 on only (FREE_GAP_LENGTHS)."""
    out = []
    for length in lengths:
        for gaps in GAP_SETS:
            if gaps not in HAND_GAP_SETS and length not in FREE_GAP_LENGTHS:
                continue                                   # stated in FREE_GAP_LENGTHS: no signal there
            for body in BODIES:
                m = match_for(length, body, 2)
                mm = -3 if body == "pk" else max(-128, -(3 * m + 1) // 2)
                go, ge = body_gap_set(gaps, m)
                assert body_of(length, match_matrix(m, mm), go, ge) == body and (go >= ge) == (gaps[0] >= gaps[1])
                out.append(gap_run_case(length, m, mm, go, ge, hand=gaps in HAND_GAP_SETS))
    return out


def corner_cases(lengths=CORNER_LENGTHS):
    """(5, -30) with gaps priced out in the packed body, (match of the body, -128) in the others; and match_matrix(3, 1),
    where the pad score equals true zero (B = 0) and the main diagonal decides: no hand value, no claim about the band --
    it is there for a kernel that lets cells past the end of a sequence add to the maximum."""
    out = []
    for length in lengths:
        for body, go, ge in _priced_out(length):
            m = match_for(length, body, 5)
            mm = -30 if body == "pk" else -128
            assert body_of(length, match_matrix(m, mm), go, ge) == body
            out.append(corner_case(length, m, mm, go, ge))
        for go, ge in SHIFT_GAPS:
            c = corner_case(length, 3, 1, go, ge)
            c.name, c.below = "corner_positive", np.full(len(c.a), -1, np.int64)
            out.append(c)
    return out


FAMILIES = {"shift": shift_cases, "gap_run": gap_run_cases, "corner": corner_cases}


def bias_cost_params():
    """(sm, open, extend, B, cost) of the packed kernel with B = max(0, -min s) in {cost - 1, cost, cost + 1}: cost = extend
    where open >= extend (three kinds: open > extend, open = extend), cost = open otherwise; cost = 0 and B = 0 included.
    The hand-over addend B - cost is a plain per-half addend for B >= cost and a two's-complement pair for B < cost."""
    out = []
    for cost in (0, 1, 5, 20, 126):
        for bias in (cost - 1, cost, cost + 1):
            if bias < 0 or bias > 128:
                continue
            for go, ge in ((min(127, cost + 3), cost), (cost, cost), (cost, min(127, cost + 4))):     # cost 126: (127, 126), (126, 127)
                if (go >= ge and ge != cost) or (go < ge and go != cost):
                    continue
                sm = match_matrix(3, -bias) if bias else match_matrix(3, 1)        # B = 0: no negative score at all
                out.append((sm, go, ge, bias, cost))
    return out


def mixed_batch(case, seed=1):
    """The case's pairs, each next to an unrelated random pair (one wavefront of the packed kernel scores pairs 2k and
    2k + 1 in the two halves of its registers), n odd (the last wavefront scores its pair twice).  Returns (a, b, index of
    each case pair in the batch)."""
    rng = np.random.default_rng(seed + case.length)
    n = len(case.a)
    a = rng.integers(0, 4, (2 * n + 1, case.length), dtype=np.uint8)
    b = rng.integers(0, 4, (2 * n + 1, case.length), dtype=np.uint8)
    at = 2 * np.arange(n)
    a[at], b[at] = case.a, case.b
    a[-1], b[-1] = case.a[0], case.b[0]
    return a, b, at


def swap_halves(x):
    """pairs 2k and 2k + 1 exchanged (the last one of an odd batch stays)"""
    perm = np.arange(len(x))
    even = len(x) & ~1
    perm[:even] = perm[:even] ^ 1
    return x[perm], perm


# ---- the pin through the unbanded affine local aligner (len 128) ---------------------------------------------------------

def in_band(path, lo=LO, hi=HI):
    """every cell (i, j) of a path on a diagonal lo <= j - i <= hi"""
    d = np.asarray(path)[:, 1].astype(np.int64) - np.asarray(path)[:, 0]
    return bool((d >= lo).all() and (d <= hi).all())


def cross_pin_inputs():
    """120 pairs of 128-mers: related ones, 20 unrelated, 20 rolled by 40 .. 89 in either direction (half of those leave
    the band)"""
    rng = np.random.default_rng(128)
    a, b = related(rng, 120, 128, sub=0.08, indel=0.03)
    b[80:100] = rng.integers(0, 4, (20, 128), dtype=np.uint8)
    for k in range(100, 120):
        b[k] = np.roll(a[k], int(rng.integers(40, 90)) * (1 if k % 2 else -1))
    return a, b


CROSS_PIN_MATRICES = [match_matrix(2, -3), match_matrix(1, -1), random_matrix(), match_matrix(5, -4)]


def cross_pin(a, b, banded, align, expand):
    """banded(sm, go, ge) -> scores, align(sm, go, ge) -> (scores, ends, moves, steps) of the unbanded affine local aligner:
    banded <= unbanded everywhere, equal wherever the reported optimal path stays in the band.  Returns (cases, in band,
    strictly lower out of band)."""
    cases = inside = lower = 0
    for sm in CROSS_PIN_MATRICES:
        for go, ge in AFFINE_GAPS:
            got = banded(sm, go, ge)
            sc, ends, moves, steps = align(sm, go, ge)
            for k in range(len(a)):
                path = expand(moves[k], steps[k], ends[k, 0], ends[k, 1])
                cases += 1
                assert got[k] <= sc[k], (k, go, ge, int(got[k]), int(sc[k]))
                if in_band(path):
                    inside += 1
                    assert got[k] == sc[k], (k, go, ge, int(got[k]), int(sc[k]))
                else:
                    lower += int(got[k] < sc[k])
    return cases, inside, lower
