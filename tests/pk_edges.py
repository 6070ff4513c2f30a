"""Parameter sets and a structured batch for the packed scorer sw128_pk_kernel<MODE, VARIANT, L> at the edges of the range
argument its three cell bodies rest on (sw_kernels.hip "packed kernel", gen_pk_sweeps.py):

  * every 16-bit half stays a finite half-precision pattern, 0 <= v < 0x7C00;
  * no half carries into its neighbour (the 32-bit adds on a packed pair, the 64-bit v_lshl_add_u64 on a register pair);
  * every row byte  s + gap + Q  (vert: s + 2 gap)  fits 0..255;
  * the host rule (swmi_api.cpp make_config, restated in `expected_variant`) sends each set to a body whose domain holds it.

Importable without a device.  test_pk_edges_cpu.py proves, through a numpy restatement of the recurrence that keeps every H
matrix, that the table and the batch stand on those edges; test_gpu_pk_edges.py sends them through all 27 instantiations by
name and through every other schedule, bit-exact against oracle/sw_oracle.c."""
from collections import namedtuple

import numpy as np

from conftest import match_matrix

MODES = {"pairs": 0, "packed2bit": 1, "one_vs_many": 2}
VARIANTS = ("q0", "bias", "vert")      # template argument 0, 1, 2
LANES = (4, 8, 16)                     # lanes per pair of alignments; 128 / L rows per lane, 128 / L alignments per wavefront
PK_LIMIT = 0x7C00                      # first half-precision bit pattern that is not a finite number


def expected_variant(sm, gap):
    """The packed cell body for these parameters (include/swmi.h, "schedules"):
    q0    every sm + gap >= 0: no bias at all
    vert  some sm + gap < 0 but every sm + 2 gap in [0, 255] and the row offsets fit: vertical-offset form
    bias  everything else: values shifted by Q = -(min sm + gap)"""
    sm = np.asarray(sm, np.int32)
    gap = int(gap)
    if sm.min() + gap >= 0:
        return "q0"
    if sm.min() + 2 * gap >= 0 and sm.max() + 2 * gap <= 255 and 128 * max(0, int(sm.max())) + 34 * gap + 256 < 0x7C00:
        return "vert"
    return "bias"


def expected_name(mode, variant, lanes):
    v = VARIANTS.index(variant)
    return "sw128_pk_kernel<%d,%d>" % (mode, v) if lanes == 4 else "sw128_pk_kernel<%d,%d,%d>" % (mode, v, lanes)


# ---- the parameter table ---------------------------------------------------------------------------------------------------

ParamSet = namedtuple("ParamSet", "label sm gap variant")      # variant: the body the rule must give (claimed here by hand)


def _mm(variant, match, mismatch, gap, note=""):
    return ParamSet("%s %d/%d gap %d%s" % (variant, match, mismatch, gap, note and " " + note), match_matrix(match, mismatch), gap, variant)


def asymmetric_matrix(seed, lo, hi):
    """16 entries in [lo, hi] with sm[0][1] = lo and sm[1][0] = hi, a positive diagonal, and sm[a][b] != sm[b][a] for every
    a != b: the kernel keeps the TRANSPOSED table in LDS (lds_tab), and a symmetric matrix hides a transposition error."""
    rng = np.random.default_rng(seed)
    while True:
        sm = rng.integers(lo, hi + 1, (4, 4))
        np.fill_diagonal(sm, rng.integers(max(1, hi // 2), hi + 1, 4))
        sm[0, 1], sm[1, 0] = lo, hi
        if all(sm[a, b] != sm[b, a] for a in range(4) for b in range(a)):
            return sm.astype(np.int8).reshape(16)


def _asym(variant, seed, lo, hi, gap, note):
    return ParamSet("%s asymmetric %d..%d gap %d %s" % (variant, lo, hi, gap, note), asymmetric_matrix(seed, lo, hi), gap, variant)


PARAM_SETS = [
    # q0: every s + gap >= 0; row byte s + gap
    ParamSet("q0 all 127 gap 0", np.full(16, 127, np.int8), 0, "q0"),                 # the largest H everywhere, 16 256
    _mm("q0", 127, -127, 127, "bytes 254 and 0"),                                     # min + gap = 0
    _mm("q0", 127, -1, 1),                                                            # min + gap = 0
    _mm("q0", 10, -30, 30),                                                           # min + gap = 0
    _mm("q0", 1, -1, 1),
    _mm("q0", 0, 0, 0, "every score 0"),
    _asym("q0", 1, -127, 127, 127, "bytes 0 and 254"),
    _asym("q0", 2, -3, 127, 3, "bytes 0 and 130"),
    # vert: some s + gap < 0, every s + 2 gap in [0, 255]; row byte s + 2 gap
    _mm("vert", 127, -128, 64, "bytes 0 and 255"),                                    # min + 2 gap = 0 and max + 2 gap = 255
    _mm("vert", 127, -127, 64, "byte 255"),
    _mm("vert", 127, -126, 63, "byte 0"),
    _mm("vert", 127, -2, 1, "smallest gap, largest scores"),                          # min + gap = -1, min + 2 gap = 0
    _mm("vert", 1, -2, 1),
    _mm("vert", 10, -30, 15),
    _mm("vert", 10, -30, 29),                                                         # min + gap = -1: the neighbour of q0's (10/-30, 30)
    _mm("vert", -1, -128, 64, "every score 0"),
    _asym("vert", 3, -128, 127, 64, "bytes 0 and 255"),
    _asym("vert", 4, -40, 127, 20, "byte 0 = -2 gap"),
    _asym("vert", 5, -128, 55, 100, "byte 255 = 255 - 2 gap"),
    # bias: everything else; Q = -(min s + gap), row byte s + gap + Q = s - min s
    _mm("bias", 127, -128, 0, "Q = 128, byte 255"),
    ParamSet("bias all -128 gap 0", np.full(16, -128, np.int8), 0, "bias"),
    _mm("bias", 127, -128, 63),                                                       # min + 2 gap = -2: below the vert set
    _mm("bias", 127, -128, 65),                                                       # max + 2 gap = 257: above the vert set
    _mm("bias", 126, -128, 65),                                                       # max + 2 gap = 256: the first that does not fit
    _mm("bias", 127, -128, 127, "Q = 1"),                                             # min + gap = -1, far beyond vert's byte range
    _mm("bias", 127, -3, 1),                                                          # min + 2 gap = -1
    _mm("bias", 1, -3, 1),
    _mm("bias", 10, -30, 14),                                                         # min + 2 gap = -2
    _asym("bias", 6, -128, 127, 0, "Q = 128, bytes 0 and 255"),
    _asym("bias", 7, -128, 127, 65, "Q = 63"),
    _asym("bias", 8, -128, 127, 127, "Q = 1"),
]


def sets_of(variant):
    return [p for p in PARAM_SETS if p.variant == variant]


def row_bytes(sm, gap, variant):
    """what make_config puts into the kernel's rows for this body (before the cast to a byte)"""
    sm = np.asarray(sm, np.int64)
    add = {"q0": gap, "vert": 2 * gap, "bias": gap - int(sm.min() + gap)}[variant]
    return sm + add


# ---- the structured batch --------------------------------------------------------------------------------------------------

LANE_EDGE_ROWS = [1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 96, 97, 127, 128]      # first and last rows of a lane for R = 8, 16, 32
SINGLE_COLUMNS = [1, 2, 64, 127, 128]       # column 1: the pipeline fill; column 128: lane 0 drains L - 1 steps past the end
RUN_LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33]
RUN_POSITIONS = [8, 16, 32, 64, 96]
ROTATIONS = [1, 8, 16, 32, 64, 127]
SHARED_ENDS = [1, 7, 8, 9, 31, 32, 33, 64, 127]


def homopolymer(x):
    return np.full(128, x, np.uint8)


def single_row(i):
    """seq1 of a single-match pair: base 0 with a 1 at row i (1-based)"""
    a = np.zeros(128, np.uint8)
    a[i - 1] = 1
    return a


def single_column(j):
    """seq2 of a single-match pair: base 2 with a 1 at column j (1-based)"""
    b = np.full(128, 2, np.uint8)
    b[j - 1] = 1
    return b


def build_batch(seq2=None, seed=1):
    """(seq1s, seq2s, labels): 197 pairs.  With `seq2` that sequence is every pair's second one (one-vs-many) and every
    constructed relation is built around it as a seq1: the copy with a run inserted (rows without a column: the vertical gap
    run) and the copy with the run deleted (the horizontal one), both rotations, the shared ends; `self` is the one pair of
    identical sequences.  Homopolymers and single matches, whose construction dictates seq2, keep their seq1 only --
    ovm_batches() gives them their seq2 in batches of their own."""
    rng = np.random.default_rng(seed)
    A, B, labels = [], [], []
    base = (lambda: rng.integers(0, 4, 128).astype(np.uint8)) if seq2 is None else (lambda: np.asarray(seq2, np.uint8).copy())

    def add(a, b, label):
        A.append(np.asarray(a, np.uint8).copy())
        B.append(np.asarray(b, np.uint8).copy())
        labels.append(label)
    for x in range(4):                      # all 16 homopolymer pairs: the largest score 128 sm[x][x], and 0 where sm[x][y] <= 0
        for y in range(4):
            add(homopolymer(x), homopolymer(y), "homopolymer %d / %d" % (x, y))
    r = base()
    add(r, r, "self")
    for i in LANE_EDGE_ROWS:                # one matching cell at (i, j), every other cell a mismatch
        for j in SINGLE_COLUMNS:
            add(single_row(i), single_column(j), "single match at (%d, %d)" % (i, j))
    for pos in RUN_POSITIONS:               # a copy with one run deleted: a vertical / horizontal gap run across the lanes' hand-over
        for k in RUN_LENGTHS:
            a = base()
            fill = rng.integers(0, 4, k).astype(np.uint8)
            b = np.concatenate([a[:pos], a[pos + k:], fill])[:128]
            if seq2 is None:
                add(a, b, "run of %d deleted at %d" % (k, pos))       # seq2 lacks rows pos+1 .. pos+k of seq1: a vertical gap run
                add(b, a, "run of %d inserted at %d" % (k, pos))      # seq2 has k columns more: a horizontal gap run
            else:                           # the same two relations with the shared sequence in second place
                add(np.concatenate([a[:pos], fill, a[pos:]])[:128], a, "run of %d deleted at %d" % (k, pos))
                add(b, a, "run of %d inserted at %d" % (k, pos))
    for s in ROTATIONS:
        a = base()
        add(np.roll(a, -s) if seq2 is not None else a, np.roll(a, s), "rotated by %d" % s)
        add(np.roll(a, s), a, "rotated by -%d" % s)
    for k in SHARED_ENDS:                   # a matching prefix / suffix over guaranteed mismatches
        a = base()
        other = (a + 1 + rng.integers(0, 3, 128)) & 3
        pre, suf = other.copy(), other.copy()
        pre[:k] = a[:k]
        suf[-k:] = a[-k:]
        add(pre, a, "shared prefix of %d" % k)
        add(suf, a, "shared suffix of %d" % k)
    A, B = np.array(A), np.array(B)
    if seq2 is not None:
        B[:] = np.asarray(seq2, np.uint8)
    return A, B, labels


def extreme_blocks():
    """two blocks of 24 pairs: (homopolymer match, homopolymer mismatch) for every x != y, then (mismatch, match): the
    largest score beside the smallest in one register, in both orders of the halves"""
    A, B = [], []
    for first_is_match in (True, False):
        for x in range(4):
            for y in range(4):
                if x != y:
                    duo = [(x, x), (x, y)] if first_is_match else [(x, y), (x, x)]
                    for p, q in duo:
                        A.append(homopolymer(p))
                        B.append(homopolymer(q))
    return np.array(A), np.array(B)


def place(a, b):
    """Two alignments share a register as its low and high halves (pairs 2k and 2k + 1 of a batch).  The built batch, then
    the same batch once more shifted to the other parity -- rotated by one pair when its length is even; an odd length
    shifts it already -- then extreme_blocks(): every built pair sits in each half once, each time beside a different
    partner.  Returns (seq1s, seq2s, index of the built pair at each position or -1)."""
    n = len(a)
    second = np.roll(np.arange(n), -1) if n % 2 == 0 else np.arange(n)
    xa, xb = extreme_blocks()
    origin = np.concatenate([np.arange(n), second, np.full(len(xa), -1)])
    return np.concatenate([a, a[second], xa]), np.concatenate([b, b[second], xb]), origin


def with_junk(seqs, seed=99):
    """the same bases with random bits 2..7 in every byte (the byte entries score seq & 3)"""
    rng = np.random.default_rng(seed)
    return (seqs & 3) | (rng.integers(0, 64, seqs.shape).astype(np.uint8) << 2)


def tail_sizes(lanes, n):
    """prefixes that leave a register half, a lane group, a wavefront partly filled; and the batch without its last pair"""
    per_wave = 128 // lanes
    return [1, 2, per_wave - 1, per_wave + 1, 4 * per_wave + 1, n - 1]


OVM_SEED = 2


def ovm_batches():
    """[(label, seq1s, seq2)] for one-vs-many: the batch built around one random seq2 (one self-pair, gap runs in both
    directions, both rotations, shared ends); then the pairs batch's seq1s against each homopolymer (with its 4 homopolymer
    seq1s: all 16 homopolymer pairs, the extremes) and against each single-match seq2 (with its 14 single-match seq1s: one
    matching cell in each lane-edge row)."""
    shared = np.random.default_rng(OVM_SEED).integers(0, 4, 128).astype(np.uint8)
    out = [("around a random seq2", build_batch(shared)[0], shared)]
    a = build_batch()[0]
    out += [("against homopolymer %d" % y, a, homopolymer(y)) for y in range(4)]
    out += [("against the single-match seq2 of column %d" % j, a, single_column(j)) for j in SINGLE_COLUMNS]
    return out


# ---- the recurrence, restated; and the values each cell body holds -----------------------------------------------------------

def numpy_sw(a, b, sm, gap):
    """The recurrence of sw_kernels.hip's header for a batch, int64, every H kept:
        H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),  H(0,.) = H(.,0) = 0
    one anti-diagonal i + j = d at a time.  Returns (H[129, 129, n], S[128, 128, n]) with S[i-1, j-1] the score of cell (i, j);
    the score of pair k is H[:, :, k].max()."""
    a, b = np.asarray(a) & 3, np.asarray(b) & 3
    sm = np.asarray(sm, np.int64).reshape(4, 4)
    S = sm[a.T[:, None, :], b.T[None, :, :]]
    H = np.zeros((129, 129, len(a)), np.int64)
    for d in range(2, 257):
        i = np.arange(max(1, d - 128), min(128, d - 1) + 1)
        j = d - i
        H[i, j] = np.maximum(np.maximum(0, H[i - 1, j - 1] + S[i - 1, j - 1]), np.maximum(H[i - 1, j], H[i, j - 1]) - gap)
    return H, S


def held_values(H, S, sm, gap, variant, rows_per_lane):
    """(smallest, largest) value a 16-bit half holds when the body `variant` walks these H matrices with R rows per lane
    (gen_pk_sweeps.py header, pk_two_rows).  x = the cell's max3 result is the maximum of three of the listed values.
      q0    H;  t = H(i-1,j-1) + s + gap
      bias  also H + Q, (H + gap) + Q = x + Q and t = H(i-1,j-1) + s + gap + Q
      vert  L = H + D_r, D_r = gap (r + 1), r = (i - 1) mod R;  t = L_{r-1}(i-1,j-1) + s + 2 gap -- for r = 0 the lane before
            hands over H itself: t = H(i-1,j-1) + s + 2 gap and up = H(i-1,j) + D_0.  For r > 0 the kernel's `up` is the row
            above's max3 result as it is, unfloored: at most H(i-1,j) + D_r, and equal to it whenever it is >= D_r.  The term
            listed for it here is that BOUND, not the value held; the largest values of every set are reached through t."""
    diag, up, left, here = H[:-1, :-1], H[:-1, 1:], H[1:, :-1], H[1:, 1:]
    if variant == "q0":
        held = [here, diag + S + gap]
    elif variant == "bias":
        q = -(int(np.asarray(sm, np.int64).min()) + gap)
        held = [here, here + q, diag + S + gap + q, left + q, up + q]
    else:
        r = ((np.arange(1, 129) - 1) % rows_per_lane)[:, None, None]
        held = [here, here + gap * (r + 1), diag + gap * r + S + 2 * gap, left + gap * (r + 1), up + gap * (r + 1)]
    return min(int(v.min()) for v in held), max(int(v.max()) for v in held)
