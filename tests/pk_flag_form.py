"""The FLAG FORM of the packed scorer's vertical-offset kernel (sw_kernels.hip "FLAG FORM", csrc/pk_form.h): the
host rule restated, a table of parameter sets on both sides of each of its conditions, a numpy model of the cell on 16-bit
patterns, and a small structured batch.  Importable without a device; test_pk_flag_form_cpu.py and test_gpu_pk_flag_form.py
use it.

The form: when every score is either one value m or <= -2 gap (which never decides a cell), the recurrence rescaled by
255 / (m + gap) runs on q0's 8-instruction cell with ONE flag bit per matrix entry: the looked-up addend is 0x00FF (the folded
score m + gap, rescaled: 255) or 0x80FF, which turns the diagonal term into a finite negative half-precision pattern that
v_pk_maximum3_f16 drops."""
from collections import namedtuple

import numpy as np

import pk_edges as pe
from conftest import match_matrix

PK_LIMIT = pe.PK_LIMIT
FORMS = ("q0", "bias", "vert", "flag")      # what swmi_pk_cell_form returns: 0, 1, 2, 3


def flag_rule(sm, gap):
    """(m + gap, rescaled gap) when the flag form applies, else None: the existing rule gives the vertical-offset kernel; every
    entry is one value m with m + gap > 0, or <= -2 gap; (m + gap) divides 255 gap; 255 (128 m + gap) / (m + gap) + 255 < 0x7C00"""
    sm = [int(v) for v in np.asarray(sm).reshape(16)]
    gap = int(gap)
    if pe.expected_variant(sm, gap) != "vert":
        return None
    enabled = sorted(set(s for s in sm if s > -2 * gap))
    if len(enabled) != 1:
        return None
    unit = enabled[0] + gap
    if unit <= 0 or (255 * gap) % unit:
        return None
    if not 255 * (128 * enabled[0] + gap) + 255 * unit < PK_LIMIT * unit:
        return None
    return unit, 255 * gap // unit


def expected_form(sm, gap):
    return "flag" if flag_rule(sm, gap) else pe.expected_variant(sm, gap)


def matrix_of(enabled_cells, m, other):
    """4x4 matrix with m at the listed (seq1 base, seq2 base) cells and `other` elsewhere"""
    sm = np.full((4, 4), other, np.int8)
    for a, b in enabled_cells:
        sm[a, b] = m
    return sm.reshape(16)


DIAGONAL = [(0, 0), (1, 1), (2, 2), (3, 3)]
# the diagonal and two off-diagonal cells whose mirror images stay disabled: the kernel keeps the TRANSPOSED table in LDS, and
# a symmetric matrix hides a transposition error.  Bases {0, 1} against {2, 3} stay disjoint (every cell disabled).
ASYMMETRIC = DIAGONAL + [(0, 1), (3, 2)]

RuleSet = namedtuple("RuleSet", "label sm gap form scale")      # form, scale = (m + gap, rescaled gap): claimed here by hand

RULE_SETS = [
    RuleSet("headline 10/-30 gap 15", match_matrix(10, -30), 15, "flag", (25, 153)),
    RuleSet("strict 10/-40 gap 15: s < -2 gap, which the vertical-offset rule does not take", match_matrix(10, -40), 15, "bias", None),
    RuleSet("10/-29 gap 15: two enabled values", match_matrix(10, -29), 15, "vert", None),
    RuleSet("7/-30 gap 15: 22 does not divide 255 * 15", match_matrix(7, -30), 15, "vert", None),
    RuleSet("127/-127 gap 64", match_matrix(127, -127), 64, "vert", None),
    RuleSet("120/-120 gap 62", match_matrix(120, -120), 62, "vert", None),
    RuleSet("10/-30 gap 30: every s + gap >= 0", match_matrix(10, -30), 30, "q0", None),
    RuleSet("10/-30 gap 14: below the vertical-offset rule", match_matrix(10, -30), 14, "bias", None),
    RuleSet("16/-2 gap 1: largest value 30 990", match_matrix(16, -2), 1, "flag", (17, 15)),
    RuleSet("50/-2 gap 1: largest value 32 260 >= 0x7C00", match_matrix(50, -2), 1, "vert", None),
    RuleSet("-10/-30 gap 15: m < 0, every score 0", match_matrix(-10, -30), 15, "flag", (5, 765)),
    RuleSet("-15/-30 gap 15: m + gap = 0", match_matrix(-15, -30), 15, "vert", None),
    RuleSet("-20/-30 gap 15: m + gap < 0", match_matrix(-20, -30), 15, "vert", None),
    RuleSet("all -30 gap 15: no enabled entry", np.full(16, -30, np.int8), 15, "vert", None),
    RuleSet("asymmetric 10/-30 gap 15", matrix_of(ASYMMETRIC, 10, -30), 15, "flag", (25, 153)),
    RuleSet("asymmetric with a second enabled value", np.where(np.arange(16) == 1, 9, matrix_of(ASYMMETRIC, 10, -30)).astype(np.int8), 15, "vert", None),
    RuleSet("2/-6 gap 3: m + gap = 5 divides 765", match_matrix(2, -6), 3, "flag", (5, 153)),
    RuleSet("36/-30 gap 15: m + gap = 51", match_matrix(36, -30), 15, "flag", (51, 75)),
]

# what the GPU test runs: two eligible sets, the strict set (bias kernel) and the ineligible neighbour (vertical-offset cell)
GPU_SETS = [RULE_SETS[0], RULE_SETS[1], RULE_SETS[14], RULE_SETS[2]]


# ---- the cell on 16-bit patterns -------------------------------------------------------------------------------------------

def flag_model(a, b, sm, gap, unit, scaled_gap):
    """The flag cell for a batch, every value a 16-bit pattern as the kernel holds it (one anti-diagonal at a time):
        t = H(i-1,j-1) + (0x00FF enabled | 0x80FF disabled)         a 16-bit add: must not carry out of the half
        x = max3(H(i,j-1), H(i-1,j), t) by the half-precision order: a pattern with the sign bit set loses
        H = x -sat scaled_gap;  best = max x;  score = max(best - scaled_gap, 0) * unit / 255
    Returns (scores, H[129, 129, n] rescaled, dict of the extreme patterns held)."""
    a, b = np.asarray(a) & 3, np.asarray(b) & 3
    sm = np.asarray(sm, np.int64).reshape(4, 4)
    disabled = sm[a.T[:, None, :], b.T[None, :, :]] <= -2 * gap             # [i-1, j-1, pair]
    addend = np.where(disabled, 0x80FF, 0x00FF).astype(np.int64)
    n = len(a)
    H = np.zeros((129, 129, n), np.int64)
    best = np.zeros(n, np.int64)
    seen = dict(max_enabled=0, min_enabled=0xFFFF, max_negative_magnitude=0, min_negative_magnitude=0xFFFF, carries=0, max_x=0)
    for d in range(2, 257):
        i = np.arange(max(1, d - 128), min(128, d - 1) + 1)
        j = d - i
        t = H[i - 1, j - 1] + addend[i - 1, j - 1]
        seen["carries"] += int((t > 0xFFFF).sum())
        t &= 0xFFFF
        neg = (t & 0x8000) != 0
        if neg.any():
            mag = t[neg] & 0x7FFF
            seen["max_negative_magnitude"] = max(seen["max_negative_magnitude"], int(mag.max()))
            seen["min_negative_magnitude"] = min(seen["min_negative_magnitude"], int(mag.min()))
        if (~neg).any():
            seen["max_enabled"] = max(seen["max_enabled"], int(t[~neg].max()))
            seen["min_enabled"] = min(seen["min_enabled"], int(t[~neg].min()))
        x = np.maximum(np.maximum(H[i, j - 1], H[i - 1, j]), np.where(neg, -1, t))
        seen["max_x"] = max(seen["max_x"], int(x.max()))
        best = np.maximum(best, x.max(axis=0))
        H[i, j] = np.maximum(x - scaled_gap, 0)
    rescaled = np.maximum(best - scaled_gap, 0) * unit
    assert not (rescaled % 255).any(), "the best value is not a multiple of 255 / (m + gap)"
    return rescaled // 255, H, seen


# ---- a small structured batch ----------------------------------------------------------------------------------------------

LANE_BOUNDARIES = list(range(8, 128, 8))     # first row of a lane for R = 8 (every one), 16 and 32 rows per lane


def build_batch(seed=7):
    """(seq1s, seq2s, labels), 81 pairs: homopolymers against themselves (128 matches: the top of the range), disjoint alphabets
    (every score 0), a single matching row / column, a run of matches across each lane boundary on a background without any, on
    the main diagonal and shifted by five columns, random pairs and mutated copies (gaps)."""
    rng = np.random.default_rng(seed)
    A, B, labels = [], [], []

    def add(a, b, label):
        A.append(np.asarray(a, np.uint8).copy())
        B.append(np.asarray(b, np.uint8).copy())
        labels.append(label)
    for x in range(4):
        add(pe.homopolymer(x), pe.homopolymer(x), "homopolymer %d / %d" % (x, x))
    for k in range(4):
        add(rng.integers(0, 2, 128), rng.integers(2, 4, 128), "disjoint alphabets %d" % k)
    for i in (1, 32, 33, 128):
        add(pe.single_row(i), pe.homopolymer(1), "single matching row %d" % i)
    for j in (1, 64, 128):
        add(pe.homopolymer(1), pe.single_column(j), "single matching column %d" % j)
    for shift in (0, 5):
        for edge in LANE_BOUNDARIES:
            a = rng.integers(0, 2, 128).astype(np.uint8)
            b = rng.integers(2, 4, 128).astype(np.uint8)
            lo, hi = edge - 3, edge + 3                     # rows lo+1 .. hi (1-based): three on either side of the boundary
            a[lo:hi] = rng.integers(2, 4, hi - lo)          # (the run in seq2's alphabet, so that nothing else of seq1 matches it)
            b[lo + shift:hi + shift] = a[lo:hi]
            add(a, b, "run across row %d, columns shifted by %d" % (edge, shift))
    for k in range(20):
        add(rng.integers(0, 4, 128), rng.integers(0, 4, 128), "random %d" % k)
    for k in range(16):
        a = rng.integers(0, 4, 128).astype(np.uint8)
        b = np.where(rng.random(128) < 0.85, a, rng.integers(0, 4, 128)).astype(np.uint8)
        cut = int(rng.integers(20, 100))
        b = np.concatenate([b[:cut], b[cut + 1 + k % 3:], rng.integers(0, 4, 1 + k % 3).astype(np.uint8)])      # a deletion of 1..3
        add(a, b, "mutated copy %d" % k)
    return np.array(A), np.array(B), labels
