"""Hand-built inputs for the affine global / free-end-gap aligner, each with the fields worked out here.  Shared by
test_global_full_affine_gpu.py (the 4-letter kernels, every field bit-exact on the GPU and on the restatement) and, relabelled
over 32 letters, by wide_edges.py (test_wide_edges_cpu.py, test_wide_edges_gpu.py).

Background: seq1 all 0, seq2 all 1, so nothing matches but what a case plants with bases 2 and 3."""
import numpy as np

from conftest import match_matrix
from global_full_support import BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP

DIAG, UP, LEFT = 3, 2, 1
K111 = match_matrix(1, -1)
K54 = match_matrix(5, -4)
K23 = match_matrix(2, -3)
K1_127 = match_matrix(1, -127)
END_CELL_TIE_SHAPES = ((40, 1100), (1100, 40))


def background(len1, len2, n=1):
    return np.zeros((n, len1), np.uint8), np.ones((n, len2), np.uint8)


def fit_case():
    """All of seq1 = P (150 bases of {2, 3}) inside seq2 at column offset 1000; (L, off, len2, a, b)."""
    L, off, len2 = 150, 1000, 2100
    P = np.random.default_rng(6).integers(2, 4, L).astype(np.uint8)
    a = P[None, :].copy()
    _, b = background(L, len2)
    b[0, off:off + L] = P
    return L, off, len2, a, b


def column_fit_case():
    """seq2 = P of 1025 bases inside a longer seq1: column 1025 is the only valid column of wavefront 1; (L, off, len1, a, b)."""
    L, off, len1 = 1025, 200, 1500
    P = np.random.default_rng(9).integers(2, 4, L).astype(np.uint8)
    a, _ = background(len1, L)
    a[0, off:off + L] = P
    return L, off, len1, a, P[None, :].copy()


def one_long_gap_case():
    """seq2 = seq1 (300 random bases) without bases 100 .. 139; (a, b, matrix)."""
    x = np.random.default_rng(11).integers(0, 4, 300, dtype=np.uint8)
    y = np.concatenate([x[:100], x[140:]])
    return x[None], y[None], K23


def padding_case():
    """len2 = 1025, the last 20 bases of both sequences match; (L, len1, len2, a, b)."""
    L, len1, len2 = 20, 100, 1025
    P = np.random.default_rng(10).integers(2, 4, L).astype(np.uint8)
    a, b = background(len1, len2)
    a[0, len1 - L:] = P
    b[0, len2 - L:] = P
    return L, len1, len2, a, b


def end_cell_tie_case(len1, len2):
    """Homopolymer against homopolymer."""
    return np.full((1, len1), 2, np.uint8), np.full((1, len2), 2, np.uint8)


class GlobalHand:
    """One alignment under one mask with what it must give: score, ends = (end_i, end_j, start_i, start_j) and, where the path
    is pinned, its walking-order move codes (None: only the restatement decides the moves)."""

    def __init__(self, name, a, b, sm, gap_open, gap_extend, mask, score, ends, codes):
        self.name, self.sm, self.gap_open, self.gap_extend, self.mask = name, np.asarray(sm, np.int8), int(gap_open), int(gap_extend), int(mask)
        self.a, self.b = np.ascontiguousarray(a, np.uint8).reshape(1, -1), np.ascontiguousarray(b, np.uint8).reshape(1, -1)
        self.score, self.ends, self.codes = int(score), tuple(int(x) for x in ends), codes

    def __repr__(self):
        return "%s %dx%d open=%d extend=%d mask=%d" % (self.name, self.a.shape[1], self.b.shape[1], self.gap_open, self.gap_extend, self.mask)


def hand_groups():
    """{group: [GlobalHand]}: the inputs above with the fields that test_global_full_affine_gpu.py asserts of them."""
    L, off, len2, a, b = fit_case()
    fit = [GlobalHand("fit", a, b, K111, 3, 1, FIT, L, (L, off + L, 0, off), [DIAG] * L),
           GlobalHand("fit/mask0", a, b, K111, 3, 1, GLOBAL, L - (3 + off - 1) - (3 + len2 - off - L - 1), (L, len2, 0, 0),
                      [LEFT] * (len2 - off - L) + [DIAG] * L + [LEFT] * off),
           GlobalHand("fit/-127/begin2", a, b, K1_127, 3, 1, BEGIN2, -(3 + L - 1), (L, len2, 0, len2), [UP] * L),
           GlobalHand("fit/-127/end2", a, b, K1_127, 3, 1, END2, -(3 + L - 1), (L, 0, 0, 0), [UP] * L)]
    L, off, len1, a, b = column_fit_case()
    column_fit = [GlobalHand("column_fit/mask0", a, b, K111, 3, 1, GLOBAL, L - (3 + off - 1) - (3 + len1 - off - L - 1), (len1, L, 0, 0),
                             [UP] * (len1 - off - L) + [DIAG] * L + [UP] * off),
                  GlobalHand("column_fit/begin1|end1", a, b, K111, 3, 1, BEGIN1 | END1, L, (off + L, L, off, 0), [DIAG] * L)]
    a, b, sm = one_long_gap_case()
    gaps_and_padding = [GlobalHand("one_long_gap", a, b, sm, 10, 1, GLOBAL, 2 * 260 - (10 + 39), (300, 260, 0, 0), None)]
    L, len1, len2, a, b = padding_case()
    gaps_and_padding += [GlobalHand("pad/end2", a, b, K54, 0, 0, END2, 5 * L, (len1, len2, 0, 0), [DIAG] * L + [UP] * (len1 - L) + [LEFT] * (len2 - L)),
                         GlobalHand("pad/fit", a, b, K54, 0, 0, FIT, 5 * L, (len1, len2, 0, len2 - L), [DIAG] * L + [UP] * (len1 - L))]
    for len1, len2 in END_CELL_TIE_SHAPES:
        a, b = end_cell_tie_case(len1, len2)
        m = min(len1, len2)
        gaps_and_padding.append(GlobalHand("end_cell_ties/%d,%d" % (len1, len2), a, b, K111, 3, 1, OVERLAP, m, (m, m, 0, 0), [DIAG] * m))
    return {"fit": fit, "column_fit": column_fit, "gaps_and_padding": gaps_and_padding}
