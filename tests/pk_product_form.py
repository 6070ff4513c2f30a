"""The PRODUCT FORM of the packed scorer's flag form (sw_kernels.hip "PRODUCT FORM", csrc/pk_form.h): the host
rule restated, parameter sets on both sides of each of its conditions, and a numpy model of the cell on 16-bit patterns with
the multiply modulo 2^16.  Importable without a device; test_pk_product_form_cpu.py and test_gpu_pk_product_form.py use it.

The form: for plain match / mismatch scoring -- an entry is enabled exactly when row base = column base -- the flag form's
lookup and diagonal add are one 16-bit multiply-add per half,  t = a[row base] * b[column base] + H(i-1,j-1)  modulo 2^16:
H + 255 where the bases agree, a finite negative half-precision pattern (which v_pk_maximum3_f16 drops) where they differ."""
from collections import namedtuple

import numpy as np

import pk_flag_form as pf
from conftest import match_matrix

PK_LIMIT = pf.PK_LIMIT
K = 255                     # the rescaled folded score of an enabled cell, the flag form's


def product_rule(sm, gap, bound):
    """True when the product form applies: the flag form applies, the entries above -2 gap are exactly the four diagonal ones,
    and the largest rescaled H, 255 * 128 m / (m + gap), is at most `bound` (what the committed constants are verified for)"""
    scale = pf.flag_rule(sm, gap)
    if not scale:
        return False
    sm = np.asarray(sm, np.int64).reshape(4, 4)
    if not np.array_equal(sm > -2 * int(gap), np.eye(4, dtype=bool)):
        return False
    m = int(sm[0, 0])
    return 255 * 128 * m <= bound * scale[0]


RuleSet = namedtuple("RuleSet", "label sm gap form product")       # form: what swmi_pk_cell_form reports; product: claimed by hand

RULE_SETS = [
    RuleSet("headline 10/-30 gap 15: largest rescaled H 13 056", match_matrix(10, -30), 15, "flag", True),
    RuleSet("2/-6 gap 3: the same ratios on small scores", match_matrix(2, -6), 3, "flag", True),
    RuleSet("-10/-30 gap 15: m < 0, every score 0", match_matrix(-10, -30), 15, "flag", True),
    RuleSet("asymmetric 10/-30 gap 15: two enabled entries off the diagonal", pf.matrix_of(pf.ASYMMETRIC, 10, -30), 15, "flag", False),
    RuleSet("10/-30 gap 15 without entry (3, 3): a diagonal entry disabled", pf.matrix_of(pf.DIAGONAL[:3], 10, -30), 15, "flag", False),
    RuleSet("16/-2 gap 1: largest rescaled H 30 720", match_matrix(16, -2), 1, "flag", False),
    RuleSet("36/-30 gap 15: largest rescaled H 23 040", match_matrix(36, -30), 15, "flag", False),
    RuleSet("10/-29 gap 15: two enabled values", match_matrix(10, -29), 15, "vert", False),
    RuleSet("10/-40 gap 15: s < -2 gap, the bias kernel", match_matrix(10, -40), 15, "bias", False),
    RuleSet("10/-30 gap 30: every s + gap >= 0", match_matrix(10, -30), 30, "q0", False),
]

# what the GPU test runs: two eligible sets; then the ineligible neighbours, which keep their cells
GPU_ELIGIBLE = [RULE_SETS[0], RULE_SETS[1]]
GPU_NEIGHBOURS = [RULE_SETS[3], RULE_SETS[5], RULE_SETS[7], RULE_SETS[8]]


def product_model(a, b, gap, unit, scaled_gap, row_mul, col_mul):
    """The product cell for a batch, every value a 16-bit pattern as the kernel holds it (one anti-diagonal at a time):
        t = (a[row base] * b[column base] + H(i-1,j-1)) mod 65536          v_pk_mad_i16, one half
        x = max3(H(i,j-1), H(i-1,j), t) by the half-precision order: a pattern with the sign bit set loses
        H = x -sat scaled_gap;  best = max x;  score = max(best - scaled_gap, 0) * unit / 255
    Returns (scores, H[129, 129, n] rescaled, dict of the extreme patterns held)."""
    a, b = np.asarray(a) & 3, np.asarray(b) & 3
    row_mul, col_mul = np.asarray(row_mul, np.int64), np.asarray(col_mul, np.int64)
    prod = (row_mul[a.T[:, None, :]] * col_mul[b.T[None, :, :]]) & 0xFFFF          # [i-1, j-1, pair]
    n = len(a)
    H = np.zeros((129, 129, n), np.int64)
    best = np.zeros(n, np.int64)
    seen = dict(max_enabled=0, min_enabled=0xFFFF, max_negative_magnitude=0, min_negative_magnitude=0xFFFF, wraps=0, max_x=0, max_h=0)
    for d in range(2, 257):
        i = np.arange(max(1, d - 128), min(128, d - 1) + 1)
        j = d - i
        t = prod[i - 1, j - 1] + H[i - 1, j - 1]
        seen["wraps"] += int((t > 0xFFFF).sum())
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
        seen["max_h"] = max(seen["max_h"], int(H[i, j].max()))
    rescaled = np.maximum(best - scaled_gap, 0) * unit
    assert not (rescaled % 255).any(), "the best value is not a multiple of 255 / (m + gap)"
    return rescaled // 255, H, seen
