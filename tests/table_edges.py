"""Inputs that reach the edges of the two table aligners' mappings, the predicates that say which edge an alignment reaches,
and a whole-table numpy formulation of both aligners to select ties with.  Shared by test_table_edges_cpu.py (every claimed
edge checked through the C restatements, no device), test_table_edges_gpu.py (every field bit-exact on the GPU) and
fuzz_parity.py.

    swmi_local_align*       csrc/local_kernels.hip,  DESIGN.md section 12: 16 lanes x 8 columns per alignment, 4 alignments
                            per wavefront, 16 per workgroup, len1 + 15 steps in trips of 8
    swmi_semiglobal_full*   csrc/sgfull_kernels.hip, DESIGN.md section 13: W = ceil(len2 / 1024) wavefronts of 64 lanes x 16
                            columns, chunks of 32 steps, wave w three chunks behind wave w - 1, an LDS ring of 256 rows per
                            wave boundary, a walk staged in blocks of 128 rows x 1024 columns

The grids are derived from the kernels' constants, read from the sources (kernel_constants), so a change of a constant
moves the grid with it.  Every generator is deterministic: the CPU coverage test and the GPU test see the same inputs."""
import os
import re

import numpy as np

from conftest import ROOT, match_matrix
from local_support import random_matrix
from sgfull_support import K111

CSRC = os.path.join(ROOT, "smith-waterman-simd_amd", "csrc")
WAVE = 64                                    # lanes of a gfx950 wavefront


def kernel_constants(source, env=None):
    """{name: value} of the `constexpr int kName = ...;` lines of a kernel source (integer expressions of earlier ones), those of
    the csrc headers it includes first, as the compiler reads them (a name the source defines again takes its value)."""
    env = {} if env is None else env
    with open(os.path.join(CSRC, source)) as fh:
        for include, name, expr in re.findall(r'#include "([^"]+)"|constexpr int (k\w+) = ([^;]+);', fh.read()):
            if include:
                if os.path.basename(include) == include and os.path.exists(os.path.join(CSRC, include)):
                    kernel_constants(include, env)
                continue
            cast = expr.startswith("(int)")                 # a 32-bit pattern written in hex: wrap it as the compiler does
            v = int(eval(expr[5:] if cast else expr, {"__builtins__": {}}, dict(env)))
            env[name] = (v + (1 << 31)) % (1 << 32) - (1 << 31) if cast else v
    return env


SG = kernel_constants("sgfull_kernels.hip")
LOC = kernel_constants("local_kernels.hip")
SG_WAVE_COLS = WAVE * SG["kCols"]                          # 1024 columns per wavefront
SG_MAX_LEN = SG_WAVE_COLS * SG["kMaxWaves"]                # 16384
SG_STAGE_ROWS = SG["kStageRows"]                           # 128
SG_STAGE_COLS = SG["kStageLanes"] * SG["kCols"]            # 1024
LOC_SEQ2 = LOC["kLanes"] * LOC["kCols"]                    # 128
LOC_MAX_LEN = 16384


def _around(x, lo=1, hi=SG_MAX_LEN):
    return [v for v in (x - 1, x, x + 1) if lo <= v <= hi]


def sg_waves(len2):
    return -(-len2 // SG_WAVE_COLS)


# ---- shape grids ---------------------------------------------------------------------------------------------------------

# len1 at the edges of the trip (kUnroll steps), the chunk (kChunk steps: local_chunks = ceil((len1 + 63) / kChunk) steps
# up at len1 = 32 m + 1), the 64-lane pipeline of a wave (lane 63 is 63 rows behind lane 0), the staging block
# (kStageRows), the ring (kRing), 16 rings, and the longest sequence
def sg_len1_grid(sg):
    return sorted({1, 2, 3} | set(_around(sg["kUnroll"])) | set(range(sg["kChunk"] - 1, sg["kChunk"] + 3)) | set(_around(WAVE))
                  | set(_around(sg["kStageRows"])) | set(_around(sg["kRing"])) | set(_around(16 * sg["kRing"]))
                  | {SG_MAX_LEN - 1, SG_MAX_LEN})


SG_LEN1 = sg_len1_grid(SG)
# W whose len2 take every edge of the wave: W * 1024 (no pad column in the last wave), W * 1024 - 1, (W - 1) * 1024 + 1
# (one valid column in the last wave) and a value = 15 (mod 16) (every lane of the last one but the last column valid);
# every other W takes one of them
SG_FULL_W = (1, 2, 4, 6, 11, SG["kMaxWaves"])


def _len2_edges(W, sg=SG):
    wave_cols = WAVE * sg["kCols"]
    return [wave_cols * W, wave_cols * W - 1, wave_cols * (W - 1) + 1,
            wave_cols * (W - 1) + sg["kCols"] * ((37 * W) % WAVE) + sg["kCols"] - 1]


def sg_len2_grid(sg, full_w=SG_FULL_W):
    return sorted({v for W in range(1, sg["kMaxWaves"] + 1)
                   for v in (_len2_edges(W, sg) if W in full_w else [_len2_edges(W, sg)[W % 4]])})


SG_LEN2 = sg_len2_grid(SG)


def sg_shape_grid(len1s=None, len2s=None):
    """[(len1, len2, n)]: a covering of SG_LEN1 x SG_LEN2 (or of the two lists given: the same grid derived from another
    kernel's constants), every value of both at least once, the longest len2 with the
    shortest len1 and the other way round, then a second pass rotated by a third that keeps shapes under 2^25 cells; n so
    that a shape holds about 2^24 cells (one or two alignments at 16384 rows or columns)."""
    l1, l2 = SG_LEN1 if len1s is None else len1s, (SG_LEN2 if len2s is None else len2s)[::-1]
    shapes = [(l1[k % len(l1)], l2[k % len(l2)]) for k in range(max(len(l1), len(l2)))]
    rot = len(l1) // 3
    shapes += [(l1[(k + rot) % len(l1)], l2[k]) for k in range(len(l2)) if l1[(k + rot) % len(l1)] * l2[k] <= 1 << 25]
    out = []
    for len1, len2 in dict.fromkeys(shapes):
        cells = len1 * len2
        out.append((len1, len2, 1 if cells >= 1 << 27 else 2 if cells >= 1 << 23 else min(16, max(2, (1 << 24) // cells))))
    return out


SG_PARAMS = [("(1,-1,1)", K111, 1), ("(5,-4,0)", match_matrix(5, -4), 0), ("random/4", random_matrix(3), 4)]

# len1 where n_steps = len1 + kLanes - 1 sits at the edges of a trip of kUnroll steps (and of a step pair of codes), and
# around 128, 256, 1024 and the longest sequence; n at the edges of kAlnPerWave and kAlnPerBlock alignments
def local_len1_grid(loc):
    trip = [v for v in range(1, 3 * loc["kUnroll"]) if (v + loc["kLanes"] - 1) % loc["kUnroll"] in (0, 1, loc["kUnroll"] - 1)]
    return sorted(set(trip) | {v for x in (128, 256, 1024, LOC_MAX_LEN) for v in _around(x, hi=LOC_MAX_LEN)})


def local_n_grid(loc):
    return sorted({1} | set(_around(loc["kAlnPerWave"])) | set(_around(loc["kAlnPerBlock"])) | set(_around(WAVE)) | {3})


LOC_LEN1 = local_len1_grid(LOC)
LOC_N = local_n_grid(LOC)


def local_shape_grid(len1s=None, ns=None):
    """[(len1, n)]: every len1 of LOC_LEN1 (or of the list given) with two n of LOC_N (every n at least once)."""
    len1s, ns = LOC_LEN1 if len1s is None else len1s, LOC_N if ns is None else ns
    return [(len1, ns[(2 * k + d) % len(ns)]) for k, len1 in enumerate(len1s) for d in (0, 1)]


LOCAL_PARAMS = [("(10,-30,15)", match_matrix(10, -30), 15), ("(5,-4,0)", match_matrix(5, -4), 0), ("(1,-1,1)", match_matrix(1, -1), 1),
                ("random/6", random_matrix(), 6)]


# ---- generators ----------------------------------------------------------------------------------------------------------

def _noisy(rng, x, p):
    return np.where(rng.random(len(x)) < p, rng.integers(0, 4, len(x)), x).astype(np.uint8)


def _pad(rows, length, rng):
    out = rng.integers(0, 4, (len(rows), length), dtype=np.uint8)
    for k, r in enumerate(rows):
        out[k, : len(r)] = r
    return out


def sg_mixed_pairs(n, len1, len2, seed):
    """random pairs; every other seq2 a noisy copy of its seq1 with a deletion of 1..40 (long diagonal paths), every fourth
    pair a homopolymer (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 2):
        src = _noisy(rng, a[k, :w], 0.08)
        if w > 8:
            cut, d = int(rng.integers(1, w - 1)), int(rng.integers(1, min(40, w - 2) + 1))
            src = np.concatenate([src[:cut], src[cut + d:], rng.integers(0, 4, d, dtype=np.uint8)])[:w]
        b[k, :w] = src
    for k in range(1, n, 4):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b


def local_mixed_pairs(n, len1, seed):
    """random pairs; every other seq1 carries a noisy copy of its seq2 somewhere (long paths), every fourth pair a
    homopolymer (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, LOC_SEQ2), dtype=np.uint8)
    w = min(len1, LOC_SEQ2)
    for k in range(0, n, 2):
        at = int(rng.integers(0, len1 - w + 1))
        a[k, at:at + w] = _noisy(rng, b[k, LOC_SEQ2 - w:], 0.15)
    for k in range(1, n, 4):
        a[k] = k & 3
        b[k, rng.random(LOC_SEQ2) < 0.8] = k & 3
    return a, b


class Case:
    """One batch of one shape for one aligner and parameter set, and the edges its generator claims for it: {predicate
    name: the least number of its alignments that must meet it}."""

    def __init__(self, name, a, b, sm, gap, claims):
        self.name, self.a, self.b, self.sm, self.gap, self.claims = name, a, b, np.asarray(sm, np.int8), int(gap), claims

    @property
    def shape(self):
        return self.a.shape[1], self.b.shape[1]

    def __repr__(self):
        return "%s %dx%d n=%d gap=%d sm=%s" % (self.name, self.a.shape[1], self.b.shape[1], len(self.a), self.gap, self.sm.tolist())


def _lo(rng, n):
    """n bases of {0, 1}: the matched stretches"""
    return rng.integers(0, 2, n, dtype=np.uint8)


def _hi(rng, n):
    """n bases of {2, 3}: gap contents and tails that match no base of a stretch"""
    return rng.integers(2, 4, n, dtype=np.uint8)


def _noisy_lo(rng, x, p):
    return np.where(rng.random(len(x)) < p, _lo(rng, len(x)), x).astype(np.uint8)


def sg_gap_run_cases():
    """Long interior gap runs: seq2 = X + R + Y against seq1 = X + Y (and the other way round), X and Y of {0, 1}, R of
    {2, 3} so that no base of R matches (a linear gap would otherwise dissolve into single gaps between chance matches), |Y|
    long enough that the detour pays.  A left run of more than 1024 columns crosses a wave boundary and leaves staging
    blocks through their left edge at an interior row; an up run of more than 128 rows spans staging blocks top to bottom."""
    cases = []
    rng = np.random.default_rng(1100)
    for r, n in ((1100, 4), (1500, 4), (2100, 3), (3000, 3)):                    # insertions in seq2: left runs
        rows1, rows2 = [], []
        for _ in range(n):
            x, y = int(rng.integers(200, 1400)), int(1.3 * r) + int(rng.integers(300, 700))
            X, Y = _lo(rng, x), _lo(rng, y)
            rows1.append(np.concatenate([X, Y]))
            rows2.append(np.concatenate([_noisy_lo(rng, X, 0.03), _hi(rng, r), _noisy_lo(rng, Y, 0.03)]))
        len1 = max(map(len, rows1))
        cases.append(Case("insertion%d" % r, _pad(rows1, len1, rng), _pad(rows2, len1 + r, rng), K111, 1,
                          {"left_run_1100_across_waves": n, "block_exit_left": n}))
    for r, n in ((129, 4), (300, 4), (700, 3), (1300, 2)):                      # deletions from seq2: up runs
        rows1, rows2 = [], []
        for _ in range(n):
            x, y = int(rng.integers(100, 1500)), int(1.3 * r) + int(rng.integers(300, 700))
            X, Y = _lo(rng, x), _lo(rng, y)
            rows1.append(np.concatenate([X, _hi(rng, r), Y]))
            rows2.append(np.concatenate([_noisy_lo(rng, X, 0.03), _noisy_lo(rng, Y, 0.03)]))
        len2 = max(map(len, rows2))
        cases.append(Case("deletion%d" % r, _pad(rows1, len2 + r, rng), _pad(rows2, len2, rng), match_matrix(2, -3), 2,
                          {"up_run_over_128": n}))
    return cases


def sg_staircase_cases():
    """Several gaps of 100..200 bases, in seq1 and seq2 in turn, between matching stretches of 300..600: the walk turns
    corners and leaves staging blocks through the top, the left edge and the corner."""
    cases = []
    rng = np.random.default_rng(2200)
    for steps, n in ((6, 6), (10, 4), (14, 2)):
        rows1, rows2 = [], []
        for _ in range(n):
            s1, s2 = [], []
            for t in range(steps):
                m = _lo(rng, int(rng.integers(300, 601)))
                s1.append(m)
                s2.append(_noisy_lo(rng, m, 0.02))
                (s1 if t % 2 else s2).append(_hi(rng, int(rng.integers(100, 201))))
            rows1.append(np.concatenate(s1))
            rows2.append(np.concatenate(s2))
        cases.append(Case("staircase%d" % steps, _pad(rows1, max(map(len, rows1)) + 8, rng), _pad(rows2, max(map(len, rows2)) + 8, rng),
                          K111, 1, {"staircase": n, "block_exit_top": n, "block_across_waves": n}))
    return cases


def sg_corner_cases():
    """A walk that leaves a staging block through its corner: the best cell (x + 127, x + L + 127) in the bottom-right
    corner, 127 diagonal moves back to row x, the block's top row, then a left run of L to column x, the block's first
    column (x = 1 mod 16, L in 881..896 so that x = 16 g_lo + 1), then a diagonal move out of both edges at once."""
    cases = []
    rng = np.random.default_rng(2300)
    for x, L in ((17, 896), (33, 881), (1025, 890), (2049, 885)):
        X, Y = _lo(rng, x), _lo(rng, SG_STAGE_ROWS - 1)
        a = np.concatenate([X, Y])[None]
        b = np.concatenate([X, _hi(rng, L), Y])[None]
        cases.append(Case("corner/x=%d/L=%d" % (x, L), a, b, match_matrix(10, -10), 1, {"block_exit_corner": 1}))
    return cases


def sg_wave_edge_end_cases():
    """The best cell at j = 1024 k (the last column of wave k - 1) and 1024 k + 1 (the first of wave k): seq1 = a prefix of
    seq2 (of {0, 1}) of that length, then bases of {2, 3} that match nothing."""
    cases = []
    rng = np.random.default_rng(3300)
    for kw in (1, 2, 3, 5):
        for J in (SG_WAVE_COLS * kw, SG_WAVE_COLS * kw + 1):
            B = _lo(rng, J + 200)
            a = np.stack([np.concatenate([B[:J], _hi(rng, 150)]), np.concatenate([_noisy_lo(rng, B[:J], 0.02), _hi(rng, 150)])])
            cases.append(Case("end_j%d" % J, a, np.stack([B, B]), match_matrix(2, -3), 2, {"end_at_wave_edge": 2}))
    return cases


def _lcs_tie(z, c0, len2, tail):
    """A pair whose table under (match 1, mismatch <= 0, gap 0) -- the LCS of the prefixes -- holds its maximum z first at
    (z, c0) and again at (z + 1, z) and further right on that row:
        seq2 = 0^z 1^(c0 - 1 - z) 2 1^(len2 - c0),  seq1 = 0^(z - 1) 2 0 3^tail
    row z reaches z only through the 2 at column c0; row z + 1 reaches it at column z through its last 0."""
    b = np.ones(len2, np.uint8)
    b[:z] = 0
    b[c0 - 1] = 2
    a = np.concatenate([np.zeros(z - 1, np.uint8), [2, 0], np.full(tail, 3, np.uint8)]).astype(np.uint8)
    return a, b


TIE_MATRICES = [("match(1,0)", match_matrix(1, 0)), ("match(1,-1)", match_matrix(1, -1)),
                ("pm1", np.array([1, 0, -1, 0, -1, 1, 0, -1, 0, -1, 1, 0, 1, 0, -1, 1], np.int8))]


def sg_tie_cases(per_claim=4):
    """Ties of the maximum H that only the reduction order decides.  Constructed (_lcs_tie, gap 0): the row-major-first
    occurrence in the first lane of wave k and a later-row occurrence in wave k - 1; the first occurrence in a later lane of
    one wave than a later-row occurrence; both in one lane.  Selected from random pairs of small alphabets, matrices in
    {-1, 0, 1} and gap 0 or 1 by the whole-table numpy formulation: the maximum in two lanes of one wave."""
    cases = []
    rng = np.random.default_rng(4400)
    for name, sm in TIE_MATRICES[:2]:
        for len2, tail in ((1100, 7), (2100, 40), (3073, 1)):
            pairs, used = [], 0
            for k in range(1, sg_waves(len2)):
                lanes = min(WAVE, (len2 - SG_WAVE_COLS * k - SG["kCols"]) // SG["kCols"])   # lanes of wave k inside len2
                if lanes < 3:
                    continue
                used += 1
                c0 = SG_WAVE_COLS * k + 1                                                   # first column of wave k
                pairs += [_lcs_tie(int(z), c0, len2, tail) for z in (c0 - 1, c0 - 1 - int(rng.integers(1, 300)))]
                c0 = SG_WAVE_COLS * k + SG["kCols"] * int(rng.integers(2, lanes)) + 1       # first column of a later lane
                pairs += [_lcs_tie(c0 - 1 - int(rng.integers(1, 16)), c0, len2, tail)]
                c0 = SG_WAVE_COLS * k + SG["kCols"] * int(rng.integers(0, lanes)) + 9       # inside one lane
                pairs += [_lcs_tie(c0 - int(rng.integers(2, 9)), c0, len2, tail)]
            len1 = max(len(p[0]) for p in pairs)
            a = np.stack([np.concatenate([p[0], np.full(len1 - len(p[0]), 3, np.uint8)]) for p in pairs])
            cases.append(Case("ties/lcs/%s/len2=%d" % (name, len2), a, np.stack([p[1] for p in pairs]), sm, 0,
                              {"tie_two_waves": len(pairs) // 2, "first_in_later_wave": 2 * used, "first_in_later_lane": used,
                               "same_lane_later_row": len(pairs)}))
    want = ("tie_two_lanes_one_wave",)
    for t, (len1, len2) in enumerate(((300, 1100), (500, 1500))):
        name, sm = TIE_MATRICES[t + 1]
        gap = t
        chosen, got = [], dict.fromkeys(want, 0)
        for _ in range(40):
            a = rng.integers(0, 2, (16, len1), dtype=np.uint8)
            b = rng.integers(0, 2, (16, len2), dtype=np.uint8)
            for k in range(len(a)):
                facts = sg_tie_facts(sgfull_table(a[k], b[k], sm, gap))
                if any(facts[c] and got[c] < per_claim for c in want):
                    chosen.append((a[k], b[k]))
                    for c in want:
                        got[c] += bool(facts[c])
            if all(v >= per_claim for v in got.values()):
                break
        cases.append(Case("ties/random/%s/%d" % (name, gap), np.stack([c[0] for c in chosen]), np.stack([c[1] for c in chosen]), sm, gap,
                          {c: per_claim for c in want}))
    return cases


def sg_pad_cases():
    """gap = 0, len2 % 16 != 0 and the best cell in column len2: the pad column len2 + 1 of the same lane (score -128, no
    mask) holds exactly the best value, and only the column-ascending tie-break keeps it from being picked."""
    cases = []
    rng = np.random.default_rng(5500)
    for len2 in (17, 1000, 1025, 2047, 3001):
        assert len2 % SG["kCols"]
        rows1, rows2 = [], []
        for k in range(6):
            B = rng.integers(0, 4, len2, dtype=np.uint8)
            rows1.append(np.concatenate([B if k % 2 == 0 else _noisy(rng, B, 0.01 * k), rng.integers(0, 4, 40, dtype=np.uint8)]))
            rows2.append(B)
        for sm_name, sm in (("match(1,-1)", match_matrix(1, -1)), ("match(5,-4)", match_matrix(5, -4))):
            cases.append(Case("pad/%s/len2=%d" % (sm_name, len2), np.stack(rows1), np.stack(rows2), sm, 0, {"end_at_len2_gap0": 3}))
    return cases


def local_insertion_cases():
    """seq1 (of {2, 3}) carries the 128-mer (of {0, 1}) with an insertion of more than 128 bases of {2, 3} in it: an up run
    of more than 128 rows inside the path."""
    cases = []
    rng = np.random.default_rng(6600)
    for r, len1, gap in ((129, 700, 3), (200, 700, 3), (400, 1000, 1), (700, 1500, 1)):
        a = rng.integers(2, 4, (6, len1), dtype=np.uint8)
        b = rng.integers(0, 2, (6, LOC_SEQ2), dtype=np.uint8)
        for k in range(6):
            cut = int(rng.integers(50, 79))
            ins = np.concatenate([_noisy_lo(rng, b[k, :cut], 0.02), _hi(rng, r), _noisy_lo(rng, b[k, cut:], 0.02)])
            at = int(rng.integers(0, len1 - len(ins) + 1))
            a[k, at:at + len(ins)] = ins
        cases.append(Case("local_insertion%d" % r, a, b, match_matrix(20, -20), gap, {"up_run_over_128": 6}))
    return cases


def local_tie_cases(per_claim=4):
    """Ties of the maximum H over the 16 lanes x 8 columns.  Constructed (_lcs_tie, gap 0): the first occurrence in the
    first column of a lane, a later-row occurrence in an earlier lane; the first occurrence in a lane, a later-row
    occurrence in an earlier column of the same lane; and both with a later-row occurrence in the same column.  Selected
    from random pairs of small alphabets by the whole-table numpy formulation: the maximum in two lanes."""
    cases = []
    rng = np.random.default_rng(7700)
    cols = LOC["kCols"]
    for name, sm in TIE_MATRICES[:2]:
        pairs = []
        for lane in range(1, LOC["kLanes"]):
            c0 = cols * lane + 1
            pairs.append(_lcs_tie(c0 - 1 - int(rng.integers(0, min(c0 - 1, 40))), c0, LOC_SEQ2, int(rng.integers(1, 30))))
            c0 = cols * lane + int(rng.integers(3, cols + 1))
            pairs.append(_lcs_tie(c0 - int(rng.integers(1, c0 - cols * lane)), c0, LOC_SEQ2, int(rng.integers(1, 30))))
        len1 = max(len(p[0]) for p in pairs)
        a = np.stack([np.concatenate([p[0], np.full(len1 - len(p[0]), 3, np.uint8)]) for p in pairs])
        cases.append(Case("local_ties/lcs/%s" % name, a, np.stack([p[1] for p in pairs]), sm, 0,
                          {"tie_two_lanes": len(pairs) // 2, "first_in_later_lane": LOC["kLanes"] - 1,
                           "same_lane_earlier_col_later_row": LOC["kLanes"] - 1, "same_column_later_row": len(pairs)}))
    want = ("tie_two_lanes", "same_column_later_row")
    for t, len1 in enumerate((129, 300)):
        name, sm = TIE_MATRICES[t + 1]
        gap = t
        chosen, got = [], dict.fromkeys(want, 0)
        for _ in range(40):
            a = rng.integers(0, 2, (64, len1), dtype=np.uint8)
            b = rng.integers(0, 2, (64, LOC_SEQ2), dtype=np.uint8)
            for k in range(len(a)):
                facts = local_tie_facts(local_table(a[k], b[k], sm, gap))
                if any(facts[c] and got[c] < per_claim for c in want):
                    chosen.append((a[k], b[k]))
                    for c in want:
                        got[c] += bool(facts[c])
            if all(v >= per_claim for v in got.values()):
                break
        cases.append(Case("local_ties/random/%s/%d" % (name, gap), np.stack([c[0] for c in chosen]), np.stack([c[1] for c in chosen]),
                          sm, gap, {c: per_claim for c in want}))
    return cases


def _pair_kinds(n, len1, len2, seed):
    """identical (as far as the shorter goes), shifted by 5 and random pairs, in turn"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    for k in range(n):
        w = min(len1, len2)
        if k % 3 == 0:
            b[k, :w] = a[k, :w]
        elif k % 3 == 1:
            b[k, 5:w] = a[k, : w - 5]
    return a, b


EXTREME_SM = [("all+127/0", np.full(16, 127, np.int8), 0), ("all-128/127", np.full(16, -128, np.int8), 127),
              ("diag+127,off-128/127", np.where(np.eye(4, dtype=bool), 127, -128).astype(np.int8).reshape(16), 127)]


def sg_extreme_cases():
    """16384 x 16384 at the bounds of H: every score +127 with gap 0 (H up to 127 * 16384), every score -128 with gap 127
    (H down to -128 * 16384), and +127 / -128 with gap 127, on an identical, a shifted and a random pair."""
    a, b = _pair_kinds(3, SG_MAX_LEN, SG_MAX_LEN, 8800)
    return [Case("extreme/" + name, a, b, sm, gap, {}) for name, sm, gap in EXTREME_SM]


def local_extreme_cases():
    """len1 = 16384 at the bounds of the key: every score +127 with gap 0 (score 127 * 128 = 16256, the most the key holds,
    the end cell decided by a tie over rows), every score -128 with gap 127 (score 0) and an asymmetric matrix."""
    a, b = _pair_kinds(6, LOC_MAX_LEN, LOC_SEQ2, 9900)
    asym = random_matrix(21)
    asym[2], asym[8] = 127, -128
    return [Case("local_extreme/" + name, a, b, sm, gap, {}) for name, sm, gap in EXTREME_SM[:2] + [("asymmetric/2", asym, 2)]]


# ---- whole tables in numpy -----------------------------------------------------------------------------------------------

def _score_rows(a, b, sm):
    return np.asarray(sm, np.int64).reshape(4, 4)[np.asarray(a) & 3][:, np.asarray(b) & 3]


def sgfull_table(a, b, sm, gap):
    """H of the exact semi-global aligner, (len1 + 1) x (len2 + 1) int64, a row at a time: the left term unrolls to
    H(i,j) = max over k <= j of T(i,k) - (j - k) gap, T the diagonal / up terms, a running maximum of T(i,k) + k gap."""
    S = _score_rows(a, b, sm)
    len1, len2 = S.shape
    jg = np.arange(len2 + 1, dtype=np.int64) * gap
    H = np.empty((len1 + 1, len2 + 1), np.int64)
    H[0] = -jg
    T = np.empty(len2 + 1, np.int64)
    for i in range(1, len1 + 1):
        T[0] = -i * gap
        np.maximum(H[i - 1, :-1] + S[i - 1], H[i - 1, 1:] - gap, out=T[1:])
        H[i] = np.maximum.accumulate(T + jg) - jg
    return H


def local_table(a, b, sm, gap):
    """H of the local aligner, (len1 + 1) x 129 int64 (the same running maximum, with the zero floor)."""
    S = _score_rows(a, b, sm)
    len1, len2 = S.shape
    jg = np.arange(len2 + 1, dtype=np.int64) * gap
    H = np.zeros((len1 + 1, len2 + 1), np.int64)
    T = np.zeros(len2 + 1, np.int64)
    for i in range(1, len1 + 1):
        np.maximum(np.maximum(H[i - 1, :-1] + S[i - 1], H[i - 1, 1:] - gap), 0, out=T[1:])
        H[i] = np.maximum.accumulate(T + jg) - jg
    return H


def best_cell(H):
    """(score, i, j): the first cell in row-major order strictly above every earlier one, from 0 at (0,0)"""
    pos = int(np.argmax(H))
    if H.flat[pos] <= 0:
        return 0, 0, 0
    return int(H.flat[pos]), pos // H.shape[1], pos % H.shape[1]


def numpy_local(a, b, sm, gap):
    """The local aligner from its whole table (the counterpart of sgfull_support.numpy_sgfull): (score, (end_i, end_j),
    (start_i, start_j), path start -> end)."""
    H = local_table(a, b, sm, gap)
    S = _score_rows(a, b, sm)
    score, i, j = best_cell(H)
    end = (i, j)
    path = [end]
    while i > 0 and j > 0 and H[i, j] != 0:
        if H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
            i, j = i - 1, j - 1
        elif H[i, j] == H[i - 1, j] - gap:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return score, end, (i, j), np.array(path[::-1], np.int32).reshape(-1, 2)


# ---- predicates ----------------------------------------------------------------------------------------------------------

def _max_cells(H):
    score, i0, j0 = best_cell(H)
    if score <= 0:
        return None
    cells = np.argwhere(H == score)
    return (i0, j0), cells[:, 0], cells[:, 1]


def sg_tie_facts(H):
    """Which ties of the maximum the sgfull reductions meet in this table (lane G = (j - 1) // 16, wave = G // 64)."""
    out = dict.fromkeys(("tie_two_waves", "first_in_later_wave", "tie_two_lanes_one_wave", "first_in_later_lane",
                         "same_lane_later_row"), False)
    m = _max_cells(H)
    if m is None:
        return out
    (i0, j0), ii, jj = m
    G = (jj - 1) // SG["kCols"]
    w = G // WAVE
    G0 = (j0 - 1) // SG["kCols"]
    w0 = G0 // WAVE
    later = ii > i0
    out["tie_two_waves"] = len(np.unique(w)) >= 2
    out["first_in_later_wave"] = bool(np.any(later & (w < w0)))
    out["tie_two_lanes_one_wave"] = any(len(np.unique(G[w == x])) >= 2 for x in np.unique(w))
    out["first_in_later_lane"] = bool(np.any(later & (w == w0) & (G < G0)))
    out["same_lane_later_row"] = bool(np.any(later & (G == G0)))
    return out


def local_tie_facts(H):
    """Which ties of the maximum the local kernel's reductions meet (lane = (j - 1) // 8 of 16)."""
    out = dict.fromkeys(("tie_two_lanes", "first_in_later_lane", "same_lane_earlier_col_later_row", "same_column_later_row"), False)
    m = _max_cells(H)
    if m is None:
        return out
    (i0, j0), ii, jj = m
    lane, lane0 = (jj - 1) // LOC["kCols"], (j0 - 1) // LOC["kCols"]
    later = ii > i0
    out["tie_two_lanes"] = len(np.unique(lane)) >= 2
    out["first_in_later_lane"] = bool(np.any(later & (lane < lane0)))
    out["same_lane_earlier_col_later_row"] = bool(np.any(later & (lane == lane0) & (jj < j0)))
    out["same_column_later_row"] = bool(np.any(later & (jj == j0)))
    return out


def walk_cells(row, count, end_i, end_j):
    """(codes, i, j) of a walk: codes[t] the move taken at step t (walking order, 3 / 2 / 1 = diagonal / up / left) and
    (i[t], j[t]) the cell it was taken from; (i[count], j[count]) the cell the walk ends on."""
    words = np.asarray(row, np.uint64)[: (count + 31) // 32]
    c = ((words[:, None] >> (2 * np.arange(32, dtype=np.uint64))) & np.uint64(3)).reshape(-1)[:count].astype(np.int64)
    i = end_i - np.concatenate([[0], np.cumsum(c != 1)])
    j = end_j - np.concatenate([[0], np.cumsum(c != 2)])
    return c, i, j


def gap_runs(c, i, j):
    """[(code, length, i, j)] of the walk's runs of up (2) or left (1) moves, (i, j) the cell the run starts from"""
    if len(c) == 0:
        return []
    edges = np.flatnonzero(np.diff(c)) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [len(c)]])
    return [(int(c[s]), int(e - s), int(i[s]), int(j[s])) for s, e in zip(starts, ends) if c[s] in (1, 2)]


def staging_exits(i, j, stage_rows=SG_STAGE_ROWS, stage_lanes=SG["kStageLanes"], steps=False):
    """How the sgfull walk leaves each staging block it loads (stage_rows rows x stage_lanes lanes ending at its cell; the
    linear kernel's by default): [(exit, block spans two waves)], exit 'top', 'left' or 'corner' (both at one diagonal
    move), or 'border' (row or column 0 reached inside the block).  steps=True: [(exit, spans, t)], move t - 1 the one
    that left the block and cell t the first outside it."""
    out = []
    t, n = 0, len(i) - 1
    while i[t] > 0 and j[t] > 0:
        g1 = (j[t] - 1) // SG["kCols"]
        i_lo = max(i[t] - stage_rows + 1, 1)
        g_lo = max(g1 - stage_lanes + 1, 0)
        rest_i, rest_j = i[t:], j[t:]
        top = rest_i < i_lo
        left = (rest_j - 1) // SG["kCols"] < g_lo
        border = (rest_i == 0) | (rest_j == 0)
        out_at = np.flatnonzero(top | left | border)
        if len(out_at) == 0:
            break
        s = int(out_at[0])
        kind = "border" if border[s] and not (top[s] and i_lo > 1) and not (left[s] and rest_j[s] > 0) else \
            "corner" if top[s] and left[s] else "top" if top[s] else "left"
        t += s
        out.append((kind, g_lo // WAVE != g1 // WAVE) + ((t,) if steps else ()))
        if t >= n:
            break
    return out


def sg_path_facts(score, ends, moves, length, stage_rows=SG_STAGE_ROWS, stage_lanes=SG["kStageLanes"]):
    """The walk-shape predicates of one sgfull alignment (oracle or GPU result), for a staging block of stage_rows x
    stage_lanes (the linear kernel's by default)."""
    c, i, j = walk_cells(moves, int(length) - 1, int(ends[0]), int(ends[1]))
    return sg_walk_facts(score, c, i, j, stage_rows, stage_lanes)


def sg_walk_facts(score, c, i, j, stage_rows=SG_STAGE_ROWS, stage_lanes=SG["kStageLanes"]):
    """sg_path_facts of a walk given as walk_cells returns it"""
    end_j = int(j[0])
    runs = gap_runs(c, i, j)
    left = [(L, ri, rj) for code, L, ri, rj in runs if code == 1 and ri > 0]
    up = [(L, ri, rj) for code, L, ri, rj in runs if code == 2 and rj > 0]
    exits = staging_exits(i, j, stage_rows, stage_lanes)
    crosses = lambda L, rj: (rj - 1) // SG_WAVE_COLS > (rj - L - 1) // SG_WAVE_COLS  # noqa: E731  (columns rj - L .. rj)
    return {
        "left_run_1100_across_waves": any(L >= 1100 and rj - L >= 1 and crosses(L, rj) for L, ri, rj in left),
        "left_run_over_1024": any(L > stage_lanes * SG["kCols"] for L, _, _ in left),     # wider than a staging block
        "up_run_over_128": any(L > stage_rows for L, _, _ in up),
        "staircase": sum(100 <= L <= 250 for L, _, _ in left) >= 2 and sum(100 <= L <= 250 for L, _, _ in up) >= 2,
        "block_exit_top": any(e == "top" for e, _ in exits),
        "block_exit_left": any(e == "left" for e, _ in exits),
        "block_exit_corner": any(e == "corner" for e, _ in exits),
        "block_across_waves": any(x for _, x in exits),
        "end_at_wave_edge": score > 0 and end_j % SG_WAVE_COLS in (0, 1) and end_j > 1,
    }


def local_path_facts(score, ends, moves, steps):
    c, i, j = walk_cells(moves, int(steps), int(ends[0]), int(ends[1]))
    runs = gap_runs(c, i, j)
    return {"up_run_over_128": any(code == 2 and L > 128 for code, L, _, _ in runs)}


def sg_claim_counts(case, result):
    """{claim: number of alignments of the case that meet it} from an oracle (or GPU) result with traceback."""
    sc, ends, moves, lengths = result
    counts = dict.fromkeys(case.claims, 0)
    for k in range(len(sc)):
        facts = sg_path_facts(int(sc[k]), ends[k], moves[k], lengths[k])
        if "end_at_len2_gap0" in counts:
            facts["end_at_len2_gap0"] = case.gap == 0 and sc[k] > 0 and ends[k, 1] == case.b.shape[1] and case.b.shape[1] % SG["kCols"] != 0
        if any(c.startswith(("tie", "first_in", "same_")) for c in counts):
            facts.update(sg_tie_facts(sgfull_table(case.a[k], case.b[k], case.sm, case.gap)))
        for c in counts:
            counts[c] += bool(facts[c])
    return counts


def local_claim_counts(case, result):
    sc, ends, moves, steps = result
    counts = dict.fromkeys(case.claims, 0)
    for k in range(len(sc)):
        facts = local_path_facts(int(sc[k]), ends[k], moves[k], steps[k])
        if any(c != "up_run_over_128" for c in counts):
            facts.update(local_tie_facts(local_table(case.a[k], case.b[k], case.sm, case.gap)))
        for c in counts:
            counts[c] += bool(facts[c])
    return counts


# ---- comparisons ---------------------------------------------------------------------------------------------------------

def first_difference(got, want, count_offset, traceback=True):
    """None, or (field, alignment) of the first field that differs: scores, ends, then count and move words up to the
    last step, in that order, for the lowest alignment that differs."""
    sc, ends, mv, cnt = got
    wsc, wends, wmv, wcnt = want
    bad = []
    d = np.flatnonzero(sc != wsc)
    if len(d):
        bad.append((int(d[0]), "score"))
    d = np.flatnonzero((ends != wends).any(axis=1))
    if len(d):
        bad.append((int(d[0]), "ends"))
    if traceback:
        d = np.flatnonzero(cnt != wcnt)
        if len(d):
            bad.append((int(d[0]), "count"))
        for k in range(len(sc)):
            steps = int(wcnt[k]) - count_offset
            full, part = divmod(steps, 32)
            same = np.array_equal(mv[k, :full], wmv[k, :full])
            if same and part:
                mask = np.uint64((1 << (2 * part)) - 1)
                same = (mv[k, full] & mask) == (wmv[k, full] & mask)
            if not same:
                bad.append((k, "moves"))
                break
    if not bad:
        return None
    k, field = min(bad)
    return field, k


def assert_same(got, want, what, aligner, traceback=True):
    """every field bit-exact; the message names the case, the field and the first differing alignment"""
    diff = first_difference(got, want, 1 if aligner == "sgfull" else 0, traceback)
    if diff is not None:
        field, k = diff
        sc, ends = got[0], got[1]
        raise AssertionError("%s: %s of alignment %d differs: got score %d ends %s, want score %d ends %s" % (
            what, field, k, int(sc[k]), ends[k].tolist(), int(want[0][k]), want[1][k].tolist()))
