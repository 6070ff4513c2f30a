"""Helpers of the long global / fit / overlap aligners' tests (test_global_long_gpu.py, test_global_long_affine_gpu.py,
test_global_long_cpu.py): the shapes at the kernels' stripe edges (a stripe is 16384 columns: 16 wavefronts of 1024), planted
pairs whose paths cross a stripe boundary, and the parameter sets.  The definitions stay the two C restatements
tests/native/global_full_oracle.c and global_full_affine_oracle.c, which take any lengths."""
import numpy as np

from conftest import match_matrix
from global_full_support import BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP
from local_support import random_matrix

STRIPE = 16384
MAX_LEN = 65536
LEN2S = (16385, 16399, 16400, 17408, 17409, 32767, 32768, 32769, 49153, 65536)
LEN1S = (1, 3, 33, 64, 129, 257)
MASKS = (GLOBAL, FIT, OVERLAP, BEGIN1, BEGIN2, END1, END2)
# (matrix, gap): the unit costs, the usual 5 / -4, the int8 extremes (127 * (257 + 65536) < 2^23: inside the domain rule), an
# asymmetric matrix, and gap 0 (every tie there is)
LINEAR_PARAMS = ((match_matrix(1, -1), 1), (match_matrix(5, -4), 3), (match_matrix(127, -127), 127), (random_matrix(), 7),
                 (match_matrix(2, -3), 0))
# (matrix, open, extend): open > extend, open < extend, the extremes, an asymmetric matrix, extend 0
AFFINE_PARAMS = ((match_matrix(1, -1), 3, 1), (match_matrix(5, -4), 2, 6), (match_matrix(127, -127), 127, 127),
                 (random_matrix(), 11, 2), (match_matrix(2, -3), 4, 0))


def noisy_copy(src, rng):
    """src with 10 % mismatches and 5 % indels (half deletions, half insertions)."""
    out = []
    for x in src:
        u = rng.random()
        if u < 0.025:
            continue
        if u < 0.05:
            out.append(int(rng.integers(0, 4)))
        out.append(int(rng.integers(0, 4)) if rng.random() < 0.10 else int(x))
    return np.array(out, np.uint8)


def plant(b_row, copy, centre):
    """Writes `copy` into b_row so that it straddles column `centre` (clipped into the row)."""
    at = max(0, min(len(b_row) - len(copy), centre - len(copy) // 2))
    w = min(len(copy), len(b_row) - at)
    b_row[at:at + w] = copy[:w]


def planted_batch(len1, len2, seed):
    """Four pairs of one shape: seq2 0 holds a noisy copy of seq1 0 across column 16384, seq2 1 one across column 32768 where
    len2 reaches it (else across 16384, shifted), seq2 2 one at its very end, and pair 3 is random."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (4, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (4, len2), dtype=np.uint8)
    plant(b[0], noisy_copy(a[0], rng), STRIPE)
    plant(b[1], noisy_copy(a[1], rng), 2 * STRIPE if len2 > 2 * STRIPE else STRIPE + 1)
    plant(b[2], noisy_copy(a[2], rng), len2)
    return a, b


def crosses(ends, column):
    """Per alignment: whether the path from (start_i, start_j) to (end_i, end_j) holds a cell left of and at most `column` and
    one right of it."""
    ends = np.asarray(ends)
    return (ends[:, 3] <= column) & (ends[:, 1] > column)
