"""Helpers of the long banded aligners' tests (test_banded_long_cpu.py, test_banded_long_gpu.py): the two existing C restatements
through banded_width_support.WidthOracle, unchanged -- they take lo and hi and store only the band, 100 .. 400 MB at 65536 rows
of 128 or 256 diagonals -- the slice arithmetic of include/swmi_banded_long.h, which is the width header's, and the builders of
long inputs: an all-mismatch background with planted identical motifs, and related pairs whose indels lie where a test wants
them.  There is no restatement of the recurrences here."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from banded_width_support import (ALL_MASKS, EO_BUDGET, FORMS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_SLICE, NO_ALIGNMENT,  # noqa: F401
                                  SLOT_BYTES, TB_BUDGET, WIDTHS, Batch, WidthOracle, assert_same, code_bytes, move_words, moves_of,
                                  path_from, per_alignment, related_batch, related_pairs, slices_by_hand)

MAX_LEN = 65536
MOTIF = 40


def planted(len1, len2, ends, motif=MOTIF, distinct=False):
    """seq1 all 0 and seq2 all 1 -- no cell of the background matches -- with one identical `motif`-mer of letters 2 / 3 per
    (i, j) of `ends`, ending at cell (i, j): the same word everywhere, or with `distinct` all 2 for the first end and all 3 for
    the second, so that no motif matches a base of the other.  Under a matrix that pays only for a match the best local paths
    are the motifs."""
    a, b = np.zeros(len1, np.uint8), np.ones(len2, np.uint8)
    word = (2 + np.random.default_rng(40).integers(0, 2, motif)).astype(np.uint8)
    assert not distinct or len(ends) == 2
    for k, (i, j) in enumerate(ends):
        assert motif <= i <= len1 and motif <= j <= len2
        a[i - motif:i] = 2 + k if distinct else word
        b[j - motif:j] = 2 + k if distinct else word
    return a, b


def drifting_pair(rng, length, first, runs, run, insert, sub=0.03):
    """seq1 of `length` bases and seq2 = seq1 with `sub` substitutions and `runs` runs of `run` bases inserted (insert) or
    deleted, the first at base `first`, the others 150 bases behind the one before: the path drifts by runs * run diagonals behind row `first`."""
    a = rng.integers(0, 4, length, dtype=np.uint8)
    b = np.where(rng.random(length) < sub, rng.integers(0, 4, length, dtype=np.uint8), a).astype(np.uint8)
    pieces, at = [], 0
    for k in range(runs):
        cut = first + (run + 150) * k
        pieces.append(b[at:cut])
        if insert:
            pieces.append(rng.integers(0, 4, run, dtype=np.uint8))
            at = cut
        else:
            at = cut + run
    pieces.append(b[at:])
    return a, np.concatenate(pieces)


def align_each(orc, kind, batch, band, sm, gap_open, gap_extend, free_ends=0, workers=4):
    """orc.align(...) of `batch`, its alignments restated on `workers` threads at once (the restatements run outside the
    interpreter's lock; the global one fills 24 bytes a band cell of len1 + 1 rows, 1.6 GB at 65536 x 1024, before it starts)."""
    ones = [Batch([batch.seq1s[k]], [batch.seq2s[k]], None if batch.diagonals is None else batch.diagonals[k:k + 1]) for k in range(batch.n)]
    with ThreadPoolExecutor(workers) as pool:
        parts = list(pool.map(lambda one: orc.align(kind, one, band, sm, gap_open, gap_extend, free_ends), ones))
    moves = np.zeros(int(batch.move_offsets[-1]), np.uint64)
    for k, part in enumerate(parts):
        moves[int(batch.move_offsets[k]):int(batch.move_offsets[k + 1])] = part[2]
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), moves, np.concatenate([p[3] for p in parts]))
