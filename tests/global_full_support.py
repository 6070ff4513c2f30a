"""Helpers of the global / free-end-gap aligner's tests (test_global_full_cpu.py, test_global_full_gpu.py,
test_table_host_fake.py): the C restatement tests/native/global_full_oracle.c, compiled into a temporary directory
(these semantics have no reference counterpart, so the restatement is their definition), an independent numpy formulation
for small shapes, and the checks every path has to pass whatever the tie rules."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from local_full_support import assert_same, move_words, moves_of, path_from  # noqa: F401  (the result layout is local_full's)

BEGIN1, BEGIN2, END1, END2 = 1, 2, 4, 8
GLOBAL, FIT, OVERLAP = 0, BEGIN2 | END2, 15
ALL_MASKS = tuple(range(16))


class GlobalFullOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libglobal_full_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "global_full_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap, free_ends, traceback=True):
        """(scores, ends[n, 4], moves[n, move_words], steps) for n pairs of one (len1, len2) under one mask."""
        a = np.ascontiguousarray(seq1s, np.uint8)
        b = np.ascontiguousarray(seq2s, np.uint8)
        m = np.ascontiguousarray(sm, np.int8)
        n, len1 = a.shape
        len2 = b.shape[1]
        mw = move_words(len1, len2)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros((n, mw), np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        rc = self.lib.global_full_oracle_batch(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                               b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                               m.ctypes.data_as(ctypes.c_void_p), int(gap), ctypes.c_uint(int(free_ends)),
                                               scores.ctypes.data_as(ctypes.c_void_p), ends.ctypes.data_as(ctypes.c_void_p),
                                               moves.ctypes.data_as(ctypes.c_void_p) if traceback else None, ctypes.c_size_t(mw),
                                               steps.ctypes.data_as(ctypes.c_void_p) if traceback else None)
        assert rc == 0
        return scores, ends, moves, steps


def numpy_table(a, b, sm, gap, free_ends):
    """(H, S): the whole table by anti-diagonals in numpy, and the score of every cell's pair of bases."""
    len1, len2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)[np.asarray(a) & 3][:, np.asarray(b) & 3]
    H = np.zeros((len1 + 1, len2 + 1), np.int64)
    if not free_ends & BEGIN1:
        H[:, 0] = -np.arange(len1 + 1) * gap
    if not free_ends & BEGIN2:
        H[0, :] = -np.arange(len2 + 1) * gap
    for d in range(2, len1 + len2 + 1):
        i = np.arange(max(1, d - len2), min(len1, d - 1) + 1)
        j = d - i
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + S[i - 1, j - 1], H[i - 1, j] - gap), H[i, j - 1] - gap)
    return H, S


def numpy_global_full(a, b, sm, gap, free_ends):
    """An independent formulation for small sizes: numpy_table, the end cell by a masked argmax over the whole table, then
    the walk on H itself.  (score, (end_i, end_j), path from the start cell to the end cell, H)."""
    len1, len2 = len(a), len(b)
    H, S = numpy_table(a, b, sm, gap, free_ends)
    allowed = np.zeros(H.shape, bool)
    allowed[len1, len2] = True
    if free_ends & END1:
        allowed[:, len2] = True
    if free_ends & END2:
        allowed[len1, :] = True
    masked = np.where(allowed, H, np.iinfo(np.int64).min)
    i, j = divmod(int(np.argmax(masked.reshape(-1))), len2 + 1)      # the first maximum in row-major order
    end = (i, j)
    path = [(i, j)]
    while i or j:
        if i == 0:
            if free_ends & BEGIN2:
                break
            j -= 1
        elif j == 0:
            if free_ends & BEGIN1:
                break
            i -= 1
        elif H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
            i, j = i - 1, j - 1
        elif H[i, j] == H[i - 1, j] - gap:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return int(H[end]), end, np.array(path[::-1], np.int32).reshape(-1, 2), H


def check_path(a, b, sm, gap, free_ends, score, ends, moves_row, steps):
    """What every path satisfies whatever the tie rules: it runs from the start cell it names to the end cell it names inside
    the matrix; the start lies at (0, 0), or on column 0 with BEGIN1, or on row 0 with BEGIN2; the end lies at (len1, len2),
    or in the last column with END1, or in the last row with END2; and its steps re-scored from the sequences give the score
    (a path that starts on a free border pays nothing for the border before it)."""
    len1, len2 = len(a), len(b)
    path = path_from(moves_row, steps, ends[0], ends[1])
    assert tuple(path[0]) == (int(ends[2]), int(ends[3])) and tuple(path[-1]) == (int(ends[0]), int(ends[1]))
    assert path.min() >= 0 and path[:, 0].max() <= len1 and path[:, 1].max() <= len2
    si, sj = (int(x) for x in path[0])
    assert (si, sj) == (0, 0) or (sj == 0 and free_ends & BEGIN1) or (si == 0 and free_ends & BEGIN2), (si, sj, free_ends)
    ei, ej = (int(x) for x in path[-1])
    assert (ei, ej) == (len1, len2) or (ej == len2 and free_ends & END1) or (ei == len1 and free_ends & END2), (ei, ej, free_ends)
    d = np.diff(path, axis=0)
    diag = (d[:, 0] == 1) & (d[:, 1] == 1)
    S = np.asarray(sm, np.int64).reshape(4, 4)
    i, j = path[1:, 0][diag], path[1:, 1][diag]
    total = int(S[np.asarray(a)[i - 1] & 3, np.asarray(b)[j - 1] & 3].sum()) - int(gap) * int((~diag).sum())
    assert total == int(score), (total, int(score))
    return path


def inputs(n, len1, len2, seed):
    """Random pairs; every third seq2 holds a 90 % copy of (a stretch of) its seq1 with a 5-base indel, placed at the END of
    seq2 (so that a global path runs through every wavefront and holds all three kinds of move), every seventh pair a
    homopolymer against a mostly equal one (ties), every sixth from the fifth a seq1 whose first base seq2 lacks."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, len1 - w:], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 8:
            cut = int(rng.integers(1, w - 1))
            src = np.concatenate([src[:cut], src[cut + min(5, w - cut - 1):], rng.integers(0, 4, min(5, w - cut - 1), dtype=np.uint8)])
        b[k, len2 - w:] = src[:w]
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    for k in range(4, n, 6):
        # seq1 = one base that nothing in seq2 equals, then the first bases of seq2: where a mismatch costs more than two gaps
        # that base is left unaligned (an up move), however few rows the table has.  (Where it costs less, and seq2 is the
        # longer one, no walk holds an up move: it needs one more left move, and a mismatch is cheaper than the two.)
        if len1 >= 3:
            a[k][a[k] == 3] = 0
            b[k][b[k] == 3] = 0
            a[k, 0] = 3
            w = min(len1 - 1, len2)
            b[k, :w] = a[k, 1:1 + w]
    return a, b
