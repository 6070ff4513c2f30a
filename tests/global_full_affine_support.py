"""Helpers of the affine global / free-end-gap aligner's tests (test_global_full_affine_cpu.py, test_global_full_affine_gpu.py):
the C restatement tests/native/global_full_affine_oracle.c, compiled into a temporary directory (these semantics have no
reference counterpart, so the restatement is their definition), an independent numpy/Python three-matrix formulation for
small shapes, the checks every path has to pass whatever the tie rules, and the related pairs of the prefix identity."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from global_full_support import ALL_MASKS, BEGIN1, BEGIN2, END1, END2, FIT, GLOBAL, OVERLAP  # noqa: F401
from local_full_support import assert_same, move_words, moves_of, path_from  # noqa: F401  (the result layout is local_full's)

DIAG, UP, LEFT = 3, 2, 1


class GlobalFullAffineOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libglobal_full_affine_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "global_full_affine_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend, free_ends, traceback=True):
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
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731
        rc = self.lib.global_full_affine_oracle_batch(P(a), ctypes.c_size_t(len1), P(b), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                                      P(m), int(gap_open), int(gap_extend), ctypes.c_uint(int(free_ends)), P(scores),
                                                      P(ends), P(moves), ctypes.c_size_t(mw), P(steps))
        assert rc == 0
        return scores, ends, moves, steps


def gotoh_tables(a, b, sm, gap_open, gap_extend, free_ends):
    """(H, E, F, S): three whole matrices, E by rows in numpy, F by a running scan, -inf as a value far below every score."""
    a = np.asarray(a, np.int64) & 3
    b = np.asarray(b, np.int64) & 3
    n1, n2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)[a][:, b]
    neg = -(1 << 40)
    H = np.zeros((n1 + 1, n2 + 1), np.int64)
    E = np.full((n1 + 1, n2 + 1), neg, np.int64)
    F = np.full((n1 + 1, n2 + 1), neg, np.int64)
    if not free_ends & BEGIN2:
        H[0, 1:] = -(gap_open + np.arange(n2) * gap_extend)
    if not free_ends & BEGIN1:
        H[1:, 0] = -(gap_open + np.arange(n1) * gap_extend)
    for i in range(1, n1 + 1):
        E[i, 1:] = np.maximum(H[i - 1, 1:] - gap_open, E[i - 1, 1:] - gap_extend)
        part = np.maximum(H[i - 1, :-1] + S[i - 1], E[i, 1:])
        f = neg
        for j in range(1, n2 + 1):
            f = max(H[i, j - 1] - gap_open, f - gap_extend)
            F[i, j] = f
            H[i, j] = max(part[j - 1], f)
    return H, E, F, S


def numpy_global_full_affine(a, b, sm, gap_open, gap_extend, free_ends):
    """An independent formulation for small sizes: gotoh_tables, the end cell by a masked argmax over the whole of H, then
    the three-state walk on the tables themselves.  (score, (end_i, end_j), path from the start cell to the end cell, H)."""
    n1, n2 = len(a), len(b)
    H, E, F, S = gotoh_tables(a, b, sm, gap_open, gap_extend, free_ends)
    allowed = np.zeros(H.shape, bool)
    allowed[n1, n2] = True
    if free_ends & END1:
        allowed[:, n2] = True
    if free_ends & END2:
        allowed[n1, :] = True
    masked = np.where(allowed, H, np.iinfo(np.int64).min)
    i, j = divmod(int(np.argmax(masked.reshape(-1))), n2 + 1)        # the first maximum in row-major order
    end = (i, j)
    path, state = [(i, j)], "H"
    while i or j:
        if i == 0:
            assert state == "H"
            if free_ends & BEGIN2:
                break
            j -= 1
        elif j == 0:
            assert state == "H"
            if free_ends & BEGIN1:
                break
            i -= 1
        else:
            if state == "H" and H[i, j] != H[i - 1, j - 1] + S[i - 1, j - 1]:
                state = "E" if H[i, j] == E[i, j] else "F"
            if state == "H":
                i, j = i - 1, j - 1
            elif state == "E":
                state = "H" if E[i, j] == H[i - 1, j] - gap_open else "E"
                i -= 1
            else:
                state = "H" if F[i, j] == H[i, j - 1] - gap_open else "F"
                j -= 1
        path.append((i, j))
    return int(H[end]), end, np.array(path[::-1], np.int32).reshape(-1, 2), H


def gap_runs(codes):
    """[(code, run length)] of consecutive equal move codes, in the order given."""
    out = []
    for c in (int(x) for x in codes):
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(c, k) for c, k in out]


def check_path(a, b, sm, gap_open, gap_extend, free_ends, score, ends, moves_row, steps):
    """global_full_support.check_path with gap runs re-scored as open + (k-1) extend: the path runs from the start cell it
    names to the end cell it names inside the matrix; the start lies at (0, 0), or on column 0 with BEGIN1, or on row 0 with
    BEGIN2; the end lies at (len1, len2), or in the last column with END1, or in the last row with END2; and its diagonal
    steps re-scored from the sequences, less the cost of every maximal run of k up moves and of k left moves, give the score.
    A run of k costs open + (k-1) extend as one gap.  Where open < extend the recurrences make k gaps of one base out of it
    instead (E reopens from an H that E itself holds), which cost k open; any split into m gaps costs m open + (k-m) extend,
    the score is the optimum, so the run's cost is open + (k-1) min(open, extend) whatever the tie rules.  A run along a
    border that is not free is forced and costs what the border's closed form says, open + (k-1) extend."""
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
    total = int(S[np.asarray(a)[i - 1] & 3, np.asarray(b)[j - 1] & 3].sum())
    kinds = np.where(diag, DIAG, np.where(d[:, 0] == 1, UP, LEFT))
    at = 0
    for code, k in gap_runs(kinds):
        if code != DIAG:
            on_border = path[at, 0] == 0 if code == LEFT else path[at, 1] == 0     # forced moves: the border's own closed form
            total -= int(gap_open) + (k - 1) * (int(gap_extend) if on_border else min(int(gap_open), int(gap_extend)))
        at += k
    assert total == int(score), (total, int(score))
    return path


def related_pairs(n, len1, len2, seed):
    """Random pairs as the affine exact semi-global aligner's GPU tests draw them: every third seq2 a noisy copy of its seq1
    with an indel of up to 40 bases (long E / F runs), every seventh pair a homopolymer (ties)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 8:
            cut = int(rng.integers(1, w - 1))
            d = int(rng.integers(1, min(40, w - cut - 1) + 1)) if w - cut > 2 else 1
            src = np.concatenate([src[:cut], src[cut + d:], rng.integers(0, 4, d, dtype=np.uint8)]) if k % 2 else \
                np.concatenate([src[:cut], rng.integers(0, 4, d, dtype=np.uint8), src[cut:]])
        b[k, :w] = src[:w]
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b
