"""Helpers of the banded local aligner's tests (test_banded_align_cpu.py, test_banded_align_gpu.py): the C restatement
tests/native/banded_align_oracle.c compiled into a temporary directory, the case generators, a numpy re-scoring of a path
that shares nothing with either, and the slice arithmetic of include/swmi_banded.h."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from local_full_support import assert_same, move_words, moves_of, path_from  # noqa: F401  (re-exported)

LO, HI = -64, 63
MAX_LEN = 16384
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# (match, mismatch, open, extend) of the issue's "related" family
RELATED_PARAMS = [(2, -3, 5, 1), (1, -1, 1, 1), (5, -4, 10, 1), (1, -1, 1, 3)]
RELATED_DIAGONALS = [0, 40, -37]
TB_BUDGET = 4096 * (16384 + 128 + 4 + 16 + 4 * 262400 + 8 * 516 + 4)      # swmi_local_affine_slices_for's, in bytes


class BandedOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libbanded_align_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "banded_align_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend, diagonals=None, traceback=True, lo=LO, hi=HI):
        """(scores, ends[n, 4], moves[n, move_words], steps) for n pairs of one (len1, len2)."""
        a = np.ascontiguousarray(seq1s, np.uint8)
        b = np.ascontiguousarray(seq2s, np.uint8)
        m = np.ascontiguousarray(sm, np.int8)
        n, len1 = a.shape
        len2 = b.shape[1]
        d = None if diagonals is None else np.ascontiguousarray(np.broadcast_to(np.asarray(diagonals, np.int64), (n,)), np.int32)
        mw = move_words(len1, len2)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros((n, mw), np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731
        rc = self.lib.banded_align_oracle_batch(P(a), ctypes.c_size_t(len1), P(b), ctypes.c_size_t(len2), ctypes.c_size_t(n), P(d),
                                                int(lo), int(hi), P(m), int(gap_open), int(gap_extend), P(scores), P(ends), P(moves),
                                                ctypes.c_size_t(mw), P(steps))
        assert rc == 0
        return scores, ends, moves, steps


def code_bytes(len1):
    """bytes of codes one alignment of a traceback launch takes: 256 per trip of four iterations, len1 + 63 iterations"""
    return 256 * (-(-(len1 + 63) // 4))


def per_alignment(len1, len2, traceback):
    """device bytes one alignment of a slice takes (inputs, diagonal, score, four ends; codes, moves and steps with a traceback)"""
    per = len1 + len2 + 4 + 4 + 16
    if traceback:
        per += code_bytes(len1) + 8 * move_words(len1, len2) + 4
    return per


def related_pairs(rng, n, len1, len2, d0=0, sub=0.08, runs=3, max_run=8):
    """seq1 random; seq2 = seq1 with `sub` substitutions and `runs` indel runs of 1 .. max_run bases, behind max(d0, 0) random
    bases (and with the first -d0 bases of seq1 cut off for d0 < 0), cut or filled with random bases to len2: the alignment
    lies along diagonal d0."""
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    for k in range(n):
        src = a[k, max(-d0, 0):].copy()
        flip = rng.random(len(src)) < sub
        src[flip] = rng.integers(0, 4, int(flip.sum()), dtype=np.uint8)
        parts, at = [], 0
        cuts = sorted(int(x) for x in rng.integers(1, max(2, len(src) - 1), runs)) if len(src) > 2 else []
        for c in cuts:
            g = int(rng.integers(1, max_run + 1))
            parts.append(src[at:c])
            if rng.random() < 0.5:
                parts.append(rng.integers(0, 4, g, dtype=np.uint8))      # an insertion in seq2
                at = c
            else:
                at = min(len(src), c + g)                                # a deletion
        parts.append(src[at:])
        out = np.concatenate([rng.integers(0, 4, max(d0, 0), dtype=np.uint8)] + parts)[:len2]
        b[k, :len(out)] = out
    return a, b


def in_band(path, d0=0, lo=LO, hi=HI):
    """every cell (i, j) of a path, its start cell on the border included, on a diagonal lo <= j - i - d0 <= hi"""
    p = np.asarray(path, np.int64)
    d = p[:, 1] - p[:, 0] - int(d0)
    return bool((d >= lo).all() and (d <= hi).all())


def rescore(a, b, sm, gap_open, gap_extend, path):
    """The score of a path (list of (i, j) from the start cell to the end cell), re-scored by numpy alone: diagonal steps by
    the matrix, every run of k up or k left moves at open + (k - 1) extend.  Exact for open >= extend (with open < extend the
    contract's walk may open at every step of a run, which the moves do not show)."""
    path = np.asarray(path, np.int64)
    d = np.diff(path, axis=0)
    kind = np.where((d[:, 0] == 1) & (d[:, 1] == 1), 3, np.where(d[:, 0] == 1, 2, 1))
    S = np.asarray(sm, np.int64).reshape(4, 4)
    diag = kind == 3
    i, j = path[1:, 0][diag], path[1:, 1][diag]
    total = int(S[np.asarray(a)[i - 1] & 3, np.asarray(b)[j - 1] & 3].sum())
    gaps = int((~diag).sum())
    opens = int(np.sum(~diag & (np.concatenate([[0], kind[:-1]]) != kind)))
    return total - opens * int(gap_open) - (gaps - opens) * int(gap_extend), gaps - opens


def check_path(a, b, sm, gap_open, gap_extend, d0, score, ends, moves_row, steps):
    """Path validity without any oracle: the expanded path re-scored gives the score, it starts where ends says, at a cell
    whose H is 0 (a border cell, or a cell the path's first move leaves with exactly that move's score: a positive H there
    would have continued the walk), and it stays in the band and in the table."""
    path = path_from(moves_row, steps, ends[0], ends[1])
    assert tuple(path[0]) == (int(ends[2]), int(ends[3])) and tuple(path[-1]) == (int(ends[0]), int(ends[1]))
    assert path.min() >= 0 and path[:, 0].max() <= len(a) and path[:, 1].max() <= len(b)
    if int(score) > 0:
        assert in_band(path[1:], d0), "the path leaves the band"
        # (the start cell may be a border cell next to the band: it is where H = 0 is read, not a cell of the alignment)
    total, extended = rescore(a, b, sm, gap_open, gap_extend, path)
    if gap_open >= gap_extend:
        assert total == int(score), (total, int(score))
    else:
        assert total <= int(score) <= total + extended * (int(gap_extend) - int(gap_open)), (total, int(score))
    # a prefix of the path never scores below 0 and the whole path is the maximum: H at the start cell is 0
    return path


def numpy_band_table(a, b, sm, gap_open, gap_extend, d0=0, lo=LO, hi=HI):
    """H of a small shape, (len1 + 1) x (len2 + 1) with 0 outside the band, by plain loops over int64 arrays: a formulation that
    shares no code with the C restatement."""
    len1, len2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)
    neg = -(1 << 40)
    H = np.zeros((len1 + 1, len2 + 1), np.int64)
    E = np.full((len1 + 1, len2 + 1), neg, np.int64)
    F = np.full((len1 + 1, len2 + 1), neg, np.int64)
    for i in range(1, len1 + 1):
        for j in range(max(1, i + d0 + lo), min(len2, i + d0 + hi) + 1):
            E[i, j] = max(H[i - 1, j] - gap_open, E[i - 1, j] - gap_extend)
            F[i, j] = max(H[i, j - 1] - gap_open, F[i, j - 1] - gap_extend)
            H[i, j] = max(0, H[i - 1, j - 1] + S[a[i - 1] & 3, b[j - 1] & 3], E[i, j], F[i, j])
    return H
