"""Helpers of the affine exact semi-global tests (test_sgfull_affine_cpu.py, test_sgfull_affine_gpu.py): the C restatement
tests/native/sgfull_affine_oracle.c compiled into a temporary directory, an independent numpy/Python formulation of the same
semantics, the hand-checked inputs and the slice arithmetic."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT, match_matrix
from sgfull_support import move_words


class SgAffineOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libsgfull_affine_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "sgfull_affine_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend, traceback=True):
        """(scores, ends[n, 2], moves[n, move_words], lengths) for n pairs of one (len1, len2)."""
        a = np.ascontiguousarray(seq1s, np.uint8)
        b = np.ascontiguousarray(seq2s, np.uint8)
        m = np.ascontiguousarray(sm, np.int8)
        n, len1 = a.shape
        len2 = b.shape[1]
        mw = move_words(len1, len2)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 2), np.int32)
        moves = np.zeros((n, mw), np.uint64) if traceback else None
        lengths = np.zeros(n, np.uint32) if traceback else None
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731
        rc = self.lib.sgfull_affine_oracle_batch(P(a), ctypes.c_size_t(len1), P(b), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                                 P(m), int(gap_open), int(gap_extend), P(scores), P(ends), P(moves),
                                                 ctypes.c_size_t(mw), P(lengths))
        assert rc == 0
        return scores, ends, moves, lengths


def gotoh_numpy(seq1, seq2, sm, gap_open, gap_extend):
    """One alignment, formulated independently of the C restatement: whole rows of E and of the diagonal term at once in
    numpy, F by a running scan along the row, the best cell as numpy's first maximum, then the walk as 'D' / 'U' / 'L'
    letters.  Returns (score, (i, j), letters)."""
    a = np.asarray(seq1, np.int64) & 3
    b = np.asarray(seq2, np.int64) & 3
    s = np.asarray(sm, np.int64).reshape(4, 4)
    n1, n2 = len(a), len(b)
    neg = -(1 << 40)
    H = np.zeros((n1 + 1, n2 + 1), np.int64)
    E = np.full((n1 + 1, n2 + 1), neg, np.int64)
    F = np.full((n1 + 1, n2 + 1), neg, np.int64)
    H[0, 1:] = -(gap_open + np.arange(n2) * gap_extend)
    H[1:, 0] = -(gap_open + np.arange(n1) * gap_extend)
    for i in range(1, n1 + 1):
        E[i, 1:] = np.maximum(H[i - 1, 1:] - gap_open, E[i - 1, 1:] - gap_extend)
        part = np.maximum(H[i - 1, :-1] + s[a[i - 1], b], E[i, 1:])
        f = neg
        for j in range(1, n2 + 1):
            f = max(H[i, j - 1] - gap_open, f - gap_extend)
            F[i, j] = f
            H[i, j] = max(part[j - 1], f)
    pos = int(np.argmax(H.reshape(-1)))                # the first maximum in row-major order; (0,0) holds 0
    bi, bj = divmod(pos, n2 + 1)
    i, j, state, out = bi, bj, "H", []
    while i > 0 and j > 0:
        if state == "H":
            if H[i, j] == H[i - 1, j - 1] + s[a[i - 1], b[j - 1]]:
                out.append("D")
                i, j = i - 1, j - 1
                continue
            state = "E" if H[i, j] == E[i, j] else "F"
        if state == "E":
            out.append("U")
            state = "H" if E[i, j] == H[i - 1, j] - gap_open else "E"
            i -= 1
        else:
            out.append("L")
            state = "H" if F[i, j] == H[i, j - 1] - gap_open else "F"
            j -= 1
    out += ["U"] * i + ["L"] * j
    return int(H[bi, bj]), (bi, bj), out


def hand_cases():
    """(name, seq1s[1, len1], seq2s[1, len2], sm, open, extend, score, best cell, the one gap run)."""
    rng = np.random.default_rng(2024)
    x = rng.integers(0, 4, 400, dtype=np.uint8)
    deleted = np.concatenate([x[:150], x[250:]])                                  # seq2 lacks 100 bases of seq1
    inserted = np.concatenate([x[:150], rng.integers(0, 4, 100, dtype=np.uint8), x[150:]])   # seq2 holds 100 more
    sm = match_matrix(2, -3)
    return [("deletion100", x[None], deleted[None], sm, 10, 1, 2 * 300 - (10 + 99), (400, 300), ("U", 100)),
            ("insertion100", x[None], inserted[None], sm, 10, 1, 2 * 400 - (10 + 99), (400, 500), ("L", 100))]


def code_qwords(len1, len2):
    """qwords of codes one alignment of the kernel takes: ceil(len2 / 1024) waves x the padded sweep's trips x 256."""
    return -(-len2 // 1024) * (-(-(len1 + 63) // 32) * 8) * 256


def per_alignment(len1, len2, traceback):
    """device bytes one alignment of a slice takes (inputs, score, best cell; codes, moves and length with a traceback)"""
    per = len1 + len2 + 4 + 8
    if traceback:
        per += 8 * code_qwords(len1, len2) + 8 * move_words(len1, len2) + 4
    return per
