"""Helpers of the any-length affine local aligner's tests (test_local_full_affine_cpu.py, test_local_full_affine_gpu.py): the
C restatement tests/native/local_full_affine_oracle.c, compiled into a temporary directory, an independent numpy / Python
formulation of Gotoh's recurrences with the zero floor that also yields the walk's states, the checks every path has to pass
whatever the tie rules, input builders and the slice arithmetic."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from local_full_support import assert_same, move_words, moves_of, path_from  # noqa: F401  (re-exported)


class LocalFullAffineOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "liblocal_full_affine_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "local_full_affine_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend, traceback=True):
        """(scores, ends[n, 4], moves[n, move_words], steps) for n pairs of one (len1, len2)."""
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
        rc = self.lib.local_full_affine_oracle_batch(P(a), ctypes.c_size_t(len1), P(b), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                                     P(m), int(gap_open), int(gap_extend), P(scores), P(ends), P(moves),
                                                     ctypes.c_size_t(mw), P(steps))
        assert rc == 0
        return scores, ends, moves, steps


def gotoh_numpy(seq1, seq2, sm, gap_open, gap_extend):
    """One alignment, formulated independently of the C restatement: whole rows of E and of the diagonal term at once in
    numpy, F by a running scan along the row, the end cell as numpy's first maximum, then the walk.
    Returns (score, (end_i, end_j, start_i, start_j), letters 'D' / 'U' / 'L' in walking order, the state 'H' / 'E' / 'F' each
    move was made in, H)."""
    a = np.asarray(seq1, np.int64) & 3
    b = np.asarray(seq2, np.int64) & 3
    s = np.asarray(sm, np.int64).reshape(4, 4)
    n1, n2 = len(a), len(b)
    neg = -(1 << 40)
    H = np.zeros((n1 + 1, n2 + 1), np.int64)
    E = np.full((n1 + 1, n2 + 1), neg, np.int64)
    F = np.full((n1 + 1, n2 + 1), neg, np.int64)
    for i in range(1, n1 + 1):
        E[i, 1:] = np.maximum(H[i - 1, 1:] - gap_open, E[i - 1, 1:] - gap_extend)
        part = np.maximum(np.maximum(H[i - 1, :-1] + s[a[i - 1], b], E[i, 1:]), 0)
        f = neg
        for j in range(1, n2 + 1):
            f = max(H[i, j - 1] - gap_open, f - gap_extend)
            F[i, j] = f
            H[i, j] = max(part[j - 1], f)
    pos = int(np.argmax(H.reshape(-1)))                # the first maximum in row-major order; (0,0) holds 0
    ei, ej = divmod(pos, n2 + 1)
    i, j, state, out, states = ei, ej, "H", [], []
    while i > 0 and j > 0:
        if state == "H":
            if H[i, j] == 0:
                break
            if H[i, j] == H[i - 1, j - 1] + s[a[i - 1], b[j - 1]]:
                out.append("D")
                states.append("H")
                i, j = i - 1, j - 1
                continue
            state = "E" if H[i, j] == E[i, j] else "F"
        states.append(state)
        if state == "E":
            out.append("U")
            state = "H" if E[i, j] == H[i - 1, j] - gap_open else "E"
            i -= 1
        else:
            out.append("L")
            state = "H" if F[i, j] == H[i, j - 1] - gap_open else "F"
            j -= 1
    return int(H[ei, ej]), (ei, ej, i, j), out, states, H


def moves_as_letters(moves_row, steps):
    """Walking-order moves -> 'D' / 'U' / 'L' letters."""
    return ["?LUD"[c] for c in moves_of(moves_row, steps)]


def check_path(a, b, sm, gap_open, gap_extend, score, ends, moves_row, steps):
    """What every affine local path satisfies whatever the tie rules: its moves re-scored from the sequences, every run of
    k up or k left moves at open + (k - 1) extend, give the score; it starts at its start cell and never leaves the matrix."""
    path = path_from(moves_row, steps, ends[0], ends[1])
    assert tuple(path[0]) == (int(ends[2]), int(ends[3])) and tuple(path[-1]) == (int(ends[0]), int(ends[1]))
    assert path.min() >= 0 and path[:, 0].max() <= len(a) and path[:, 1].max() <= len(b)
    d = np.diff(path, axis=0)
    kind = np.where((d[:, 0] == 1) & (d[:, 1] == 1), 3, np.where(d[:, 0] == 1, 2, 1))      # in path order
    S = np.asarray(sm, np.int64).reshape(4, 4)
    diag = kind == 3
    i, j = path[1:, 0][diag], path[1:, 1][diag]
    total = int(S[np.asarray(a)[i - 1] & 3, np.asarray(b)[j - 1] & 3].sum())
    gaps = int((~diag).sum())
    opens = int(np.sum(~diag & (np.concatenate([[0], kind[:-1]]) != kind)))                 # first move of every gap run
    total -= opens * int(gap_open) + (gaps - opens) * int(gap_extend)
    # with open < extend a run of k may be cheaper as k runs of one: the contract's walk can then open at every step, which
    # the moves alone do not show -- so the re-scored total is a lower bound there and exact otherwise
    if gap_open >= gap_extend:
        assert total == int(score), (total, int(score))
    else:
        assert total <= int(score) <= total + (gaps - opens) * (int(gap_extend) - int(gap_open)), (total, int(score))
    return path


def inputs(n, len1, len2, seed):
    """Random pairs; every third seq2 a 90 % copy of its seq1 with a deletion of 1..40 bases and an insertion of 1..40 (long
    paths through F and E runs), every seventh pair a homopolymer (ties)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 100:
            c1, c2 = sorted(int(x) for x in rng.integers(1, w - 1, 2))
            d1, d2 = (int(x) for x in rng.integers(1, 41, 2))
            src = np.concatenate([src[:c1], src[c1 + d1:c2], rng.integers(0, 4, d2, dtype=np.uint8), src[c2:],
                                  rng.integers(0, 4, d1, dtype=np.uint8)])[:w]
        b[k, :w] = src
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b


def code_qwords(len1, len2):
    """qwords of codes one alignment of the kernel takes: ceil(len2 / 1024) waves x the padded sweep's trips x 256."""
    return -(-len2 // 1024) * (-(-(len1 + 63) // 32) * 8) * 256


def per_alignment(len1, len2, traceback):
    """device bytes one alignment of a slice takes (inputs, score, four ends; codes, moves and steps with a traceback)"""
    per = len1 + len2 + 4 + 16
    if traceback:
        per += 8 * code_qwords(len1, len2) + 8 * move_words(len1, len2) + 4
    return per
