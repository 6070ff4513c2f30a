"""Helpers of the affine local-aligner tests (test_local_affine_cpu.py, test_local_affine_gpu.py): the C restatement
tests/native/local_affine_oracle.c compiled into a temporary directory, an independent numpy/Python formulation of the same
semantics, and the three hand-checked inputs."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT, match_matrix
from local_support import move_words

# (gap_open, gap_extend) pairs every parameter-set test crosses its matrices with
AFFINE_GAPS = [(0, 0), (0, 5), (5, 0), (11, 1), (3, 7), (127, 127), (127, 0)]


class AffineOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "liblocal_affine_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "local_affine_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend):
        """(scores, ends[n, 4], moves[n, move_words], steps) for n pairs of one seq1 length."""
        a = np.ascontiguousarray(seq1s, np.uint8)
        b = np.ascontiguousarray(seq2s, np.uint8)
        m = np.ascontiguousarray(sm, np.int8)
        n, len1 = a.shape
        mw = move_words(len1)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros((n, mw), np.uint64)
        steps = np.zeros(n, np.uint32)
        rc = self.lib.local_affine_oracle_batch(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                                b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n),
                                                m.ctypes.data_as(ctypes.c_void_p), int(gap_open), int(gap_extend),
                                                scores.ctypes.data_as(ctypes.c_void_p), ends.ctypes.data_as(ctypes.c_void_p),
                                                moves.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(mw),
                                                steps.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        return scores, ends, moves, steps


def gotoh_numpy(seq1, seq2, sm, gap_open, gap_extend):
    """One alignment, formulated independently of the C oracle: whole rows of E and of the diagonal candidate at once in
    numpy, F by a running scan along the row, then a walk that returns its moves as a list of 'D' / 'U' / 'L'.
    Returns (score, (end_i, end_j, start_i, start_j), moves)."""
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
        diag = H[i - 1, :-1] + s[a[i - 1], b]
        part = np.maximum(np.maximum(diag, E[i, 1:]), 0)      # H without F; F needs the row's own H to its left
        f = neg
        for j in range(1, n2 + 1):
            f = max(H[i, j - 1] - gap_open, f - gap_extend)
            F[i, j] = f
            H[i, j] = max(part[j - 1], f)
    score = int(H.max())
    if score == 0:
        ei, ej = 0, 0
    else:
        flat = int(np.argmax(H.reshape(-1) == score))          # first in row-major order
        ei, ej = divmod(flat, n2 + 1)
    i, j, state, out = ei, ej, "H", []
    while i > 0 and j > 0:
        if state == "H":
            if H[i, j] == 0:
                break
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
    return score, (ei, ej, i, j), out


def moves_as_letters(moves_row, steps):
    """Walking-order moves -> 'D' / 'U' / 'L' letters."""
    return ["?LUD"[(int(moves_row[t // 32]) >> (2 * (t % 32))) & 3] for t in range(int(steps))]


def runs(letters):
    """[(letter, length)] of consecutive equal moves."""
    out = []
    for c in letters:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [tuple(r) for r in out]


def hand_cases():
    """The three hand-checked inputs: (name, seq1s[1, len1], seq2s[1, 128], sm, open, extend, score)."""
    rng = np.random.default_rng(1234)
    seq2 = rng.integers(0, 4, 128, dtype=np.uint8)
    deleted = np.concatenate([seq2[:59], seq2[69:]])                                  # 10 bases of seq2 missing from seq1
    spliced = np.concatenate([seq2[0:14], seq2[114:128]])                             # 100 bases missing, across lanes
    inserted = np.concatenate([seq2[:64], rng.integers(0, 4, 3000, dtype=np.uint8), seq2[64:]])   # 3000 extra rows
    return [("deletion10", deleted[None], seq2[None], match_matrix(2, -3), 8, 1, 2 * 118 - 17),
            ("left100", spliced[None], seq2[None], match_matrix(5, -4), 3, 0, 137),
            ("up3000", inserted[None], seq2[None], match_matrix(1, -1), 10, 0, 118)]


def mixed_inputs(n, len1, seed):
    """random pairs, with every third seq1 carrying a noisy copy of its seq2 with a gap in it (long paths through E and F),
    and some homopolymers (ties)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, 128), dtype=np.uint8)
    for k in range(0, n, 3):
        w = min(len1, 128)
        src = np.where(rng.random(w) < 0.85, b[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 20:
            cut, gap = int(rng.integers(5, w - 10)), int(rng.integers(1, 9))
            src = np.concatenate([src[:cut], src[cut + gap:], rng.integers(0, 4, gap, dtype=np.uint8)])[:w] \
                if k % 2 else np.concatenate([src[:cut], rng.integers(0, 4, gap, dtype=np.uint8), src[cut:]])[:w]
        at = int(rng.integers(0, len1 - w + 1))
        a[k, at:at + w] = src
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(128) < 0.8] = k & 3
    return a, b
