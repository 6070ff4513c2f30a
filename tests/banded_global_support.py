"""Helpers of the banded global / fit / overlap / extension aligner's tests (test_banded_global_cpu.py, test_banded_global_gpu.py):
the C restatement tests/native/banded_global_oracle.c compiled into a temporary directory, an independent numpy formulation
(three full tables with -infinity outside the band), the case generators and the slice arithmetic of
include/swmi_banded_global.h."""
import ctypes
import os
import subprocess

import numpy as np

from banded_align_support import INT32_MAX, INT32_MIN, RELATED_PARAMS, TB_BUDGET, in_band, related_pairs  # noqa: F401  (re-exported)
from conftest import ROOT
from global_full_support import BEGIN1, BEGIN2, END1, END2  # noqa: F401
from local_full_support import assert_same, move_words, moves_of, path_from  # noqa: F401  (re-exported)

LO, HI = -64, 63
MAX_LEN = 16384
ANYWHERE = 16
EXTEND = 16
NO_ALIGNMENT = INT32_MIN
ALL_MASKS = tuple(range(20))
IDENTITY_MASKS = (0, 3, 5, 10, 12, 15)
NEG = -(1 << 40)


class BandedGlobalOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libbanded_global_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "banded_global_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True, lo=LO, hi=HI):
        """(scores, ends[n, 4], moves[n, move_words], steps) for n pairs of one (len1, len2) under one mask."""
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
        rc = self.lib.banded_global_oracle_batch(P(a), ctypes.c_size_t(len1), P(b), ctypes.c_size_t(len2), ctypes.c_size_t(n), P(d),
                                                 int(lo), int(hi), P(m), int(gap_open), int(gap_extend), ctypes.c_uint(int(free_ends)),
                                                 P(scores), P(ends), P(moves), ctypes.c_size_t(mw), P(steps))
        assert rc == 0
        return scores, ends, moves, steps


def code_bytes(len1):
    """bytes of codes one alignment of a traceback launch takes: 256 per trip of four iterations, len1 + 64 iterations (row 0
    is swept)"""
    return 256 * (-(-(len1 + 64) // 4))


def per_alignment(len1, len2, traceback):
    """device bytes one alignment of a slice takes (inputs, diagonal, score, four ends; codes, moves and steps with a traceback)"""
    per = len1 + len2 + 4 + 4 + 16
    if traceback:
        per += code_bytes(len1) + 8 * move_words(len1, len2) + 4
    return per


def band_mask(len1, len2, d0=0, lo=LO, hi=HI):
    """bool (len1 + 1) x (len2 + 1): the table's cells in the band"""
    ii, jj = np.meshgrid(np.arange(len1 + 1), np.arange(len2 + 1), indexing="ij")
    return (jj - ii - int(d0) >= lo) & (jj - ii - int(d0) <= hi)


def numpy_banded_global(a, b, sm, gap_open, gap_extend, free_ends, d0=0, lo=LO, hi=HI):
    """An independent formulation for small shapes: three full (len1 + 1) x (len2 + 1) int64 tables with NEG outside the band
    (NEG is absorbing: anything made from it is put back to NEG), the end cell by a masked argmax over the whole of H, then the
    three-state walk on the tables themselves.  (score or None, (end_i, end_j), path from the start cell to the end cell, H)."""
    a = np.asarray(a, np.int64) & 3
    b = np.asarray(b, np.int64) & 3
    n1, n2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)
    band = band_mask(n1, n2, d0, lo, hi)
    H = np.full((n1 + 1, n2 + 1), NEG, np.int64)
    E = H.copy()
    F = H.copy()
    fin = lambda v: v > NEG // 2  # noqa: E731
    origin = bool(band[0, 0])
    for i in range(n1 + 1):
        for j in range(n2 + 1):
            if not band[i, j]:
                continue
            if i == 0 and j == 0:
                H[i, j] = 0
            elif i == 0:
                H[i, j] = 0 if free_ends & BEGIN2 else -(gap_open + (j - 1) * gap_extend) if origin else NEG
            elif j == 0:
                H[i, j] = 0 if free_ends & BEGIN1 else -(gap_open + (i - 1) * gap_extend) if origin else NEG
            else:
                e = max(H[i - 1, j] - gap_open if fin(H[i - 1, j]) else NEG, E[i - 1, j] - gap_extend if fin(E[i - 1, j]) else NEG)
                f = max(H[i, j - 1] - gap_open if fin(H[i, j - 1]) else NEG, F[i, j - 1] - gap_extend if fin(F[i, j - 1]) else NEG)
                d = H[i - 1, j - 1] + S[a[i - 1], b[j - 1]] if fin(H[i - 1, j - 1]) else NEG
                E[i, j], F[i, j], H[i, j] = e, f, max(d, e, f)
    allowed = np.zeros(H.shape, bool)
    allowed[n1, n2] = True
    if free_ends & END1:
        allowed[:, n2] = True
    if free_ends & END2:
        allowed[n1, :] = True
    if free_ends & ANYWHERE:
        allowed[:, :] = True
    masked = np.where(allowed & band, H, NEG)
    i, j = divmod(int(np.argmax(masked.reshape(-1))), n2 + 1)        # the first maximum in row-major order
    if not fin(masked[i, j]):
        return None, (0, 0), np.zeros((1, 2), np.int32), H
    end = (i, j)
    path, state = [(i, j)], "H"
    while i or j:
        if i == 0:
            if free_ends & BEGIN2:
                break
            j -= 1
        elif j == 0:
            if free_ends & BEGIN1:
                break
            i -= 1
        else:
            if state == "H" and not (fin(H[i - 1, j - 1]) and H[i, j] == H[i - 1, j - 1] + S[a[i - 1], b[j - 1]]):
                state = "E" if H[i, j] == E[i, j] else "F"
            if state == "H":
                i, j = i - 1, j - 1
            elif state == "E":
                state = "H" if fin(H[i - 1, j]) and E[i, j] == H[i - 1, j] - gap_open else "E"
                i -= 1
            else:
                state = "H" if fin(H[i, j - 1]) and F[i, j] == H[i, j - 1] - gap_open else "F"
                j -= 1
        assert band[i, j], "the walk left the band"
        path.append((i, j))
    return int(H[end]), end, np.array(path[::-1], np.int32).reshape(-1, 2), H


def feasible_by_hand(len1, len2, d0, free_ends):
    """Whether an alignment exists, from the geometry alone: a start cell the mask allows in the band ((0,0); column 0 with
    BEGIN1; row 0 with BEGIN2) and a candidate end cell in the band.  The band's part of the table is connected by down, right
    and diagonal moves from any such start to any such end that lies below or right of it, which these do."""
    band = band_mask(len1, len2, d0)
    start = band[0, 0] or (free_ends & BEGIN1 and band[:, 0].any()) or (free_ends & BEGIN2 and band[0, :].any())
    end = band[len1, len2] or (free_ends & END1 and band[:, len2].any()) or (free_ends & END2 and band[len1, :].any()) or \
        (free_ends & ANYWHERE and band.any())
    return bool(start and end)


def band_leaver(rng, n, len1=400):
    """Pairs whose best global path must leave the band: seq2 = seq1 with 80 bases deleted and, 150 bases on, 80 random bases
    inserted (len2 = len1): between the two the path runs 80 diagonals below the main one."""
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = np.empty_like(a)
    for k in range(n):
        b[k] = np.concatenate([a[k, :60], a[k, 140:290], rng.integers(0, 4, 80, dtype=np.uint8), a[k, 290:]])
    return a, b
