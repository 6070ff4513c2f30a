"""Helpers of the any-length local aligner's tests (test_local_full_cpu.py, test_local_full_gpu.py): the C restatement
tests/native/local_full_oracle.c, compiled into a temporary directory, an independent numpy formulation for small shapes,
and the checks every path has to pass whatever the tie rules."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT


def move_words(len1, len2):
    return (((len1 + len2 + 31) // 32) + 1) & ~1


class LocalFullOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "liblocal_full_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "local_full_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap, traceback=True):
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
        rc = self.lib.local_full_oracle_batch(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                              b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                              m.ctypes.data_as(ctypes.c_void_p), int(gap), scores.ctypes.data_as(ctypes.c_void_p),
                                              ends.ctypes.data_as(ctypes.c_void_p),
                                              moves.ctypes.data_as(ctypes.c_void_p) if traceback else None, ctypes.c_size_t(mw),
                                              steps.ctypes.data_as(ctypes.c_void_p) if traceback else None)
        assert rc == 0
        return scores, ends, moves, steps


def numpy_table(a, b, sm, gap):
    """(H, S): the whole local table by anti-diagonals in numpy, and the score of every cell's pair of bases."""
    len1, len2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)[np.asarray(a) & 3][:, np.asarray(b) & 3]
    H = np.zeros((len1 + 1, len2 + 1), np.int64)
    for d in range(2, len1 + len2 + 1):
        i = np.arange(max(1, d - len2), min(len1, d - 1) + 1)
        j = d - i
        H[i, j] = np.maximum(np.maximum(0, H[i - 1, j - 1] + S[i - 1, j - 1]), np.maximum(H[i - 1, j], H[i, j - 1]) - gap)
    return H, S


def numpy_local_full(a, b, sm, gap):
    """An independent formulation for small sizes: numpy_table, then the reference's walk on it.
    (score, (end_i, end_j), path from the start cell to the end cell, H)."""
    H, S = numpy_table(a, b, sm, gap)
    flat = H.reshape(-1)
    pos = int(np.argmax(flat))                     # the first maximum in row-major order
    if flat[pos] <= 0:
        pos = 0
    i, j = divmod(pos, len(b) + 1)
    end = (i, j)
    path = [(i, j)]
    while H[i, j] != 0:
        if H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
            i, j = i - 1, j - 1
        elif H[i, j] == H[i - 1, j] - gap:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return int(flat[pos]), end, np.array(path[::-1], np.int32).reshape(-1, 2), H


def moves_of(moves_row, steps):
    """The first `steps` move codes of a row, in walking order."""
    t = np.arange(int(steps))
    return ((np.asarray(moves_row, np.uint64)[t // 32] >> (2 * (t % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)


def path_from(moves_row, steps, end_i, end_j):
    """Reference-order path (start -> end) from walking-order moves, in numpy (independent of the library's expander)."""
    c = moves_of(moves_row, steps)
    assert np.all(c > 0)
    i = int(end_i) - np.concatenate([[0], np.cumsum(c != 1)])
    j = int(end_j) - np.concatenate([[0], np.cumsum(c != 2)])
    return np.stack([i, j], axis=1)[::-1].astype(np.int32)


def check_path(a, b, sm, gap, score, ends, moves_row, steps, H=None):
    """What every local path satisfies whatever the tie rules: its steps re-scored from the sequences give the score, it
    starts where it says, never leaves the matrix, and (with the table H of a small shape) its start cell holds 0 and no cell
    strictly inside it does."""
    path = path_from(moves_row, steps, ends[0], ends[1])
    assert tuple(path[0]) == (int(ends[2]), int(ends[3])) and tuple(path[-1]) == (int(ends[0]), int(ends[1]))
    assert path.min() >= 0
    d = np.diff(path, axis=0)
    diag = (d[:, 0] == 1) & (d[:, 1] == 1)
    S = np.asarray(sm, np.int64).reshape(4, 4)
    i, j = path[1:, 0][diag], path[1:, 1][diag]
    total = int(S[np.asarray(a)[i - 1] & 3, np.asarray(b)[j - 1] & 3].sum()) - int(gap) * int((~diag).sum())
    assert total == int(score), (total, int(score))
    if H is not None:
        assert H[path[0, 0], path[0, 1]] == 0
        assert np.all(H[path[1:, 0], path[1:, 1]] > 0)
        assert H[path[-1, 0], path[-1, 1]] == int(score)
    return path


def assert_same(got, want, what, traceback=True):
    """Every field of two results equal; moves up to `steps` only (words past it are unspecified)."""
    sc, ends, mv, st = got
    wsc, wends, wmv, wst = want
    assert np.array_equal(sc, wsc), (what, np.flatnonzero(sc != wsc)[:8])
    if not traceback:
        assert np.array_equal(ends[:, :2], wends[:, :2]), (what, np.flatnonzero((ends[:, :2] != wends[:, :2]).any(axis=1))[:8])
        assert np.all(ends[:, 2:] == -1), what
        return
    assert np.array_equal(ends, wends), (what, np.flatnonzero((ends != wends).any(axis=1))[:8])
    assert np.array_equal(st, wst), (what, np.flatnonzero(st != wst)[:8])
    for k in range(len(sc)):
        full, part = divmod(int(st[k]), 32)
        assert np.array_equal(mv[k, :full], wmv[k, :full]), (what, k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (mv[k, full] & mask) == (wmv[k, full] & mask), (what, k)


def inputs(n, len1, len2, seed):
    """Random pairs; every third seq2 a 90 % copy of its seq1 with a 5-base indel (long diagonal paths), every seventh pair a
    homopolymer (ties)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, (n, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (n, len2), dtype=np.uint8)
    w = min(len1, len2)
    for k in range(0, n, 3):
        src = np.where(rng.random(w) < 0.9, a[k, :w], rng.integers(0, 4, w)).astype(np.uint8)
        if w > 8:
            cut = int(rng.integers(1, w - 1))
            src = np.concatenate([src[:cut], src[cut + min(5, w - cut - 1):], rng.integers(0, 4, min(5, w - cut - 1), dtype=np.uint8)])
        b[k, :w] = src[:w]
    for k in range(1, n, 7):
        a[k] = k & 3
        b[k, rng.random(len2) < 0.8] = k & 3
    return a, b
