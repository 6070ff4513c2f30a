"""Helpers of the exact semi-global tests (test_sgfull_cpu.py, test_sgfull_gpu.py): the C restatement
tests/native/sgfull_oracle.c, compiled into a temporary directory, and the F8 fixture."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

K111 = np.array([1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1], np.int8)


def move_words(len1, len2):
    return (((len1 + len2 + 31) // 32) + 1) & ~1


class SgFullOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libsgfull_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "sgfull_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap, traceback=True):
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
        rc = self.lib.sgfull_oracle_batch(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                          b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len2), ctypes.c_size_t(n),
                                          m.ctypes.data_as(ctypes.c_void_p), int(gap), scores.ctypes.data_as(ctypes.c_void_p),
                                          ends.ctypes.data_as(ctypes.c_void_p),
                                          moves.ctypes.data_as(ctypes.c_void_p) if traceback else None, ctypes.c_size_t(mw),
                                          lengths.ctypes.data_as(ctypes.c_void_p) if traceback else None)
        assert rc == 0
        return scores, ends, moves, lengths


def moves_to_path(moves_row, length, end_i, end_j):
    """Reference-order path ((0,0) -> best cell) from walking-order moves, in Python (independent of the library)."""
    i, j = int(end_i), int(end_j)
    path = [(i, j)]
    for t in range(int(length) - 1):
        c = (int(moves_row[t // 32]) >> (2 * (t % 32))) & 3
        i -= 1 if c in (3, 2) else 0
        j -= 1 if c in (3, 1) else 0
        path.append((i, j))
    return np.array(path[::-1], np.int32).reshape(-1, 2)


def path_to_moves(path, words):
    """Walking-order moves of a reference path ((0,0) -> best cell)."""
    row = np.zeros(words, np.uint64)
    d = np.diff(np.asarray(path), axis=0)[::-1]
    codes = np.where((d[:, 0] == 1) & (d[:, 1] == 1), 3, np.where(d[:, 0] == 1, 2, 1)).astype(np.uint64)
    for t, c in enumerate(codes):
        row[t // 32] |= c << np.uint64(2 * (t % 32))
    return row


def load_f8():
    """F8 as a dict of arrays plus 'paths' (the reference's (i, j) lists) and 'kind' names."""
    f = np.load(os.path.join(GOLDEN, "f8_sgfull.npz"), allow_pickle=False)
    out = {k: f[k] for k in f.files}
    step = np.array([[0, 0], [1, 1], [1, 0], [0, 1]], np.int32)
    paths = []
    for k in range(len(out["scores"])):
        mv = out["moves"][out["move_offsets"][k]: out["move_offsets"][k + 1]]
        paths.append(np.concatenate([np.zeros((1, 2), np.int32), np.cumsum(step[mv], axis=0, dtype=np.int32)]))
    out["paths"] = paths
    out["kind"] = [str(out["kind_names"][i]) for i in out["kinds"]]
    return out


def numpy_sgfull(a, b, sm, gap):
    """An independent formulation for small sizes: the whole table by anti-diagonals in numpy, then the reference's walk
    on it.  (score, (i, j), path from (0,0))."""
    len1, len2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(4, 4)[np.asarray(a) & 3][:, np.asarray(b) & 3]
    H = np.full((len1 + 1, len2 + 1), np.iinfo(np.int64).min // 4, np.int64)
    H[0, :] = -np.arange(len2 + 1) * gap
    H[:, 0] = -np.arange(len1 + 1) * gap
    for d in range(2, len1 + len2 + 1):
        i = np.arange(max(1, d - len2), min(len1, d - 1) + 1)
        j = d - i
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + S[i - 1, j - 1], H[i - 1, j] - gap), H[i, j - 1] - gap)
    flat = H.reshape(-1)
    pos = int(np.argmax(flat))                     # the first maximum in row-major order
    if flat[pos] <= 0:
        pos = 0
    bi, bj = divmod(pos, len2 + 1)
    path = [(bi, bj)]
    i, j = bi, bj
    while i or j:
        if i and j and H[i, j] == H[i - 1, j - 1] + S[i - 1, j - 1]:
            i, j = i - 1, j - 1
        elif i and H[i, j] == H[i - 1, j] - gap:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return int(flat[pos]) if pos else 0, (bi, bj), np.array(path[::-1], np.int32)
