"""Helpers of the local-aligner tests (test_local_cpu.py, test_local_gpu.py): the C restatement tests/native/local_oracle.c,
compiled into a temporary directory, and the F7 fixture split into alignments."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

PARAMS = [(10, -30, 15), (1, -1, 1), (5, -4, 0), (127, -127, 127), (2, -3, 5)]


def move_words(len1):
    return (((len1 + 128 + 31) // 32) + 1) & ~1


class LocalOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "liblocal_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "local_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, seq1s, seq2s, sm, gap):
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
        rc = self.lib.local_oracle_batch(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                         b.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), m.ctypes.data_as(ctypes.c_void_p),
                                         int(gap), scores.ctypes.data_as(ctypes.c_void_p), ends.ctypes.data_as(ctypes.c_void_p),
                                         moves.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(mw),
                                         steps.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0
        return scores, ends, moves, steps


def moves_to_path(moves_row, steps, end_i, end_j):
    """Reference-order path (start -> end) from walking-order moves, in Python (independent of the library's expander)."""
    i, j = int(end_i), int(end_j)
    path = [(i, j)]
    for t in range(int(steps)):
        c = (int(moves_row[t // 32]) >> (2 * (t % 32))) & 3
        i -= 1 if c in (3, 2) else 0
        j -= 1 if c in (3, 1) else 0
        path.append((i, j))
    return np.array(path[::-1], np.int32).reshape(-1, 2)


def path_to_moves(path, words):
    """Walking-order moves of a reference path (start -> end)."""
    row = np.zeros(words, np.uint64)
    p = np.asarray(path)
    for t in range(len(p) - 1):
        (i1, j1), (i0, j0) = p[len(p) - 1 - t], p[len(p) - 2 - t]
        c = 3 if (i1 - i0, j1 - j0) == (1, 1) else 2 if (i1 - i0, j1 - j0) == (1, 0) else 1
        row[t // 32] |= np.uint64(c << (2 * (t % 32)))
    return row


def load_f7():
    """F7 as a list of dicts: len1, kind, seq1, seq2, score, path."""
    f = np.load(os.path.join(GOLDEN, "f7_local.npz"), allow_pickle=False)
    out = []
    for k in range(len(f["lens"])):
        out.append(dict(len1=int(f["lens"][k]), kind=str(f["kind_names"][f["kinds"][k]]),
                        seq1=f["seq1"][f["seq1_off"][k]:f["seq1_off"][k + 1]], seq2=f["seq2"][k], score=int(f["scores"][k]),
                        path=f["path"][f["path_off"][k]:f["path_off"][k + 1]]))
    return out


def f7_by_length():
    """{len1: (seq1s[n, len1], seq2s[n, 128], scores[n], paths list)} of F7."""
    groups = {}
    for v in load_f7():
        groups.setdefault(v["len1"], []).append(v)
    return {L: (np.stack([v["seq1"] for v in vs]), np.stack([v["seq2"] for v in vs]), np.array([v["score"] for v in vs], np.int32),
                [v["path"] for v in vs]) for L, vs in sorted(groups.items())}


def random_matrix(seed=11):
    """An asymmetric int8 matrix (sm[a*4+b] != sm[b*4+a])."""
    rng = np.random.default_rng(seed)
    sm = rng.integers(-20, 21, 16).astype(np.int8)
    sm[1], sm[4] = 7, -9
    return sm
