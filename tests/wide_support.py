"""Helpers of the wide-alphabet aligners' tests (test_wide_cpu.py, test_wide_gpu.py): the C restatement
tests/native/wide_affine_oracle.c compiled into a temporary directory, an independent numpy Gotoh over 32 letters for small
shapes, inputs over all 32 letters with junk in the bytes' high bits, the matrices, and the field-by-field comparison."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

LOCAL, GLOBAL = 0, 1
BEGIN1, BEGIN2, END1, END2 = 1, 2, 4, 8
ALL_MASKS = list(range(16))


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    if len(seqs):
        off[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
    return off


def concat(seqs):
    cat = np.concatenate([np.asarray(x, np.uint8) for x in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(np.concatenate([cat, np.zeros(16, np.uint8)]))      # never an empty buffer


def move_offsets(a, b):
    """The one move layout: SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) words per alignment."""
    mo = np.zeros(len(a) + 1, np.uint64)
    for k in range(len(a)):
        mo[k + 1] = mo[k] + np.uint64((((len(a[k]) + len(b[k]) + 31) // 32) + 1) & ~1)
    return mo


class WideOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libwide_affine_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "wide_affine_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, kind, a, b, sm, gap_open, gap_extend, free_ends=0, traceback=True):
        """(scores, ends[n, 4], moves (flat), move_offsets, steps) of lists of sequences a and b: the result layout of
        swmi.wide.local / global_."""
        n = len(a)
        cat1, cat2, off1, off2 = concat(a), concat(b), offsets(a), offsets(b)
        m = np.ascontiguousarray(np.asarray(sm).reshape(-1), np.int8)
        assert m.size == 1024
        mo = move_offsets(a, b)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros(int(mo[-1]) + 2, np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731
        rc = self.lib.wide_affine_oracle_ragged(int(kind), P(cat1), P(off1), P(cat2), P(off2), ctypes.c_size_t(n), P(m), int(gap_open),
                                                int(gap_extend), ctypes.c_uint(int(free_ends)), P(scores), P(ends), P(moves), P(mo),
                                                P(steps))
        assert rc == 0
        return scores, ends, moves, mo if traceback else None, steps


def assert_same(got, want, what, traceback=True):
    """Every field and every move of two results in the layout above (bits past the last step are unspecified)."""
    sc, ends, moves, mo, steps = got
    wsc, wends, wmoves, wmo, wsteps = want
    assert np.array_equal(sc, wsc), (what, "scores", np.flatnonzero(sc != wsc)[:8], sc[sc != wsc][:8], wsc[sc != wsc][:8])
    assert np.array_equal(ends, wends), (what, "ends", np.flatnonzero((ends != wends).any(axis=1))[:8])
    if not traceback:
        assert moves is None and steps is None
        return
    assert np.array_equal(steps, wsteps), (what, "steps", np.flatnonzero(steps != wsteps)[:8])
    assert np.array_equal(mo, wmo), (what, "move_offsets")
    for k in range(len(sc)):
        full, part = divmod(int(steps[k]), 32)
        at = int(mo[k])
        assert np.array_equal(moves[at:at + full], wmoves[at:at + full]), (what, "moves", k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (moves[at + full] & mask) == (wmoves[at + full] & mask), (what, "moves", k)


def asymmetric_matrix(seed, lo=-128, hi=127):
    """A random int8 matrix that is not symmetric, flat."""
    sm = np.random.default_rng(seed).integers(lo, hi + 1, (32, 32)).astype(np.int8)
    assert not np.array_equal(sm, sm.T)
    return sm.reshape(-1)


def scoring_matrix(seed):
    """Asymmetric, random, with a diagonal that makes related sequences align: paths of all three kinds of move."""
    rng = np.random.default_rng(seed)
    sm = rng.integers(-9, 4, (32, 32)).astype(np.int8)
    sm[np.arange(32), np.arange(32)] = rng.integers(3, 12, 32).astype(np.int8)
    return sm.reshape(-1)


def only_letter_31():
    """Every entry negative but the one of the pair (31, 31)."""
    sm = np.full((32, 32), -3, np.int8)
    sm[31, 31] = 5
    return sm.reshape(-1)


def embed_dna(sm16):
    sm = np.full((32, 32), -128, np.int8)
    sm[:4, :4] = np.asarray(sm16, np.int8).reshape(4, 4)
    return sm.reshape(-1)


def inputs(shapes, seed, letters=32, junk=True):
    """Pairs of the given (len1, len2) over `letters` letters: random; every third seq2 ends in a 90 % copy of (the end of) its
    seq1 with a 5-letter indel, so that a path runs through every wavefront and holds all three kinds of move; every seventh
    pair a run of one letter against a mostly equal one (ties).  With `junk` the bytes carry random bits 5 - 7."""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for k, (len1, len2) in enumerate(shapes):
        x = rng.integers(0, letters, len1, dtype=np.uint8)
        y = rng.integers(0, letters, len2, dtype=np.uint8)
        w = min(len1, len2)
        if k % 3 == 0 and w:
            src = np.where(rng.random(w) < 0.9, x[len1 - w:], rng.integers(0, letters, w)).astype(np.uint8)
            if w > 8:
                cut = int(rng.integers(1, w - 1))
                d = min(5, w - cut - 1)
                src = np.concatenate([src[:cut], src[cut + d:], rng.integers(0, letters, d, dtype=np.uint8)])
            y[len2 - w:] = src[:w]
        elif k % 7 == 1:
            x[:] = (letters - 1) if k % 2 else k % letters
            y[rng.random(len2) < 0.8] = x[0] if len1 else 0
        if junk:
            x = x | (rng.integers(0, 8, len1, dtype=np.uint8) << 5).astype(np.uint8)
            y = y | (rng.integers(0, 8, len2, dtype=np.uint8) << 5).astype(np.uint8)
        a.append(x.astype(np.uint8))
        b.append(y.astype(np.uint8))
    return a, b


def numpy_gotoh(kind, a, b, sm, gap_open, gap_extend, free_ends=0):
    """An independent formulation for small shapes: three whole int64 tables, the end cell by an argmax over H (masked to the
    allowed cells for the global kind), the three-state walk on the tables themselves.  (score, ends[4], moves as a list of
    codes in walking order)."""
    a = np.asarray(a, np.int64) & 31
    b = np.asarray(b, np.int64) & 31
    n1, n2 = len(a), len(b)
    S = np.asarray(sm, np.int64).reshape(32, 32)[a][:, b] if n1 and n2 else np.zeros((n1, n2), np.int64)
    neg = -(1 << 40)
    H = np.zeros((n1 + 1, n2 + 1), np.int64)
    E = np.full((n1 + 1, n2 + 1), neg, np.int64)
    F = np.full((n1 + 1, n2 + 1), neg, np.int64)
    if kind == GLOBAL:
        if not free_ends & BEGIN2:
            H[0, 1:] = -(gap_open + np.arange(n2) * gap_extend)
        if not free_ends & BEGIN1:
            H[1:, 0] = -(gap_open + np.arange(n1) * gap_extend)
    for i in range(1, n1 + 1):
        for j in range(1, n2 + 1):
            E[i, j] = max(H[i - 1, j] - gap_open, E[i - 1, j] - gap_extend)
            F[i, j] = max(H[i, j - 1] - gap_open, F[i, j - 1] - gap_extend)
            h = max(H[i - 1, j - 1] + S[i - 1, j - 1], E[i, j], F[i, j])
            H[i, j] = max(h, 0) if kind == LOCAL else h
    if kind == LOCAL:
        i, j = divmod(int(np.argmax(H.reshape(-1))), n2 + 1) if H.max() > 0 else (0, 0)
    else:
        allowed = np.zeros(H.shape, bool)
        allowed[n1, n2] = True
        if free_ends & END1:
            allowed[:, n2] = True
        if free_ends & END2:
            allowed[n1, :] = True
        i, j = divmod(int(np.argmax(np.where(allowed, H, np.iinfo(np.int64).min).reshape(-1))), n2 + 1)
    end, score, moves, state = (i, j), int(H[i, j]), [], "H"
    while i or j:
        if i == 0 or j == 0:
            if kind == LOCAL or (i == 0 and free_ends & BEGIN2) or (j == 0 and free_ends & BEGIN1):
                break
            m = 1 if i == 0 else 2
        else:
            if state == "H":
                if kind == LOCAL and H[i, j] == 0:
                    break
                if H[i, j] != H[i - 1, j - 1] + S[i - 1, j - 1]:
                    state = "E" if H[i, j] == E[i, j] else "F"
            if state == "H":
                m = 3
            elif state == "E":
                m = 2
                state = "H" if E[i, j] == H[i - 1, j] - gap_open else "E"
            else:
                m = 1
                state = "H" if F[i, j] == H[i, j - 1] - gap_open else "F"
        moves.append(m)
        i -= m != 1
        j -= m != 2
    return score, [end[0], end[1], i, j], moves


def moves_of(result, k):
    """Alignment k's move codes in walking order, from a result in the layout above."""
    _, _, moves, mo, steps = result
    at = int(mo[k])
    return [int(moves[at + (t >> 5)] >> np.uint64(2 * (t & 31))) & 3 for t in range(int(steps[k]))]
