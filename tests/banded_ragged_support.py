"""Helpers of the mixed-shape banded aligners' tests (test_banded_ragged_cpu.py, test_banded_ragged_gpu.py): the two existing C
restatements, tests/native/banded_align_oracle.c and tests/native/banded_global_oracle.c, compiled into ONE shared object in a
temporary directory and called through their SINGLE-ALIGNMENT functions, once per alignment with that alignment's lengths and
diagonal, the moves laid out by move_offsets; the batch container; the comparison; and the slice arithmetic of
include/swmi_banded_ragged.h.  There is no restatement of the recurrences here."""
import ctypes
import os
import subprocess

import numpy as np

from banded_align_support import INT32_MAX, INT32_MIN, RELATED_PARAMS, TB_BUDGET, related_pairs  # noqa: F401  (re-exported)
from conftest import ROOT
from local_full_support import move_words, moves_of, path_from  # noqa: F401  (re-exported)

LOCAL, GLOBAL = 0, 1
LO, HI = -64, 63
MAX_LEN = 16384
NO_ALIGNMENT = INT32_MIN
ALL_MASKS = tuple(range(20))
SLOT_BYTES = 48
EO_BUDGET = 256 << 20
MAX_SLICE = 1 << 20
FORMS = [(5, 1), (1, 3)]                    # open >= extend, open < extend: the two instantiations


class Batch:
    """A mixed batch: lists of 1-D uint8 arrays and one int32 diagonal per alignment (or None)."""

    def __init__(self, seq1s, seq2s, diagonals=None):
        self.seq1s = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in seq1s]
        self.seq2s = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in seq2s]
        assert len(self.seq1s) == len(self.seq2s)
        self.n = len(self.seq1s)
        self.diagonals = None if diagonals is None else np.ascontiguousarray(diagonals, np.int32).reshape(self.n)
        self.off1 = np.concatenate([[0], np.cumsum([len(x) for x in self.seq1s])]).astype(np.uint64)
        self.off2 = np.concatenate([[0], np.cumsum([len(x) for x in self.seq2s])]).astype(np.uint64)
        self.cat1 = np.concatenate(self.seq1s + [np.zeros(0, np.uint8)])
        self.cat2 = np.concatenate(self.seq2s + [np.zeros(0, np.uint8)])
        self.move_offsets = np.concatenate([[0], np.cumsum([move_words(len(x), len(y)) for x, y in zip(self.seq1s, self.seq2s)])]).astype(np.uint64)

    def shapes(self):
        return [(len(x), len(y)) for x, y in zip(self.seq1s, self.seq2s)]

    def reversed(self):
        return Batch(self.seq1s[::-1], self.seq2s[::-1], None if self.diagonals is None else self.diagonals[::-1])

    def __add__(self, other):
        assert (self.diagonals is None) == (other.diagonals is None)
        return Batch(self.seq1s + other.seq1s, self.seq2s + other.seq2s,
                     None if self.diagonals is None else np.concatenate([self.diagonals, other.diagonals]))


class RaggedOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libbanded_ragged_oracle.so")
        native = os.path.join(ROOT, "tests", "native")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so, os.path.join(native, "banded_align_oracle.c"),
                               os.path.join(native, "banded_global_oracle.c")])
        self.lib = ctypes.CDLL(so)
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        self.lib.banded_align_oracle.argtypes = [vp, sz, vp, sz, ctypes.c_int32, ci, ci, vp, ci, ci, vp, vp, vp, vp]
        self.lib.banded_global_oracle.argtypes = [vp, sz, vp, sz, ctypes.c_int32, ci, ci, vp, ci, ci, ctypes.c_uint, vp, vp, vp, vp]

    def align(self, kind, batch, sm, gap_open, gap_extend, free_ends=0, traceback=True):
        """(scores, ends[n, 4], moves flat, steps): one call of the kind's single-alignment restatement per alignment."""
        m = np.ascontiguousarray(sm, np.int8)
        n = batch.n
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros(int(batch.move_offsets[-1]) + 1, np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        pad = np.zeros(1, np.uint8)
        for k in range(n):
            a, b = batch.seq1s[k], batch.seq2s[k]
            d = 0 if batch.diagonals is None else int(batch.diagonals[k])
            head = ((a if len(a) else pad).ctypes.data, len(a), (b if len(b) else pad).ctypes.data, len(b), d, LO, HI, m.ctypes.data,
                    int(gap_open), int(gap_extend))
            tail = (scores[k:].ctypes.data, ends[k:].ctypes.data, moves[int(batch.move_offsets[k]):].ctypes.data if traceback else None,
                    steps[k:].ctypes.data if traceback else None)
            if kind == GLOBAL:
                rc = self.lib.banded_global_oracle(*head, int(free_ends), *tail)
            else:
                rc = self.lib.banded_align_oracle(*head, *tail)
            assert rc == 0
        return scores, ends, None if moves is None else moves[:-1], steps


def assert_same(got, want, batch, what, traceback=True):
    """Every field of two results equal; an alignment's moves word for word up to its `steps` (words past it are unspecified)."""
    sc, ends, mv, st = got
    wsc, wends, wmv, wst = want
    assert np.array_equal(sc, wsc), (what, "scores", np.flatnonzero(sc != wsc)[:8])
    if not traceback:
        assert np.array_equal(ends[:, :2], wends[:, :2]), (what, "end cells", np.flatnonzero((ends[:, :2] != wends[:, :2]).any(axis=1))[:8])
        assert np.all(ends[:, 2:] == -1), what
        return
    assert np.array_equal(ends, wends), (what, "ends", np.flatnonzero((ends != wends).any(axis=1))[:8])
    assert np.array_equal(st, wst), (what, "steps", np.flatnonzero(st != wst)[:8])
    for k in range(len(sc)):
        at = int(batch.move_offsets[k])
        full, part = divmod(int(st[k]), 32)
        assert at + full + (1 if part else 0) <= int(batch.move_offsets[k + 1]), (what, k)
        assert np.array_equal(mv[at:at + full], wmv[at:at + full]), (what, "moves", k)
        if part:
            mask = np.uint64((1 << (2 * part)) - 1)
            assert (mv[at + full] & mask) == (wmv[at + full] & mask), (what, "last move word", k)


def permuted(result, batch, order):
    """result of batch[order] -> the result in batch's own order (moves laid out by batch.move_offsets)"""
    sc, ends, mv, st = result
    inv = np.empty(len(order), np.int64)
    inv[np.asarray(order)] = np.arange(len(order))
    out_mv = None
    if mv is not None:
        sub = Batch([batch.seq1s[k] for k in order], [batch.seq2s[k] for k in order])
        out_mv = np.zeros(int(batch.move_offsets[-1]), np.uint64)
        for pos, k in enumerate(order):
            w = int(batch.move_offsets[k + 1] - batch.move_offsets[k])
            out_mv[int(batch.move_offsets[k]):int(batch.move_offsets[k]) + w] = mv[int(sub.move_offsets[pos]):int(sub.move_offsets[pos]) + w]
    return sc[inv], ends[inv], out_mv, None if st is None else st[inv]


def code_bytes(kind, len1):
    """bytes of codes one alignment of a traceback launch takes: 256 per trip of four iterations; len1 + 63 iterations for the
    local kind, len1 + 64 for the global kind (row 0 is swept)"""
    return 256 * (-(-(len1 + (64 if kind == GLOBAL else 63)) // 4))


def per_alignment(kind, len1, len2, traceback):
    """device bytes one alignment of a slice takes (the header's arithmetic)"""
    per = len1 + len2 + SLOT_BYTES + 20
    if traceback:
        per += code_bytes(kind, len1) + 8 * move_words(len1, len2) + 4
    return per


def slices_by_hand(kind, shapes, traceback):
    """the header's slices, recomputed: longest runs in caller order within the byte budget, at most 2^20 alignments, at least one"""
    cap = TB_BUDGET if traceback else EO_BUDGET
    out, bytes_, m = [], 0, 0
    for len1, len2 in shapes:
        b = per_alignment(kind, len1, len2, traceback)
        if m and (bytes_ + b > cap or m == MAX_SLICE):
            out.append(m)
            bytes_, m = 0, 0
        bytes_ += b
        m += 1
    if m:
        out.append(m)
    return out


def related_batch(rng, shapes, diagonals, sub=0.08):
    """one related pair (banded_align_support.related_pairs) per (len1, len2) and diagonal"""
    s1, s2 = [], []
    for (len1, len2), d in zip(shapes, diagonals):
        a, b = related_pairs(rng, 1, len1, len2, int(np.clip(d, 1 - len1, len2 - 1)), sub=sub)
        s1.append(a[0])
        s2.append(b[0])
    return Batch(s1, s2, np.asarray(diagonals, np.int32))
