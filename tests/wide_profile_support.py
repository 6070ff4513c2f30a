"""Helpers of the profile aligners' tests (test_wide_profile_cpu.py, test_wide_profile_gpu.py): the C restatement
tests/native/wide_profile_oracle.c compiled into a temporary directory, an independent numpy Gotoh with position scores for
small shapes, the profiles, and THE batch that the GPU tests run -- built here so that the CPU tests can show, through the
restatement alone, that it is not trivial.  Results have wide_support's layout, so its assert_same and moves_of apply."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT
from wide_support import BEGIN1, BEGIN2, END1, END2, GLOBAL, LOCAL, concat, offsets

LEN1S = [0, 1, 2, 31, 32, 33, 127, 128, 129, 200]
LEN2S = [1, 15, 16, 17, 1023, 1024, 1025, 2049, 3073, 4096]
LONG_LEN2 = 3                       # the one len2 whose batch also holds a sequence of 16384
PROFILES = ["scoring", "random_int8", "all_-128", "all_127"]
GAPS = {"scoring": (6, 1), "random_int8": (40, 9), "all_-128": (3, 2), "all_127": (0, 0)}
SEAMS = (1024, 2048, 3072)


def move_offsets(seqs, len2):
    """The one move layout: SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) words per alignment."""
    mo = np.zeros(len(seqs) + 1, np.uint64)
    for k in range(len(seqs)):
        mo[k + 1] = mo[k] + np.uint64((((len(seqs[k]) + len2 + 31) // 32) + 1) & ~1)
    return mo


class ProfileOracle:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libwide_profile_oracle.so")
        subprocess.check_call(["gcc", "-O2", "-fopenmp", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "wide_profile_oracle.c")])
        self.lib = ctypes.CDLL(so)

    def align(self, kind, seqs, profile, gap_open, gap_extend, free_ends=0, traceback=True):
        """(scores, ends[n, 4], moves (flat), move_offsets, steps) of a list of sequences (or a (concatenated, offsets) pair)
        against profile (len2 * 32 int8): the result layout of swmi.wide_profile.local / global_."""
        p = np.ascontiguousarray(np.asarray(profile).reshape(-1), np.int8)
        assert p.size % 32 == 0
        len2 = p.size // 32
        p = np.concatenate([p, np.zeros(32, np.int8)])        # never an empty buffer
        if isinstance(seqs, tuple):                           # (concatenated, offsets[n + 1]): a batch too large for a list
            cat, off = seqs
            lens = np.diff(off.astype(np.int64))
            mo = np.zeros(len(off), np.uint64)
            mo[1:] = np.cumsum((((lens + len2 + 31) // 32) + 1) & ~1)
        else:
            cat, off, mo = concat(seqs), offsets(seqs), move_offsets(seqs, len2)
        n = len(off) - 1
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros(int(mo[-1]) + 2, np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p) if x is not None else None  # noqa: E731
        rc = self.lib.wide_profile_oracle_ragged(int(kind), P(cat), P(off), ctypes.c_size_t(n), P(p), ctypes.c_size_t(len2), int(gap_open),
                                                 int(gap_extend), ctypes.c_uint(int(free_ends)), P(scores), P(ends), P(moves), P(mo), P(steps))
        assert rc == 0
        return scores, ends, moves, mo if traceback else None, steps


def numpy_gotoh_profile(kind, a, profile, gap_open, gap_extend, free_ends=0):
    """wide_support.numpy_gotoh's recurrence restated for position scores: three whole int64 tables, S[i, j] = profile[j, a[i]],
    the end cell by an argmax over H (masked to the allowed cells for the global kind), the three-state walk on the tables
    themselves.  (score, ends[4], moves as a list of codes in walking order)."""
    a = np.asarray(a, np.int64) & 31
    prof = np.asarray(profile, np.int64).reshape(-1, 32)
    n1, n2 = len(a), len(prof)
    S = prof[:, a].T if n1 and n2 else np.zeros((n1, n2), np.int64)
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


def from_sequence(query, sm):
    """profile[j, a] = sm[a * 32 + (query[j] & 31)], in numpy."""
    q = np.asarray(query, np.int64) & 31
    return np.ascontiguousarray(np.asarray(sm, np.int8).reshape(32, 32)[:, q].T)


def scoring_profile(len2, seed=5):
    """(len2, 32) int8: random in [-9, 3], and per column one consensus letter worth 3 .. 11: related sequences align, with
    paths of all three kinds of move."""
    rng = np.random.default_rng(seed * 10007 + len2)
    p = rng.integers(-9, 4, (len2, 32)).astype(np.int8)
    cons = rng.integers(0, 32, len2)
    p[np.arange(len2), cons] = rng.integers(3, 12, len2).astype(np.int8)
    return p


def consensus(profile):
    return np.argmax(np.asarray(profile).reshape(-1, 32), axis=1).astype(np.uint8)


def profile_for(name, len2):
    if name == "scoring":
        return scoring_profile(len2)
    if name == "random_int8":
        return np.random.default_rng(4000 + len2).integers(-128, 128, (len2, 32)).astype(np.int8)
    return np.full((len2, 32), {"all_-128": -128, "all_127": 127}[name], np.int8)


def noisy(rng, piece):
    """A 90 % copy of a stretch of consensus letters, five letters cut out of it and three random ones put in."""
    piece = np.where(rng.random(len(piece)) < 0.9, piece, rng.integers(0, 32, len(piece))).astype(np.uint8)
    if len(piece) > 24:
        cut = int(rng.integers(4, len(piece) // 2 - 6))
        piece = np.concatenate([piece[:cut], piece[cut + 5:]])
        put = int(rng.integers(len(piece) // 2 + 2, len(piece) - 4))
        piece = np.concatenate([piece[:put], rng.integers(0, 32, 3, dtype=np.uint8), piece[put:]])
    return piece


def sequences_for(len2, seed=9):
    """THE batch of one len2: sequences of LEN1S (and one of 16384 at len2 = 3) over all 32 letters with junk in bits 5 - 7.  From
    31 letters on they hold noisy copies of stretches of scoring_profile(len2)'s consensus: those of 31 .. 33 of its last
    columns (the padding inside the last lane and wave), those of 127, 128 and 129 a window across column 1024, 2048 and 3072
    (where len2 reaches; else across the middle), that of 200 four pieces, one out of each quarter of the columns (a global path
    through every wave)."""
    rng = np.random.default_rng(seed * 7919 + len2)
    cons = consensus(scoring_profile(len2))
    seqs = []
    for len1 in LEN1S + ([16384] if len2 == LONG_LEN2 else []):
        x = rng.integers(0, 32, len1, dtype=np.uint8)
        if len1 >= 31 and len2 >= 8:
            if len1 <= 33:
                pieces = [(max(0, len2 - 28), len2)]
            elif len1 <= 129:
                seam = SEAMS[len1 - 127] if SEAMS[len1 - 127] + 40 <= len2 else len2 // 2
                pieces = [(max(0, seam - 50), min(len2, seam + 50))]
            else:
                pieces = [(q * len2 // 4 + len2 // 16, min(len2, q * len2 // 4 + len2 // 16 + 44)) for q in range(4)]
            at = 2
            for lo, hi in pieces:
                piece = noisy(rng, cons[lo:hi])[:max(0, len1 - at)]
                x[at:at + len(piece)] = piece
                at += len(piece) + 2
        seqs.append((x | (rng.integers(0, 8, len1, dtype=np.uint8) << 5)).astype(np.uint8))
    return seqs


def all_len2s():
    return sorted(LEN2S + [LONG_LEN2])


def path_cells(result, k):
    """The cells (i, j) that alignment k's path enters by a diagonal move, walking back from the end cell."""
    _, ends, moves, mo, steps = result
    i, j = int(ends[k, 0]), int(ends[k, 1])
    at = int(mo[k])
    cells = []
    for t in range(int(steps[k])):
        m = int(moves[at + (t >> 5)] >> np.uint64(2 * (t & 31))) & 3
        if m == 3:
            cells.append((i, j))
        i -= m != 1
        j -= m != 2
    return cells
