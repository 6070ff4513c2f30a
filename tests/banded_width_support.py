"""Helpers of the width-per-call banded aligners' tests (test_banded_width_cpu.py, test_banded_width_gpu.py): the two existing C
restatements, tests/native/banded_align_oracle.c and tests/native/banded_global_oracle.c, called once per alignment with
lo = -band / 2 and hi = band / 2 - 1 (both already take lo and hi; banded_ragged_support.RaggedOracle has 128 built in and stays
as it is); the slice arithmetic of include/swmi_banded_width.h; and the drift family of DESIGN.md section 38.  There is no
restatement of the recurrences here."""
import numpy as np

from banded_ragged_support import (ALL_MASKS, EO_BUDGET, FORMS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_SLICE, NO_ALIGNMENT,  # noqa: F401
                                   SLOT_BYTES, TB_BUDGET, Batch, RaggedOracle, assert_same, move_words, moves_of, path_from, permuted,
                                   related_batch, related_pairs)

WIDTHS = (128, 256, 512, 1024)


def unbounded_for(batch):
    """a width for the restatements at which the band holds every cell of every table of `batch` (diagonals 0): the smallest
    power of two whose half exceeds the longest sequence"""
    top = max([1] + [max(len(a), len(b)) for a, b in zip(batch.seq1s, batch.seq2s)])
    assert batch.diagonals is None or not np.any(batch.diagonals)
    return 1 << (int(top).bit_length() + 1)


class WidthOracle(RaggedOracle):
    def align(self, kind, batch, band, sm, gap_open, gap_extend, free_ends=0, traceback=True):
        """(scores, ends[n, 4], moves flat, steps): one call of the kind's single-alignment restatement per alignment, the band
        -band / 2 .. band / 2 - 1 around its diagonal."""
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
            head = ((a if len(a) else pad).ctypes.data, len(a), (b if len(b) else pad).ctypes.data, len(b), d, -(band // 2), band // 2 - 1,
                    m.ctypes.data, int(gap_open), int(gap_extend))
            tail = (scores[k:].ctypes.data, ends[k:].ctypes.data, moves[int(batch.move_offsets[k]):].ctypes.data if traceback else None,
                    steps[k:].ctypes.data if traceback else None)
            if kind == GLOBAL:
                rc = self.lib.banded_global_oracle(*head, int(free_ends), *tail)
            else:
                rc = self.lib.banded_align_oracle(*head, *tail)
            assert rc == 0
        return scores, ends, None if moves is None else moves[:-1], steps


def code_bytes(kind, len1, band):
    """bytes of codes one alignment of a traceback launch takes: band / 128 bytes per lane and iteration, 64 lanes, whole trips
    of four iterations; len1 + 63 iterations for the local kind, len1 + 64 for the global kind (row 0 is swept)"""
    return (band // 128) * 256 * (-(-(len1 + (64 if kind == GLOBAL else 63)) // 4))


def per_alignment(kind, len1, len2, band, traceback):
    """device bytes one alignment of a slice takes (the header's arithmetic)"""
    per = len1 + len2 + SLOT_BYTES + 20
    if traceback:
        per += code_bytes(kind, len1, band) + 8 * move_words(len1, len2) + 4
    return per


def slices_by_hand(kind, shapes, band, traceback):
    """the header's slices, recomputed: longest runs in caller order within the byte budget, at most 2^20 alignments, at least one"""
    cap = TB_BUDGET if traceback else EO_BUDGET
    out, bytes_, m = [], 0, 0
    for len1, len2 in shapes:
        b = per_alignment(kind, len1, len2, band, traceback)
        if m and (bytes_ + b > cap or m == MAX_SLICE):
            out.append(m)
            bytes_, m = 0, 0
        bytes_ += b
        m += 1
    if m:
        out.append(m)
    return out


def drift_pair(rng, length, runs, run, sub=0.08):
    """One pair: seq1 of `length` bases, seq2 = seq1 with `sub` substitutions and `runs` runs of `run` random bases inserted at
    evenly spread places.  With diagonals = 0 the path ends runs * run diagonals above where it starts.  Both sequences keep all
    `length` related bases, so the whole path pays as long as a run costs less than the stretch beside it gains."""
    a = rng.integers(0, 4, length, dtype=np.uint8)
    b = np.where(rng.random(length) < sub, rng.integers(0, 4, length, dtype=np.uint8), a).astype(np.uint8)
    pieces, at = [], 0
    for k in range(runs):
        cut = (k + 1) * length // (runs + 1)
        pieces += [b[at:cut], rng.integers(0, 4, run, dtype=np.uint8)]
        at = cut
    pieces.append(b[at:])
    return a, np.concatenate(pieces)


def drift_batch(rng, n, length, runs, run):
    """n pairs, the runs inserted into seq2 (even k: the path drifts to higher diagonals) and into seq1 (odd k: to lower ones)
    in turn"""
    pairs = [drift_pair(rng, length, runs, run)[::1 if k % 2 == 0 else -1] for k in range(n)]
    return Batch([p[0] for p in pairs], [p[1] for p in pairs], np.zeros(n, np.int32))


def differs(x, y):
    """per alignment: any field or step count of two results differs"""
    return (x[0] != y[0]) | (x[1] != y[1]).any(axis=1) | (x[3] != y[3])
