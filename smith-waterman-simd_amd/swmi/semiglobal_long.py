"""Exact semi-global alignment of two sequences of up to 65536 bases (swmi_semiglobal_long*, include/swmi.h, DESIGN.md section
26): swmi.semiglobal_full and swmi.semiglobal_full_affine with 1 <= len1, len2 <= MAX_LEN, field for field.  H is not floored,
so a call is accepted iff max(1, max |score_matrix|, gaps) * (len1 + len2) <= 2**23: every shape up to 32768 x 32768 with any
int8 parameters, 65536 x 65536 with magnitudes <= 64.  Reached as swmi.semiglobal_long.<name>."""
import numpy as np

from . import _affine, _call, _check, _linear, _move_words, _pair_batch, _slices, _table_align, _table_time, load

MAX_LEN = 65536
MAX_TRACEBACK = 131073


def move_words(len1, len2):
    """64-bit words of moves per alignment of swmi_semiglobal_long and swmi_semiglobal_long_affine
    (SWMI_SEMIGLOBAL_LONG_MOVE_WORDS)."""
    return _move_words(len1, len2)


def semiglobal_long(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """swmi.semiglobal_full for lengths in [1, 65536] (swmi_semiglobal_long): same arguments and the same return value,
    (scores[n] int32, ends[n, 2] int32 = the best cell, moves[n, move_words(len1, len2)] uint64, lengths[n] uint32), the moves
    in walking order from the best cell to (0, 0) (3 diagonal, 2 up, 1 left), lengths = steps + 1; expand_moves rebuilds the
    positions.  traceback=False: ends-only (moves and lengths are None)."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_semiglobal_long, (a.ctypes.data, len1, b.ctypes.data, len2, n), _linear(score_matrix, gap_penalty),
                        n, 2, (n, _move_words(len1, len2)), traceback)


def semiglobal_long_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                           d_lengths=None, stream=0):
    """swmi_semiglobal_long_device on device pointers (asynchronous on `stream`); d_moves = d_lengths = None: ends-only."""
    _call(load().swmi_semiglobal_long_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty), d_scores, d_ends,
          d_moves, d_lengths, stream)


def semiglobal_long_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None,
                                d_lengths=None, stream=0, iters=10):
    """Average ms of one swmi_semiglobal_long_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_semiglobal_long_time_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty),
                       d_scores, d_ends, d_moves, d_lengths, stream, iters=iters)


def semiglobal_long_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_semiglobal_long cuts n alignments into (needs no device)."""
    return _slices(load().swmi_semiglobal_long_slices_for, n, len1, len2, 1 if traceback else 0)


def semiglobal_long_release_workspaces():
    """Free the linear-gap long semi-global aligner's device buffers on the current GPU."""
    _check(load().swmi_semiglobal_long_release_workspaces())


def semiglobal_long_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi.semiglobal_full_affine for lengths in [1, 65536] (swmi_semiglobal_long_affine): same arguments and return value as
    semiglobal_long, with (gap_open, gap_extend) for the gap, both in [0, 127]."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_semiglobal_long_affine, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _affine(score_matrix, gap_open, gap_extend), n, 2, (n, _move_words(len1, len2)), traceback)


def semiglobal_long_affine_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                  d_moves=None, d_lengths=None, stream=0):
    """swmi_semiglobal_long_affine_device on device pointers (asynchronous on `stream`); d_moves = d_lengths = None: ends-only."""
    _call(load().swmi_semiglobal_long_affine_device, (d_seq1s, len1, d_seq2s, len2, n), _affine(score_matrix, gap_open, gap_extend),
          d_scores, d_ends, d_moves, d_lengths, stream)


def semiglobal_long_affine_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                       d_moves=None, d_lengths=None, stream=0, iters=10):
    """Average ms of one swmi_semiglobal_long_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_semiglobal_long_affine_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_lengths, stream, iters=iters)


def semiglobal_long_affine_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_semiglobal_long_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_semiglobal_long_affine_slices_for, n, len1, len2, 1 if traceback else 0)


def semiglobal_long_affine_release_workspaces():
    """Free the affine long semi-global aligner's device buffers on the current GPU."""
    _check(load().swmi_semiglobal_long_affine_release_workspaces())


def expand_moves(moves_row, length, cap=None):
    """One alignment's moves -> the (length, 2) int32 list of (i, j) from (0, 0) to the best cell
    (swmi_semiglobal_long_expand_moves: lengths up to 131073)."""
    row = np.ascontiguousarray(moves_row, dtype=np.uint64)
    cap = int(length) if cap is None else int(cap)
    tb = np.zeros((min(int(length), cap), 2), np.int32)
    _check(load().swmi_semiglobal_long_expand_moves(row.ctypes.data, int(length), tb.ctypes.data, cap))
    return tb
