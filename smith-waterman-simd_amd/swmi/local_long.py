"""Local (Smith-Waterman / Gotoh) alignment of two sequences of up to 65536 bases (swmi_local_long*, include/swmi.h, DESIGN.md
section 25): swmi.local_full and swmi.local_full_affine with 1 <= len1, len2 <= MAX_LEN, field for field; every int8 matrix
and gap is accepted at every shape (there is no domain rule).  Reached as swmi.local_long.<name>."""
from . import _affine, _call, _check, _expand, _linear, _move_words, _pair_batch, _slices, _table_align, _table_time, load

MAX_LEN = 65536


def move_words(len1, len2):
    """64-bit words of moves per alignment of swmi_local_long and swmi_local_long_affine (SWMI_LOCAL_LONG_MOVE_WORDS)."""
    return _move_words(len1, len2)


def local_long(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """swmi.local_full for lengths in [1, 65536] (swmi_local_long): same arguments and the same return value, (scores[n]
    int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, move_words(len1, len2)] uint64, steps[n] uint32), the
    moves in walking order from the end cell (3 diagonal, 2 up, 1 left); expand_moves rebuilds the positions.
    traceback=False: ends-only (moves and steps are None, the start cell is (-1, -1))."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_local_long, (a.ctypes.data, len1, b.ctypes.data, len2, n), _linear(score_matrix, gap_penalty), n,
                        4, (n, _move_words(len1, len2)), traceback)


def local_long_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None, d_steps=None,
                      stream=0):
    """swmi_local_long_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_long_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty), d_scores, d_ends,
          d_moves, d_steps, stream)


def local_long_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves=None, d_steps=None,
                           stream=0, iters=10):
    """Average ms of one swmi_local_long_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_long_time_device, (d_seq1s, len1, d_seq2s, len2, n), _linear(score_matrix, gap_penalty),
                       d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def local_long_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_local_long cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_long_slices_for, n, len1, len2, 1 if traceback else 0)


def local_long_release_workspaces():
    """Free the linear-gap long local aligner's device buffers on the current GPU."""
    _check(load().swmi_local_long_release_workspaces())


def local_long_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi.local_full_affine for lengths in [1, 65536] (swmi_local_long_affine): same arguments and return value as
    local_long, with (gap_open, gap_extend) for the gap, both in [0, 127]."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_local_long_affine, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _affine(score_matrix, gap_open, gap_extend), n, 4, (n, _move_words(len1, len2)), traceback)


def local_long_affine_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                             d_steps=None, stream=0):
    """swmi_local_long_affine_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_local_long_affine_device, (d_seq1s, len1, d_seq2s, len2, n), _affine(score_matrix, gap_open, gap_extend),
          d_scores, d_ends, d_moves, d_steps, stream)


def local_long_affine_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                                  d_moves=None, d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_local_long_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_local_long_affine_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_steps, stream, iters=iters)


def local_long_affine_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_local_long_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_local_long_affine_slices_for, n, len1, len2, 1 if traceback else 0)


def local_long_affine_release_workspaces():
    """Free the affine long local aligner's device buffers on the current GPU."""
    _check(load().swmi_local_long_affine_release_workspaces())


def expand_moves(moves_row, steps, end_i, end_j, cap=None):
    """One alignment's moves -> the (steps + 1, 2) int32 list of (i, j) from the start cell to the end cell
    (swmi_local_long_expand_moves: end cells up to (65536, 65536))."""
    return _expand(load().swmi_local_long_expand_moves, moves_row, steps, end_i, end_j, cap)
