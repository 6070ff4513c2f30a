"""Global (Needleman-Wunsch / Gotoh), fit and overlap alignment with AFFINE gaps of two sequences of any length
(swmi_global_full_affine*, include/swmi.h): swmi.global_full with a gap of length k costing
gap_open + (k-1) gap_extend.  Reached as swmi.global_affine.<name>; the masks (swmi.ENDS_GLOBAL, swmi.ENDS_FIT,
swmi.ENDS_OVERLAP, swmi.FREE_*), the move-word count (swmi.global_full_move_words) and the expander
(swmi.local_full_expand_moves) are the package's."""
from . import ENDS_GLOBAL, _affine, _call, _check, _free_ends, _move_words, _pair_batch, _slices, _table_align, _table_time, load


def _params(score_matrix, gap_open, gap_extend, free_ends):
    """`params` of the affine global aligner, checked: (matrix, gap_open, gap_extend, mask)."""
    return _affine(score_matrix, gap_open, gap_extend) + (_free_ends(free_ends),)


def global_full_affine(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """Global and free-end-gap alignment with affine gaps of two sequences of any length in [1, 16384], with end cell, start
    cell and traceback (swmi_global_full_affine): swmi.global_full with a gap of length k costing gap_open + (k-1) gap_extend,
    both in [0, 127].  Same arguments and return value as swmi.global_full, with (gap_open, gap_extend) for the gap:
    (scores[n] int32, which may be negative, ends[n, 4] int32 = (end_i, end_j, start_i, start_j),
    moves[n, swmi.global_full_move_words(len1, len2)] uint64, steps[n] uint32), the moves in walking order from the end cell
    (3 diagonal, 2 up, 1 left), forced moves along a border that is not free included; swmi.local_full_expand_moves rebuilds
    the positions.  With gap_open == gap_extend every field equals swmi.global_full's.  traceback=False: ends-only (moves and
    steps are None, the start cell is (-1, -1))."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    return _table_align(load().swmi_global_full_affine, (a.ctypes.data, len1, b.ctypes.data, len2, n),
                        _params(score_matrix, gap_open, gap_extend, free_ends), n, 4, (n, _move_words(len1, len2)), traceback)


def global_full_affine_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                              d_moves=None, d_steps=None, stream=0):
    """swmi_global_full_affine_device on device pointers (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _call(load().swmi_global_full_affine_device, (d_seq1s, len1, d_seq2s, len2, n),
          _params(score_matrix, gap_open, gap_extend, free_ends), d_scores, d_ends, d_moves, d_steps, stream)


def global_full_affine_time_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_open, gap_extend, free_ends, d_scores,
                                   d_ends, d_moves=None, d_steps=None, stream=0, iters=10):
    """Average ms of one swmi_global_full_affine_device call over `iters` back-to-back calls (HIP events on `stream`)."""
    return _table_time(load().swmi_global_full_affine_time_device, (d_seq1s, len1, d_seq2s, len2, n),
                       _params(score_matrix, gap_open, gap_extend, free_ends), d_scores, d_ends, d_moves, d_steps, stream,
                       iters=iters)


def global_full_affine_slices_for(n, len1, len2, traceback=True):
    """The slices swmi_global_full_affine cuts n alignments into (needs no device)."""
    return _slices(load().swmi_global_full_affine_slices_for, n, len1, len2, 1 if traceback else 0)


def global_full_affine_release_workspaces():
    """Free the affine global aligner's device buffers on the current GPU."""
    _check(load().swmi_global_full_affine_release_workspaces())
