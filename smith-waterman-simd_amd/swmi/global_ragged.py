"""Global (Needleman-Wunsch / Gotoh), fit and overlap alignment on a batch of MIXED (len1, len2) in one call
(swmi_global_full_ragged*, swmi_global_full_affine_ragged*, include/swmi.h): swmi.global_full and
swmi.global_affine.global_full_affine with a (len1, len2) of its own per alignment, 0 .. 16384 each, and one mask and one set
of gaps per call.  Reached as swmi.global_ragged.<name>; the masks (swmi.ENDS_GLOBAL, swmi.ENDS_FIT, swmi.ENDS_OVERLAP,
swmi.FREE_*), the layout of the moves (swmi.local_full_ragged_move_offsets) and the expander
(swmi.local_full_expand_moves) are the package's.

An empty sequence is NOT the local aligners' "score 0": the table is then one border.  With L the other length and cost(L) =
L gap or gap_open + (L-1) gap_extend: a free end on that border gives score 0 at (0, 0); else the end cell is (L, 0) or
(0, L), with score 0 and no steps if that border's begin is free, else score -cost(L) and L forced steps to (0, 0)."""
from . import (ENDS_GLOBAL, _affine, _free_ends, _full_ragged_call, _full_ragged_device, _linear, _offsets_pair, _slices, load)


def global_full_ragged(seq1s, seq2s, score_matrix, gap_penalty, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_global_full_ragged: swmi.global_full with a (len1, len2) of its own per alignment.  seq1s and seq2s: each a list of
    1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair.

    Returns (scores[n] int32, which may be negative, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat:
    alignment k's at move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and
    steps are None and the start cell is (-1, -1)."""
    return _full_ragged_call(load().swmi_global_full_ragged, seq1s, seq2s, _linear(score_matrix, gap_penalty, _free_ends(free_ends)),
                             traceback)


def global_full_affine_ragged(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_global_full_affine_ragged: swmi.global_affine.global_full_affine on a ragged batch; arguments and result as
    global_full_ragged, with (gap_open, gap_extend) for the gap."""
    return _full_ragged_call(load().swmi_global_full_affine_ragged, seq1s, seq2s,
                             _affine(score_matrix, gap_open, gap_extend) + (_free_ends(free_ends),), traceback)


def global_full_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_penalty, free_ends, d_scores, d_ends,
                              d_moves=None, d_steps=None, stream=0):
    """swmi_global_full_ragged_device: device pointers, both offset arrays host arrays of n + 1 (asynchronous on `stream`);
    d_moves = d_steps = None: ends-only."""
    _full_ragged_device(load().swmi_global_full_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _linear(score_matrix, gap_penalty, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream)


def global_full_affine_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends,
                                     d_scores, d_ends, d_moves=None, d_steps=None, stream=0):
    """swmi_global_full_affine_ragged_device: as global_full_ragged_device with (gap_open, gap_extend)."""
    _full_ragged_device(load().swmi_global_full_affine_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _affine(score_matrix, gap_open, gap_extend) + (_free_ends(free_ends),), d_scores, d_ends, d_moves, d_steps,
                        stream)


def global_full_ragged_slices_for(seq1_offsets, seq2_offsets, affine=False, traceback=True):
    """The slices a ragged global call cuts its batch into (swmi_global_full_ragged_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_global_full_ragged_slices_for, off1.ctypes.data, off2.ctypes.data, len(off1) - 1, 1 if affine else 0,
                   1 if traceback else 0)
