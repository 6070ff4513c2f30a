"""Exact semi-global alignment on a batch of MIXED (len1, len2) in one call (swmi_semiglobal_full_ragged*,
swmi_semiglobal_full_affine_ragged*, include/swmi.h): swmi.semiglobal_full and
swmi.semiglobal_full_affine with a (len1, len2) of its own per alignment, 0 .. 16384 each, and one set of gaps per call.
Reached as swmi.semiglobal_ragged.<name>; the layout of the moves (swmi.local_full_ragged_move_offsets) and the expander
(swmi.semiglobal_expand_moves) are the package's.

An empty sequence is NOT the local aligners' "score 0 and no steps": the table is then one border whose cells are all <= 0,
(0, 0) first, so the score is 0, the best cell (0, 0), and lengths = 1 -- the path's one position."""
from . import _affine, _full_ragged_device, _linear, _offsets_pair, _ragged_pair, _slices, _table_align, load, np
from . import local_full_ragged_move_offsets


def _call(entry, seq1s, seq2s, params, traceback):
    """A host entry on fresh result arrays with TWO ends per alignment: (scores, ends[n, 2], moves flat, move_offsets, lengths)."""
    cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
    n = len(off1) - 1
    mo = local_full_ragged_move_offsets(off1, off2) if traceback else None
    if len(cat1) == 0:
        cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
    if len(cat2) == 0:
        cat2 = np.zeros(16, np.uint8)
    scores, ends, moves, lengths = _table_align(entry, (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n),
                                                params, n, 2, int(mo[-1]) if traceback else 0, traceback)
    return scores, ends, moves, mo, lengths


def semiglobal_full_ragged(seq1s, seq2s, score_matrix, gap_penalty, traceback=True):
    """swmi_semiglobal_full_ragged: swmi.semiglobal_full with a (len1, len2) of its own per alignment.  seq1s and seq2s: each a
    list of 1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair.

    Returns (scores[n] int32, ends[n, 2] int32 = the best cell, moves uint64 (flat: alignment k's at move_offsets[k] ..),
    move_offsets[n + 1], lengths[n] uint32 = steps + 1); traceback=False: moves, move_offsets and lengths are None."""
    return _call(load().swmi_semiglobal_full_ragged, seq1s, seq2s, _linear(score_matrix, gap_penalty), traceback)


def semiglobal_full_affine_ragged(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_semiglobal_full_affine_ragged: swmi.semiglobal_full_affine on a ragged batch; arguments and result as
    semiglobal_full_ragged, with (gap_open, gap_extend) for the gap."""
    return _call(load().swmi_semiglobal_full_affine_ragged, seq1s, seq2s, _affine(score_matrix, gap_open, gap_extend), traceback)


def semiglobal_full_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_penalty, d_scores, d_ends,
                                  d_moves=None, d_lengths=None, stream=0):
    """swmi_semiglobal_full_ragged_device: device pointers, both offset arrays host arrays of n + 1 (asynchronous on `stream`);
    d_ends holds two int32 per alignment; d_moves = d_lengths = None: ends-only."""
    _full_ragged_device(load().swmi_semiglobal_full_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _linear(score_matrix, gap_penalty), d_scores, d_ends, d_moves, d_lengths, stream)


def semiglobal_full_affine_ragged_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores,
                                         d_ends, d_moves=None, d_lengths=None, stream=0):
    """swmi_semiglobal_full_affine_ragged_device: as semiglobal_full_ragged_device with (gap_open, gap_extend)."""
    _full_ragged_device(load().swmi_semiglobal_full_affine_ragged_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                        _affine(score_matrix, gap_open, gap_extend), d_scores, d_ends, d_moves, d_lengths, stream)


def semiglobal_full_ragged_slices_for(seq1_offsets, seq2_offsets, affine=False, traceback=True):
    """The slices a ragged semi-global call cuts its batch into (swmi_semiglobal_full_ragged_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_semiglobal_full_ragged_slices_for, off1.ctypes.data, off2.ctypes.data, len(off1) - 1,
                   1 if affine else 0, 1 if traceback else 0)
