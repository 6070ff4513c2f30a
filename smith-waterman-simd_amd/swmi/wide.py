"""Local and global / fit / overlap alignment with affine gaps over an alphabet of 32 LETTERS and a caller-supplied 32 x 32
int8 matrix, on a batch of MIXED (len1, len2): the ctypes binding of libswmi_wide.so (include/swmi_wide.h, DESIGN.md section
29).  Reached as swmi.wide.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  The semantics are swmi.local_full_affine_ragged's and
swmi.global_ragged.global_full_affine_ragged's, with the score of cell (i, j) = score_matrix[(seq1[i-1] & 31) * 32 +
(seq2[j-1] & 31)].  0 <= len1 <= 16384, 0 <= len2 <= 4096: put the shorter sequence second.  The masks (swmi.ENDS_*,
swmi.FREE_*), the layout of the moves (swmi.local_full_ragged_move_offsets) and the expander (swmi.local_full_expand_moves)
are the package's.  No substitution table is shipped: pass your own."""
import numpy as np

from . import (ENDS_GLOBAL, ERR_DOMAIN, ERR_NOT_INITIALIZED, SwmiError, _affine_gap, _free_ends,  # noqa: F401  (reachable here as before)
               local_full_ragged_move_offsets)
from ._wide_binding import WideBinding

LETTERS = 32
MAX_LEN1 = 16384
MAX_LEN2 = 4096
LOCAL, GLOBAL = 0, 1

_binding = WideBinding("swmi_wide", "libswmi_wide.so", "SWMI_WIDE_LIB", local_full_ragged_move_offsets)
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_wide.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_wide_last_error: the text of the calling thread's last failed swmi.wide call."""
    return _binding.last_error()


def version():
    """swmi_wide_version."""
    return _binding.version()


def _sm(score_matrix):
    raw = np.asarray(score_matrix).reshape(-1)
    if raw.size != LETTERS * LETTERS:
        raise ValueError("score_matrix must have 1024 entries")
    if raw.dtype != np.int8 and (raw.min() < -128 or raw.max() > 127):   # the cast below would wrap silently
        raise SwmiError(ERR_DOMAIN, "score_matrix entries must lie in [-128, 127] (got %d..%d)" % (raw.min(), raw.max()))
    return np.ascontiguousarray(raw, dtype=np.int8)


def _params(score_matrix, gap_open, gap_extend, *mask):
    """(matrix, gap_open, gap_extend[, mask]), checked for what ctypes would wrap."""
    return (_sm(score_matrix), _affine_gap("gap_open", gap_open), _affine_gap("gap_extend", gap_extend)) + mask


def match_matrix(match, mismatch):
    """32 x 32 matrix (flat, 1024 int8) with `match` on the diagonal and `mismatch` elsewhere."""
    sm = np.full((LETTERS, LETTERS), mismatch, np.int8)
    np.fill_diagonal(sm, match)
    return sm.reshape(-1)


def embed_dna(sm16):
    """A 4 x 4 matrix of the 4-letter aligners in the top-left corner of a 32 x 32 one (flat, 1024 int8), -128 elsewhere: on
    sequences of letters 0 .. 3 the wide aligners then compute what the 4-letter ones do."""
    raw = np.asarray(sm16).reshape(-1)
    if raw.size != 16:
        raise ValueError("sm16 must have 16 entries")
    if raw.dtype != np.int8 and (raw.min() < -128 or raw.max() > 127):
        raise SwmiError(ERR_DOMAIN, "score_matrix entries must lie in [-128, 127] (got %d..%d)" % (raw.min(), raw.max()))
    sm = np.full((LETTERS, LETTERS), -128, np.int8)
    sm[:4, :4] = raw.astype(np.int8).reshape(4, 4)
    return sm.reshape(-1)


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_wide_local: local alignment (Smith-Waterman / Gotoh, zero floor) over 32 letters.  seq1s and seq2s: each a list of
    1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair; score_matrix: 1024 int8, row = seq1's letter.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _binding.host("local", seq1s, seq2s, _params(score_matrix, gap_open, gap_extend), traceback)


def global_(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_wide_global: global / fit / overlap alignment (free_ends: a mask of swmi.FREE_*) over 32 letters; arguments and
    result as local(), with scores that may be negative."""
    return _binding.host("global", seq1s, seq2s, _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), traceback)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, stream=0):
    """swmi_wide_local_device: device pointers of the current device, both offset arrays host arrays of n + 1 (asynchronous on
    `stream`); d_moves = d_steps = None: ends-only."""
    _binding.device("local_device", d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, _params(score_matrix, gap_open, gap_extend),
                    d_scores, d_ends, d_moves, d_steps, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, stream=0):
    """swmi_wide_global_device: as local_device with the mask."""
    _binding.device("global_device", d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                    _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream)


def slices_for(seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call cuts its batch into (swmi_wide_slices_for; needs no device)."""
    return _binding.slices_for(seq1_offsets, seq2_offsets, traceback)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, stream=0, iters=10):
    """swmi_wide_time_device: average ms of `iters` device calls of kind LOCAL or GLOBAL, after one untimed call."""
    return _binding.time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                                _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps,
                                stream, iters=iters)


def release_workspaces():
    """swmi_wide_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
