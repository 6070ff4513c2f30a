"""The banded aligners on a batch of mixed (len1, len2) with the band's width per call, for sequences UP TO 65536 LONG: the
ctypes binding of libswmi_banded_long.so (include/swmi_banded_long.h).  Reached as swmi.banded_long.<name>.

The functions are swmi.banded_width's, argument for argument, and for every length up to 16384 so is every result.  What
differs: MAX_LEN; the moves are laid out by move_offsets() (swmi_banded_long_move_offsets, the running sum of
SWMI_LOCAL_LONG_MOVE_WORDS: the values of swmi.wide_long.move_offsets, without that library); and a path is expanded by
swmi.local_long.expand_moves.  A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's
current HIP device, and keeps its own workspaces and its own last error."""
import ctypes

import numpy as np

from . import ERR_NOT_INITIALIZED, SwmiError, _offsets_pair  # noqa: F401  (reachable here as in the sibling modules)
from ._banded_ragged_binding import RaggedBinding
from .local_long import expand_moves

LOCAL, GLOBAL = 0, 1          # SWMI_BANDED_LONG_LOCAL / SWMI_BANDED_LONG_GLOBAL
MAX_LEN = 65536
WIDTHS = (128, 256, 512, 1024)
SLOT_BYTES = 48               # SWMI_BANDED_LONG_SLOT_BYTES
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment (global kind)


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a mixed batch (swmi_banded_long_move_offsets; needs no device): the running sum of
    SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    out = np.zeros(len(off1), np.uint64)
    _binding.check(_binding.entry("move_offsets")(off1.ctypes.data, off2.ctypes.data, len(off1) - 1, out.ctypes.data))
    return out


_binding = RaggedBinding("swmi_banded_long", "libswmi_banded_long.so", "SWMI_BANDED_LONG_LIB", has_band=True, move_offsets=move_offsets,
                         extra={"move_offsets": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]})
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_banded_long.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_banded_long_last_error: the text of the calling thread's last failed swmi.banded_long call."""
    return _binding.last_error()


def version():
    """swmi_banded_long_version."""
    return _binding.version()


def local(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_long_local: swmi.banded_width.local for sequences of up to 65536; the arguments and the result are that
    function's, the moves laid out by move_offsets()."""
    return _binding.host(LOCAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def global_(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_long_global: swmi.banded_width.global_ for sequences of up to 65536."""
    return _binding.host(GLOBAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, diagonals=None, stream=0):
    """swmi_banded_long_local_device: swmi.banded_width.local_device for sequences of up to 65536."""
    _binding.device(LOCAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, 0, d_scores, d_ends, d_moves,
                    d_steps, diagonals, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, diagonals=None, stream=0):
    """swmi_banded_long_global_device: as local_device, under the mask free_ends."""
    _binding.device(GLOBAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                    d_moves, d_steps, diagonals, stream)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10):
    """swmi_banded_long_time_device: average ms of `iters` device calls of `kind` (LOCAL / GLOBAL) after one untimed call;
    arguments as global_device (free_ends is ignored by the local kind)."""
    return _binding.time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores,
                                d_ends, d_moves, d_steps, diagonals, stream, iters)


def slices_for(kind, band, seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call of `kind` at width `band` cuts its batch into (swmi_banded_long_slices_for; needs no device)."""
    return _binding.slices_for(kind, band, seq1_offsets, seq2_offsets, traceback)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local() or
    global_() (swmi.local_long.expand_moves); None for an infeasible alignment."""
    scores, ends, moves, mo, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else
            expand_moves(moves[int(mo[k]):int(mo[k + 1])], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_long_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
