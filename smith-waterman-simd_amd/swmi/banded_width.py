"""The banded aligners on a batch of mixed (len1, len2) with the BAND'S WIDTH per call: the ctypes binding of
libswmi_banded_width.so (include/swmi_banded_width.h).  Reached as swmi.banded_width.<name>.

The functions are swmi.banded_ragged's with one more argument, `band`, directly before score_matrix as in the C ABI: 128, 256,
512 or 1024 diagonals, cell (i, j) of alignment k being in the band iff -band/2 <= (j - i) - diagonals[k] <= band/2 - 1.  With
band = 128 every result is swmi.banded_ragged's.  A library of its own beside libswmi.so: it needs no swmi.init(), runs on the
calling thread's current HIP device, and keeps its own workspaces and its own last error."""
from . import ERR_NOT_INITIALIZED, SwmiError, local_full_expand_moves, local_full_ragged_move_offsets  # noqa: F401  (reachable here as before)
from ._banded_ragged_binding import RaggedBinding

LOCAL, GLOBAL = 0, 1          # SWMI_BANDED_WIDTH_LOCAL / SWMI_BANDED_WIDTH_GLOBAL
MAX_LEN = 16384
WIDTHS = (128, 256, 512, 1024)
SLOT_BYTES = 48               # SWMI_BANDED_WIDTH_SLOT_BYTES
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment (global kind)

_binding = RaggedBinding("swmi_banded_width", "libswmi_banded_width.so", "SWMI_BANDED_WIDTH_LIB", has_band=True,
                         move_offsets=local_full_ragged_move_offsets)
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_banded_width.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_banded_width_last_error: the text of the calling thread's last failed swmi.banded_width call."""
    return _binding.last_error()


def version():
    """swmi_banded_width_version."""
    return _binding.version()


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a mixed batch (swmi.local_full_ragged_move_offsets: there is no second function)."""
    return local_full_ragged_move_offsets(seq1_offsets, seq2_offsets)


def local(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_width_local: swmi.banded_ragged.local under a band of `band` diagonals (128, 256, 512 or 1024); the other
    arguments and the result are that function's."""
    return _binding.host(LOCAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def global_(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_width_global: swmi.banded_ragged.global_ under a band of `band` diagonals."""
    return _binding.host(GLOBAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, diagonals=None, stream=0):
    """swmi_banded_width_local_device: swmi.banded_ragged.local_device under a band of `band` diagonals."""
    _binding.device(LOCAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, 0, d_scores, d_ends, d_moves,
                    d_steps, diagonals, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, diagonals=None, stream=0):
    """swmi_banded_width_global_device: as local_device, under the mask free_ends."""
    _binding.device(GLOBAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                    d_moves, d_steps, diagonals, stream)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10):
    """swmi_banded_width_time_device: average ms of `iters` device calls of `kind` (LOCAL / GLOBAL) after one untimed call;
    arguments as global_device (free_ends is ignored by the local kind)."""
    return _binding.time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores,
                                d_ends, d_moves, d_steps, diagonals, stream, iters)


def slices_for(kind, band, seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call of `kind` at width `band` cuts its batch into (swmi_banded_width_slices_for; needs no device)."""
    return _binding.slices_for(kind, band, seq1_offsets, seq2_offsets, traceback)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local() or
    global_(); None for an infeasible alignment."""
    scores, ends, moves, mo, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else
            local_full_expand_moves(moves[int(mo[k]):int(mo[k + 1])], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_width_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
