"""Global, fit, overlap and extension alignment with AFFINE gaps restricted to a BAND of 128 diagonals, with end cell, start cell
and traceback or ends-only: the ctypes binding of libswmi_banded_global.so (include/swmi_banded_global.h).
Reached as swmi.banded_global.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  Cell (i, j) of alignment k is in the band iff -64 <= (j - i) - diagonals[k] <= 63;
every cell outside it holds H = E = F = -infinity and there is no zero floor.  free_ends is swmi.FREE_BEGIN1 / FREE_BEGIN2 /
FREE_END1 / FREE_END2 (0 .. 15) or END_ANYWHERE with the BEGIN bits (16 .. 19).  An alignment with no finite candidate in the
band scores NO_ALIGNMENT.  1 <= len1, len2 <= 16384, one (len1, len2) per call; every int32 is a legal diagonal.  The walk, the
tie rules and the move encoding are swmi.global_full_affine's, and the expander (swmi.local_full_expand_moves) is the package's."""
from . import ERR_NOT_INITIALIZED, SwmiError, _move_words, local_full_expand_moves  # noqa: F401  (reachable here as before)
from ._banded_binding import Binding

MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE: the end cell is the best cell anywhere in the band
ENDS_EXTEND = 16              # SWMI_BANDED_ENDS_EXTEND: from (0, 0) to wherever the score peaks
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment

_binding = Binding("swmi_banded_global", "swmi_banded_global", "libswmi_banded_global.so", "SWMI_BANDED_GLOBAL_LIB", masked=True)
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_banded_global.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_banded_global_last_error: the text of the calling thread's last failed swmi.banded_global call."""
    return _binding.last_error()


def version():
    """swmi_banded_global_version."""
    return _binding.version()


def move_words(len1, len2):
    """64-bit words of moves per alignment (SWMI_LOCAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def align(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_global: banded alignment with no zero floor of n pairs under the mask free_ends.  seq1s: (n, len1) bases,
    seq2s: (n, len2); diagonals: n int32, or None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, move_words(len1, len2)] uint64,
    steps[n] uint32), as swmi.global_full_affine does; traceback=False: ends-only (moves and steps are None, the start cell is
    (-1, -1)).  An infeasible alignment has score NO_ALIGNMENT, ends (0, 0, 0, 0) (ends-only (0, 0, -1, -1)) and 0 steps."""
    return _binding.align(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def align_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, diagonals=None,
                 stream=None):
    """swmi_banded_global_device on torch tensors of the current device: seq1s (n, len1) and seq2s (n, len2) uint8, scores (n)
    and ends (n, 4) int32, moves (n, move_words(len1, len2)) int64 and steps (n) int32 or both None (ends-only), diagonals (n)
    int32 or None.  Asynchronous on `stream` (a torch stream or a raw handle; None: torch's current stream)."""
    _binding.align_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, free_ends, diagonals, stream)


def time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, diagonals=None,
                stream=None, iters=10):
    """swmi_banded_global_time_device: average ms of `iters` device calls after one untimed call; arguments as align_device."""
    return _binding.time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, free_ends, diagonals, stream,
                                iters)


def slices_for(n, len1, len2, traceback=True):
    """The slices swmi_banded_global cuts n alignments into (swmi_banded_global_slices_for; needs no device)."""
    return _binding.slices_for(n, len1, len2, traceback)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of align(); None for an
    infeasible alignment."""
    scores, ends, moves, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else local_full_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1])
            for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_global_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
