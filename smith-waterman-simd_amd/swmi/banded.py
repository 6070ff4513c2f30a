"""Local alignment with AFFINE gaps restricted to a BAND of 128 diagonals, with end cell, start cell and traceback or ends-only:
the ctypes binding of libswmi_banded.so (include/swmi_banded.h).  Reached as swmi.banded.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  Cell (i, j) of alignment k is in the band iff -64 <= (j - i) - diagonals[k] <= 63;
every cell outside it holds H = 0, E = F = -infinity.  1 <= len1, len2 <= 16384, one (len1, len2) per call; every int32 is a
legal diagonal.  The walk, the tie rules and the move encoding are swmi.local_full_affine's, and the expander
(swmi.local_full_expand_moves) is the package's."""
from . import ERR_NOT_INITIALIZED, SwmiError, _move_words, local_full_expand_moves  # noqa: F401  (reachable here as before)
from ._banded_binding import Binding

MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63

_binding = Binding("swmi_banded", "swmi_banded_local", "libswmi_banded.so", "SWMI_BANDED_LIB", masked=False)
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_banded.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_banded_last_error: the text of the calling thread's last failed swmi.banded call."""
    return _binding.last_error()


def version():
    """swmi_banded_version."""
    return _binding.version()


def move_words(len1, len2):
    """64-bit words of moves per alignment (SWMI_LOCAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_local: banded local alignment of n pairs.  seq1s: (n, len1) bases, seq2s: (n, len2); diagonals: n int32, or
    None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, move_words(len1, len2)] uint64,
    steps[n] uint32), as swmi.local_full_affine does; traceback=False: ends-only (moves and steps are None, the start cell is
    (-1, -1))."""
    return _binding.align(seq1s, seq2s, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def local_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, stream=None):
    """swmi_banded_local_device on torch tensors of the current device: seq1s (n, len1) and seq2s (n, len2) uint8, scores (n)
    and ends (n, 4) int32, moves (n, move_words(len1, len2)) int64 and steps (n) int32 or both None (ends-only), diagonals (n)
    int32 or None.  Asynchronous on `stream` (a torch stream or a raw handle; None: torch's current stream)."""
    _binding.align_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, 0, diagonals, stream)


def time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, stream=None,
                iters=10):
    """swmi_banded_time_device: average ms of `iters` device calls after one untimed call; arguments as local_device."""
    return _binding.time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, 0, diagonals, stream, iters)


def slices_for(n, len1, len2, traceback=True):
    """The slices swmi_banded_local cuts n alignments into (swmi_banded_slices_for; needs no device)."""
    return _binding.slices_for(n, len1, len2, traceback)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local()."""
    scores, ends, moves, steps = result
    return [local_full_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
