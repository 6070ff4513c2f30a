"""The banded aligners on a batch of MIXED (len1, len2) in one call: the ctypes binding of libswmi_banded_ragged.so
(include/swmi_banded_ragged.h).  Reached as swmi.banded_ragged.<name>.

local() is swmi.banded.align and global_() is swmi.banded_global.align with a (len1, len2) and a diagonal of its own per
alignment, 0 .. 16384 each, and one matrix, one pair of gaps and (global_) one free_ends mask per call: alignment k's score,
ends, steps and moves are what the fixed entry gives for that pair alone.  A library of its own beside libswmi.so: it needs no
swmi.init(), runs on the calling thread's current HIP device, and keeps its own workspaces and its own last error.  The layout
of the moves (swmi.local_full_ragged_move_offsets) and the expander (swmi.local_full_expand_moves) are the package's.

An empty sequence: local() gives score 0, ends (0, 0, 0, 0) and no step; global_() gives what the one border the table then
consists of gives under the band and the mask, NO_ALIGNMENT where no finite candidate lies in the band."""
from . import ERR_NOT_INITIALIZED, SwmiError, local_full_expand_moves, local_full_ragged_move_offsets  # noqa: F401  (reachable here as before)
from ._banded_ragged_binding import RaggedBinding

LOCAL, GLOBAL = 0, 1          # SWMI_BANDED_RAGGED_LOCAL / SWMI_BANDED_RAGGED_GLOBAL
MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63
SLOT_BYTES = 48               # SWMI_BANDED_RAGGED_SLOT_BYTES
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment (global kind)

_binding = RaggedBinding("swmi_banded_ragged", "libswmi_banded_ragged.so", "SWMI_BANDED_RAGGED_LIB", has_band=False,
                         move_offsets=local_full_ragged_move_offsets)
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_banded_ragged.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_banded_ragged_last_error: the text of the calling thread's last failed swmi.banded_ragged call."""
    return _binding.last_error()


def version():
    """swmi_banded_ragged_version."""
    return _binding.version()


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a mixed batch: alignment k's moves start at word move_offsets[k]
    (swmi.local_full_ragged_move_offsets: there is no second function)."""
    return local_full_ragged_move_offsets(seq1_offsets, seq2_offsets)


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_ragged_local: swmi.banded.align with a (len1, len2) of its own per alignment.  seq1s and seq2s: each a list
    of 1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair; diagonals: n int32, or None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _binding.host(LOCAL, seq1s, seq2s, None, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def global_(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_ragged_global: swmi.banded_global.align on a mixed batch under the one mask free_ends (0 .. 19); arguments
    and result as local().  An infeasible alignment has score NO_ALIGNMENT, ends (0, 0, 0, 0) (ends-only (0, 0, -1, -1)) and 0
    steps."""
    return _binding.host(GLOBAL, seq1s, seq2s, None, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, diagonals=None, stream=0):
    """swmi_banded_ragged_local_device: the sequence and result buffers are device pointers (ints or torch tensors, 16-byte
    aligned); both offset arrays AND the diagonals are host arrays, read before the call returns.  Asynchronous on `stream`;
    d_moves = d_steps = None: ends-only."""
    _binding.device(LOCAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, None, score_matrix, gap_open, gap_extend, 0, d_scores, d_ends, d_moves,
                    d_steps, diagonals, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, diagonals=None, stream=0):
    """swmi_banded_ragged_global_device: as local_device, under the mask free_ends."""
    _binding.device(GLOBAL, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, None, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                    d_moves, d_steps, diagonals, stream)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10):
    """swmi_banded_ragged_time_device: average ms of `iters` device calls of `kind` (LOCAL / GLOBAL) after one untimed call;
    arguments as global_device (free_ends is ignored by the local kind)."""
    return _binding.time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, None, score_matrix, gap_open, gap_extend, free_ends, d_scores,
                                d_ends, d_moves, d_steps, diagonals, stream, iters)


def slices_for(kind, seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call of `kind` cuts its batch into (swmi_banded_ragged_slices_for; needs no device)."""
    return _binding.slices_for(kind, None, seq1_offsets, seq2_offsets, traceback)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local() or
    global_(); None for an infeasible alignment."""
    scores, ends, moves, mo, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else
            local_full_expand_moves(moves[int(mo[k]):int(mo[k + 1])], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_ragged_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
