"""The wide-alphabet aligners (32 letters, a caller-supplied 32 x 32 int8 matrix, affine gaps, local and global / fit / overlap,
MIXED (len1, len2)) for sequences of up to 65536 letters in BOTH places: the ctypes binding of libswmi_wide_long.so
(include/swmi_wide_long.h).  Reached as swmi.wide_long.<name>.

A library of its own beside libswmi.so and libswmi_wide.so: it needs no swmi.init(), runs on the calling thread's current HIP
device, and keeps its own workspaces and its own last error.  The semantics and the call shapes are swmi.wide's, field for
field; on swmi.wide's shapes (len1 <= 16384, len2 <= 4096) the very same kernels run.  The global kind has the domain rule
P (len1 + len2) <= 2^23, P = max(1, max |score_matrix|, gap_open, gap_extend); the local kind has none.  The moves are laid out
by move_offsets() (swmi_wide_long_move_offsets) and a path is expanded by swmi.local_long.expand_moves.  match_matrix and
embed_dna are swmi.wide's."""
import ctypes

import numpy as np

from . import ENDS_GLOBAL, ERR_NOT_INITIALIZED, SwmiError, _free_ends, _offsets_pair  # noqa: F401  (reachable here as before)
from ._wide_binding import WideBinding
from .wide import _params, embed_dna, match_matrix  # noqa: F401  (the matrices are swmi.wide's, not copies)

MAX_LEN = 65536
LOCAL, GLOBAL = 0, 1
STRIPE_WAVES = (1, 4)


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a batch (swmi_wide_long_move_offsets; needs no device): the running sum of
    SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    out = np.zeros(len(off1), np.uint64)
    _binding.check(_binding.entry("move_offsets")(off1.ctypes.data, off2.ctypes.data, len(off1) - 1, out.ctypes.data))
    return out


_binding = WideBinding("swmi_wide_long", "libswmi_wide_long.so", "SWMI_WIDE_LONG_LIB", move_offsets,
                       extra={"set_stripe_waves": [ctypes.c_int],
                              "move_offsets": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]})
LIB_PATH = _binding.lib_path


def load():
    """dlopen libswmi_wide_long.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _binding.load()


def last_error():
    """swmi_wide_long_last_error: the text of the calling thread's last failed swmi.wide_long call."""
    return _binding.last_error()


def version():
    """swmi_wide_long_version."""
    return _binding.version()


def set_stripe_waves(waves):
    """swmi_wide_long_set_stripe_waves: the stripe width of the process's later calls, 1 or 4 wavefronts of 1024 columns,
    or 0 for the library's own rule (the default).  Results do not depend on it."""
    _binding.check(_binding.entry("set_stripe_waves")(int(waves)))


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_wide_long_local: swmi.wide.local for 0 <= len1, len2 <= 65536.  seq1s and seq2s: each a list of 1-D uint8 arrays,
    or a (concatenated, offsets[n + 1]) pair; score_matrix: 1024 int8, row = seq1's letter.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _binding.host("local", seq1s, seq2s, _params(score_matrix, gap_open, gap_extend), traceback)


def global_(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_wide_long_global: swmi.wide.global_ for 0 <= len1, len2 <= 65536, under the domain rule P (len1 + len2) <= 2^23;
    arguments and result as local(), with scores that may be negative."""
    return _binding.host("global", seq1s, seq2s, _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), traceback)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, stream=0):
    """swmi_wide_long_local_device: device pointers of the current device, both offset arrays host arrays of n + 1
    (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _binding.device("local_device", d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, _params(score_matrix, gap_open, gap_extend),
                    d_scores, d_ends, d_moves, d_steps, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, stream=0):
    """swmi_wide_long_global_device: as local_device with the mask."""
    _binding.device("global_device", d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                    _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream)


def slices_for(seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call cuts its batch into (swmi_wide_long_slices_for; needs no device)."""
    return _binding.slices_for(seq1_offsets, seq2_offsets, traceback)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, stream=0, iters=10):
    """swmi_wide_long_time_device: average ms of `iters` device calls of kind LOCAL or GLOBAL, after one untimed call."""
    return _binding.time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
                                _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps,
                                stream, iters=iters)


def release_workspaces():
    """swmi_wide_long_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _binding.release_workspaces()
