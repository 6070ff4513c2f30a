"""Global, fit, overlap and extension alignment with AFFINE gaps restricted to a BAND of 128 diagonals, with end cell, start cell
and traceback or ends-only: the ctypes binding of libswmi_banded_global.so (include/swmi_banded_global.h).
Reached as swmi.banded_global.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  Cell (i, j) of alignment k is in the band iff -64 <= (j - i) - diagonals[k] <= 63;
every cell outside it holds H = E = F = -infinity and there is no zero floor.  free_ends is swmi.FREE_BEGIN1 / FREE_BEGIN2 /
FREE_END1 / FREE_END2 (0 .. 15) or END_ANYWHERE with the BEGIN bits (16 .. 19).  An alignment with no finite candidate in the
band scores NO_ALIGNMENT.  1 <= len1, len2 <= 16384, one (len1, len2) per call; every int32 is a legal diagonal.  The walk, the
tie rules and the move encoding are swmi.global_full_affine's, and the expander (swmi.local_full_expand_moves) is the package's."""
import ctypes
import os

import numpy as np

from . import ERR_NOT_INITIALIZED, SwmiError, _affine, _free_ends, _move_words, _pair_batch, _ptr, _slices, local_full_expand_moves
from . import load as _load_swmi
from .banded import _device_args, _diagonals

MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE: the end cell is the best cell anywhere in the band
ENDS_EXTEND = 16              # SWMI_BANDED_ENDS_EXTEND: from (0, 0) to wherever the score peaks
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_BANDED_GLOBAL_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_banded_global.so"))

_lib = None


def load():
    """dlopen libswmi_banded_global.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _load_swmi()            # libswmi.so, which the library links
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    lib.swmi_banded_global_last_error.restype = ctypes.c_char_p
    lib.swmi_banded_global.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, cu, vp, vp, vp, vp]
    lib.swmi_banded_global_device.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, cu, vp, vp, vp, vp, vp]
    lib.swmi_banded_global_slices_for.argtypes = [sz, sz, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_banded_global_slices_for.restype = sz
    lib.swmi_banded_global_time_device.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, cu, vp, vp, vp, vp, vp, ci,
                                                   ctypes.POINTER(ctypes.c_float)]
    _lib = lib
    return lib


def last_error():
    """swmi_banded_global_last_error: the text of the calling thread's last failed swmi.banded_global call."""
    return load().swmi_banded_global_last_error().decode()


def version():
    """swmi_banded_global_version."""
    return int(load().swmi_banded_global_version())


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, last_error())
    return rc


def move_words(len1, len2):
    """64-bit words of moves per alignment (SWMI_LOCAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def align(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_global: banded alignment with no zero floor of n pairs under the mask free_ends.  seq1s: (n, len1) bases,
    seq2s: (n, len2); diagonals: n int32, or None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, move_words(len1, len2)] uint64,
    steps[n] uint32), as swmi.global_full_affine does; traceback=False: ends-only (moves and steps are None, the start cell is
    (-1, -1)).  An infeasible alignment has score NO_ALIGNMENT, ends (0, 0, 0, 0) (ends-only (0, 0, -1, -1)) and 0 steps."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    d = _diagonals(diagonals, n)
    params = _affine(score_matrix, gap_open, gap_extend)
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    moves = np.zeros((n, _move_words(len1, len2)), np.uint64) if traceback else None
    steps = np.zeros(n, np.uint32) if traceback else None
    _check(load().swmi_banded_global(a.ctypes.data, len1, b.ctypes.data, len2, n, _ptr(d), params[0].ctypes.data, params[1], params[2],
                                     _free_ends(free_ends), scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))
    return scores, ends, moves, steps


def _stream_handle(stream, tensor):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(tensor.device)
    return getattr(stream, "cuda_stream", stream)


def align_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, diagonals=None,
                 stream=None):
    """swmi_banded_global_device on torch tensors of the current device: seq1s (n, len1) and seq2s (n, len2) uint8, scores (n)
    and ends (n, 4) int32, moves (n, move_words(len1, len2)) int64 and steps (n) int32 or both None (ends-only), diagonals (n)
    int32 or None.  Asynchronous on `stream` (a torch stream or a raw handle; None: torch's current stream)."""
    shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
    params = _affine(score_matrix, gap_open, gap_extend)
    _check(load().swmi_banded_global_device(*shape, params[0].ctypes.data, params[1], params[2], _free_ends(free_ends), *out,
                                            _stream_handle(stream, seq1s)))


def time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, diagonals=None,
                stream=None, iters=10):
    """swmi_banded_global_time_device: average ms of `iters` device calls after one untimed call; arguments as align_device."""
    shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
    params = _affine(score_matrix, gap_open, gap_extend)
    ms = ctypes.c_float()
    _check(load().swmi_banded_global_time_device(*shape, params[0].ctypes.data, params[1], params[2], _free_ends(free_ends), *out,
                                                 _stream_handle(stream, seq1s), int(iters), ctypes.byref(ms)))
    return float(ms.value)


def slices_for(n, len1, len2, traceback=True):
    """The slices swmi_banded_global cuts n alignments into (swmi_banded_global_slices_for; needs no device)."""
    return _slices(load().swmi_banded_global_slices_for, int(n), int(len1), int(len2), 1 if traceback else 0)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of align(); None for an
    infeasible alignment."""
    scores, ends, moves, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else local_full_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1])
            for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_global_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_banded_global_release_workspaces())
