"""Local alignment with AFFINE gaps restricted to a BAND of 128 diagonals, with end cell, start cell and traceback or ends-only:
the ctypes binding of libswmi_banded.so (include/swmi_banded.h).  Reached as swmi.banded.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  Cell (i, j) of alignment k is in the band iff -64 <= (j - i) - diagonals[k] <= 63;
every cell outside it holds H = 0, E = F = -infinity.  1 <= len1, len2 <= 16384, one (len1, len2) per call; every int32 is a
legal diagonal.  The walk, the tie rules and the move encoding are swmi.local_full_affine's, and the expander
(swmi.local_full_expand_moves) is the package's."""
import ctypes
import os

import numpy as np

from . import ERR_NOT_INITIALIZED, SwmiError, _affine, _move_words, _pair_batch, _ptr, _slices, local_full_expand_moves
from . import load as _load_swmi

MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_BANDED_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_banded.so"))

_lib = None


def load():
    """dlopen libswmi_banded.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _load_swmi()            # libswmi.so, which the library links
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.swmi_banded_last_error.restype = ctypes.c_char_p
    lib.swmi_banded_local.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, vp, vp, vp, vp]
    lib.swmi_banded_local_device.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.swmi_banded_slices_for.argtypes = [sz, sz, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_banded_slices_for.restype = sz
    lib.swmi_banded_time_device.argtypes = [vp, sz, vp, sz, sz, vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, ctypes.POINTER(ctypes.c_float)]
    _lib = lib
    return lib


def last_error():
    """swmi_banded_last_error: the text of the calling thread's last failed swmi.banded call."""
    return load().swmi_banded_last_error().decode()


def version():
    """swmi_banded_version."""
    return int(load().swmi_banded_version())


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, last_error())
    return rc


def move_words(len1, len2):
    """64-bit words of moves per alignment (SWMI_LOCAL_FULL_MOVE_WORDS)."""
    return _move_words(len1, len2)


def _diagonals(diagonals, n):
    """int32[n] or None; a value outside int32 raises instead of wrapping."""
    if diagonals is None:
        return None
    d = np.asarray(diagonals)
    if d.shape != (n,):
        raise ValueError("diagonals must hold one entry per alignment")
    if d.size and d.dtype != np.int32 and (d.min() < -2**31 or d.max() > 2**31 - 1):
        raise ValueError("diagonals must be int32")
    return np.ascontiguousarray(d, dtype=np.int32)


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_local: banded local alignment of n pairs.  seq1s: (n, len1) bases, seq2s: (n, len2); diagonals: n int32, or
    None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves[n, move_words(len1, len2)] uint64,
    steps[n] uint32), as swmi.local_full_affine does; traceback=False: ends-only (moves and steps are None, the start cell is
    (-1, -1))."""
    a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
    d = _diagonals(diagonals, n)
    params = _affine(score_matrix, gap_open, gap_extend)
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    moves = np.zeros((n, _move_words(len1, len2)), np.uint64) if traceback else None
    steps = np.zeros(n, np.uint32) if traceback else None
    _check(load().swmi_banded_local(a.ctypes.data, len1, b.ctypes.data, len2, n, _ptr(d), params[0].ctypes.data, params[1], params[2],
                                    scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))
    return scores, ends, moves, steps


def _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps):
    """The shape and the data pointers of a device call's torch tensors, checked for dtype, layout and size."""
    import torch
    if seq1s.dim() != 2 or seq2s.dim() != 2 or seq1s.shape[0] != seq2s.shape[0]:
        raise ValueError("seq1s and seq2s must be (n, len1) and (n, len2)")
    n, len1 = seq1s.shape
    len2 = seq2s.shape[1]
    want = [("seq1s", seq1s, torch.uint8, n * len1), ("seq2s", seq2s, torch.uint8, n * len2), ("scores", scores, torch.int32, n),
            ("ends", ends, torch.int32, 4 * n)]
    if diagonals is not None:
        want.append(("diagonals", diagonals, torch.int32, n))
    if moves is not None or steps is not None:
        if moves is None or steps is None:
            raise ValueError("moves and steps must both be given or both be None")
        if moves.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
            raise ValueError("moves must be int64 or uint64")
        want += [("moves", moves, moves.dtype, n * _move_words(len1, len2)), ("steps", steps, steps.dtype, n)]
        if steps.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise ValueError("steps must be int32 or uint32")
    for name, t, dtype, count in want:
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() != count:
            raise ValueError("%s must be a contiguous device tensor of %d %s" % (name, count, dtype))
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return (p(seq1s), len1, p(seq2s), len2, n, p(diagonals)), (p(scores), p(ends), p(moves), p(steps))


def local_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, stream=None):
    """swmi_banded_local_device on torch tensors of the current device: seq1s (n, len1) and seq2s (n, len2) uint8, scores (n)
    and ends (n, 4) int32, moves (n, move_words(len1, len2)) int64 and steps (n) int32 or both None (ends-only), diagonals (n)
    int32 or None.  Asynchronous on `stream` (a torch stream or a raw handle; None: torch's current stream)."""
    import torch
    shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
    params = _affine(score_matrix, gap_open, gap_extend)
    if stream is None:
        stream = torch.cuda.current_stream(seq1s.device)
    handle = getattr(stream, "cuda_stream", stream)
    _check(load().swmi_banded_local_device(*shape, params[0].ctypes.data, params[1], params[2], *out, handle))


def time_device(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, stream=None,
                iters=10):
    """swmi_banded_time_device: average ms of `iters` device calls after one untimed call; arguments as local_device."""
    import torch
    shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
    params = _affine(score_matrix, gap_open, gap_extend)
    if stream is None:
        stream = torch.cuda.current_stream(seq1s.device)
    handle = getattr(stream, "cuda_stream", stream)
    ms = ctypes.c_float()
    _check(load().swmi_banded_time_device(*shape, params[0].ctypes.data, params[1], params[2], *out, handle, int(iters), ctypes.byref(ms)))
    return float(ms.value)


def slices_for(n, len1, len2, traceback=True):
    """The slices swmi_banded_local cuts n alignments into (swmi_banded_slices_for; needs no device)."""
    return _slices(load().swmi_banded_slices_for, int(n), int(len1), int(len2), 1 if traceback else 0)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local()."""
    scores, ends, moves, steps = result
    return [local_full_expand_moves(moves[k], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_banded_release_workspaces())
