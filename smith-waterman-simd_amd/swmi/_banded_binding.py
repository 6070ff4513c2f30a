"""The one ctypes binding body of the two banded libraries: swmi.banded (libswmi_banded.so) and
swmi.banded_global (libswmi_banded_global.so) each hold a Binding and their public functions call it.  The libraries' entries
differ by their prefix, the name of the aligning entry and one argument: the global library's take free_ends behind the gaps."""
import ctypes

import numpy as np

from . import _affine, _free_ends, _move_words, _pair_batch, _ptr, _slices
from ._library import Library


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


def _stream_handle(stream, tensor):
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(tensor.device)
    return getattr(stream, "cuda_stream", stream)


class Binding(Library):
    """One banded library: its entries are `prefix`_<name> and `align_name` (host) / `align_name`_device; `masked`: the aligning
    and timing entries take free_ends.  The library file is `lib_file` beside libswmi.so, or what the variable `env` names."""

    def __init__(self, prefix, align_name, lib_file, env, masked):
        super().__init__(prefix, lib_file, env, self._declare)
        self.align_name, self.masked = align_name, masked

    def _declare(self, lib):
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        call = [vp, sz, vp, sz, sz, vp, vp, ci, ci] + ([ctypes.c_uint] if self.masked else []) + [vp, vp, vp, vp]
        getattr(lib, self.align_name).argtypes = call
        getattr(lib, self.align_name + "_device").argtypes = call + [vp]
        getattr(lib, self.prefix + "_slices_for").argtypes = [sz, sz, sz, ci, ctypes.POINTER(sz), sz]
        getattr(lib, self.prefix + "_slices_for").restype = sz
        getattr(lib, self.prefix + "_time_device").argtypes = call + [vp, ci, ctypes.POINTER(ctypes.c_float)]

    def _call(self, entry, shape, score_matrix, gap_open, gap_extend, free_ends, *tail):
        """entry(*shape, matrix address, gaps, the mask where the entries take it, *tail), checked."""
        params = _affine(score_matrix, gap_open, gap_extend)       # carries the matrix itself, so that it outlives the call
        mask = (_free_ends(free_ends),) if self.masked else ()
        return self.check(entry(*shape, params[0].ctypes.data, *params[1:], *mask, *tail))

    def align(self, seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback):
        a, b, n, len1, len2 = _pair_batch(seq1s, seq2s)
        d = _diagonals(diagonals, n)
        scores = np.zeros(n, np.int32)
        ends = np.zeros((n, 4), np.int32)
        moves = np.zeros((n, _move_words(len1, len2)), np.uint64) if traceback else None
        steps = np.zeros(n, np.uint32) if traceback else None
        self._call(getattr(self.load(), self.align_name), (a.ctypes.data, len1, b.ctypes.data, len2, n, _ptr(d)), score_matrix, gap_open,
                   gap_extend, free_ends, scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps))
        return scores, ends, moves, steps

    def align_device(self, seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, free_ends, diagonals, stream):
        shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
        self._call(getattr(self.load(), self.align_name + "_device"), shape, score_matrix, gap_open, gap_extend, free_ends, *out,
                   _stream_handle(stream, seq1s))

    def time_device(self, seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves, steps, free_ends, diagonals, stream, iters):
        shape, out = _device_args(seq1s, seq2s, diagonals, scores, ends, moves, steps)
        ms = ctypes.c_float()
        self._call(self.entry("time_device"), shape, score_matrix, gap_open, gap_extend, free_ends, *out, _stream_handle(stream, seq1s),
                   int(iters), ctypes.byref(ms))
        return float(ms.value)

    def slices_for(self, n, len1, len2, traceback):
        return _slices(self.entry("slices_for"), int(n), int(len1), int(len2), 1 if traceback else 0)

    def release_workspaces(self):
        self.check(self.entry("release_workspaces")())
