"""The one ctypes binding body of the two wide-alphabet libraries on mixed (len1, len2) batches: swmi.wide
(libswmi_wide.so) and swmi.wide_long (libswmi_wide_long.so) each hold a WideBinding and their public functions call it.  The
libraries' entries differ by their prefix, by the function that lays out the moves, and by what the long one has besides."""
import ctypes

import numpy as np

from . import _offsets_pair, _ptr, _ragged_pair, _slices
from ._library import Library


def results(n, move_offsets):
    """The fresh result arrays of a host call on a mixed batch: (scores[n] int32, ends[n, 4] int32, moves uint64 (flat), steps[n]
    uint32); move_offsets None: ends-only (moves and steps are None)."""
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    moves = None if move_offsets is None else np.zeros(int(move_offsets[-1]), np.uint64)
    steps = None if move_offsets is None else np.zeros(n, np.uint32)
    return scores, ends, moves, steps


class WideBinding(Library):
    """One library: `move_offsets(off1, off2)` lays out a traceback call's moves; `extra`: the argtypes of the entries it has
    besides the shared ones, by name.  `params` below is (matrix, gap_open, gap_extend[, mask]), checked by the caller: it carries
    the matrix itself, so that it outlives the call."""

    def __init__(self, prefix, lib_file, env, move_offsets, extra=None):
        super().__init__(prefix, lib_file, env, self._declare)
        self.move_offsets, self.extra = move_offsets, extra or {}

    def _declare(self, lib):
        vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
        head, tail = [vp, vp, vp, vp, sz, vp, ci, ci], [vp, vp, vp, vp]
        argtypes = {"local": head + tail, "global": head + [cu] + tail,
                    "local_device": head + tail + [vp], "global_device": head + [cu] + tail + [vp],
                    "slices_for": [vp, vp, sz, ci, ctypes.POINTER(sz), sz],
                    "time_device": [ci] + head + [cu] + tail + [vp, ci, ctypes.POINTER(ctypes.c_float)]}
        argtypes.update(self.extra)
        for name, types in argtypes.items():
            getattr(lib, self.prefix + "_" + name).argtypes = types
        getattr(lib, self.prefix + "_slices_for").restype = sz

    def host(self, name, seq1s, seq2s, params, traceback):
        cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
        n = len(off1) - 1
        mo = self.move_offsets(off1, off2) if traceback else None
        if len(cat1) == 0:
            cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
        if len(cat2) == 0:
            cat2 = np.zeros(16, np.uint8)
        scores, ends, moves, steps = results(n, mo)
        self.check(self.entry(name)(cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, params[0].ctypes.data,
                                    *params[1:], scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))
        return scores, ends, moves, mo, steps

    def device(self, name, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, params, *tail, kind=()):
        """entry(*kind, the shape, matrix address, gaps and mask, *tail), checked; `kind`: what the timer takes first."""
        off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
        return self.check(self.entry(name)(*kind, d_seq1s, off1.ctypes.data, d_seq2s, off2.ctypes.data, len(off1) - 1,
                                           params[0].ctypes.data, *params[1:], *tail))

    def time_device(self, kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, params, *tail, iters):
        ms = ctypes.c_float()
        self.device("time_device", d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, params, *tail, int(iters), ctypes.byref(ms),
                    kind=(int(kind),))
        return float(ms.value)

    def slices_for(self, seq1_offsets, seq2_offsets, traceback):
        off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
        return _slices(self.entry("slices_for"), off1.ctypes.data, off2.ctypes.data, len(off1) - 1, 1 if traceback else 0)

    def release_workspaces(self):
        self.check(self.entry("release_workspaces")())
