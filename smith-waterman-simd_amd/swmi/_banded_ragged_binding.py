"""The one ctypes binding body of the three mixed-shape banded libraries (DESIGN.md sections 39 and 41): swmi.banded_ragged
(libswmi_banded_ragged.so), swmi.banded_width (libswmi_banded_width.so) and swmi.banded_long (libswmi_banded_long.so) each hold a
RaggedBinding and their public functions call it.  The libraries' entries differ by their prefix, by one argument -- the width
and the long library's take `band` directly before score_matrix (slices_for: directly behind kind) -- and by the function that
lays out the moves, which the module gives."""
import ctypes

import numpy as np

from . import _affine, _free_ends, _offsets_pair, _ptr, _ragged_pair, _slices
from ._banded_binding import _diagonals
from ._library import Library
from ._wide_binding import results

LOCAL, GLOBAL = 0, 1


def _dev(x):
    """a device pointer: an int, None, or anything with data_ptr() (a torch tensor)"""
    return x.data_ptr() if hasattr(x, "data_ptr") else x


class RaggedBinding(Library):
    """One library: its entries are `prefix`_<name>; `has_band`: they take a band, and the methods below pass the one they are
    given (the ragged library's wrappers give None).  The library file is `lib_file` beside libswmi.so, or what the variable
    `env` names.  `move_offsets(seq1_offsets, seq2_offsets)` is the library's layout of the moves; `extra`: {entry: argtypes} of entries
    that only this library has."""

    def __init__(self, prefix, lib_file, env, has_band, move_offsets, extra=None):
        super().__init__(prefix, lib_file, env, self._declare)
        self.has_band, self.move_offsets, self.extra = has_band, move_offsets, extra or {}

    def _declare(self, lib):
        vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
        band = [ci] if self.has_band else []
        head, tail = [vp, vp, vp, vp, sz, vp] + band + [vp, ci, ci], [vp, vp, vp, vp]
        entry = lambda name: getattr(lib, self.prefix + "_" + name)  # noqa: E731
        entry("local").argtypes = head + tail
        entry("global").argtypes = head + [cu] + tail
        entry("local_device").argtypes = head + tail + [vp]
        entry("global_device").argtypes = head + [cu] + tail + [vp]
        entry("slices_for").argtypes = [ci] + band + [vp, vp, sz, ci, ctypes.POINTER(sz), sz]
        entry("slices_for").restype = sz
        entry("time_device").argtypes = [ci] + head + [cu] + tail + [vp, ci, ctypes.POINTER(ctypes.c_float)]
        for name, argtypes in self.extra.items():
            entry(name).argtypes = argtypes

    def _band(self, band):
        return (int(band),) if self.has_band else ()

    def host(self, kind, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback):
        cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
        n = len(off1) - 1
        d = _diagonals(diagonals, n)
        mo = self.move_offsets(off1, off2) if traceback else None
        if len(cat1) == 0:
            cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
        if len(cat2) == 0:
            cat2 = np.zeros(16, np.uint8)
        scores, ends, moves, steps = results(n, mo)
        sm, go, ge = _affine(score_matrix, gap_open, gap_extend)
        head = (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, _ptr(d), *self._band(band), sm.ctypes.data, go, ge)
        tail = (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps))
        if kind == GLOBAL:
            self.check(self.entry("global")(*head, _free_ends(free_ends), *tail))
        else:
            self.check(self.entry("local")(*head, *tail))
        return scores, ends, moves, mo, steps

    def _device_head(self, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend):
        off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
        n = len(off1) - 1
        d = _diagonals(diagonals, n)
        sm, go, ge = _affine(score_matrix, gap_open, gap_extend)
        return ((_dev(d_seq1s), off1.ctypes.data, _dev(d_seq2s), off2.ctypes.data, n, _ptr(d), *self._band(band), sm.ctypes.data, go, ge),
                (off1, off2, d, sm))

    def device(self, kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
               d_moves, d_steps, diagonals, stream):
        head, keep = self._device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend)
        mask = (_free_ends(free_ends),) if kind == GLOBAL else ()
        self.check(self.entry("global_device" if kind == GLOBAL else "local_device")(
            *head, *mask, _dev(d_scores), _dev(d_ends), _dev(d_moves), _dev(d_steps), _dev(stream)))
        del keep

    def time_device(self, kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores,
                    d_ends, d_moves, d_steps, diagonals, stream, iters):
        head, keep = self._device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend)
        ms = ctypes.c_float()
        self.check(self.entry("time_device")(int(kind), *head, _free_ends(free_ends), _dev(d_scores), _dev(d_ends), _dev(d_moves),
                                             _dev(d_steps), _dev(stream), int(iters), ctypes.byref(ms)))
        del keep
        return float(ms.value)

    def slices_for(self, kind, band, seq1_offsets, seq2_offsets, traceback):
        off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
        return _slices(self.entry("slices_for"), int(kind), *self._band(band), off1.ctypes.data, off2.ctypes.data, len(off1) - 1,
                       1 if traceback else 0)

    def release_workspaces(self):
        self.check(self.entry("release_workspaces")())
