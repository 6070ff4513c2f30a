"""The banded aligners on a batch of mixed (len1, len2) with the BAND'S WIDTH per call: the ctypes binding of
libswmi_banded_width.so (include/swmi_banded_width.h).  Reached as swmi.banded_width.<name>.

The functions are swmi.banded_ragged's with one more argument, `band`, directly before score_matrix as in the C ABI: 128, 256,
512 or 1024 diagonals, cell (i, j) of alignment k being in the band iff -band/2 <= (j - i) - diagonals[k] <= band/2 - 1.  With
band = 128 every result is swmi.banded_ragged's.  A library of its own beside libswmi.so: it needs no swmi.init(), runs on the
calling thread's current HIP device, and keeps its own workspaces and its own last error."""
import ctypes
import os

import numpy as np

from . import (ERR_NOT_INITIALIZED, SwmiError, _affine, _free_ends, _offsets_pair, _ptr, _ragged_pair, _slices,
               local_full_expand_moves, local_full_ragged_move_offsets)
from . import load as _load_swmi
from ._banded_binding import _diagonals

LOCAL, GLOBAL = 0, 1          # SWMI_BANDED_WIDTH_LOCAL / SWMI_BANDED_WIDTH_GLOBAL
MAX_LEN = 16384
WIDTHS = (128, 256, 512, 1024)
SLOT_BYTES = 48               # SWMI_BANDED_WIDTH_SLOT_BYTES
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment (global kind)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_BANDED_WIDTH_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_banded_width.so"))
_lib = None


def load():
    """dlopen libswmi_banded_width.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _load_swmi()            # libswmi.so, which the library links
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    head, tail = [vp, vp, vp, vp, sz, vp, ci, vp, ci, ci], [vp, vp, vp, vp]
    lib.swmi_banded_width_last_error.restype = ctypes.c_char_p
    lib.swmi_banded_width_local.argtypes = head + tail
    lib.swmi_banded_width_global.argtypes = head + [cu] + tail
    lib.swmi_banded_width_local_device.argtypes = head + tail + [vp]
    lib.swmi_banded_width_global_device.argtypes = head + [cu] + tail + [vp]
    lib.swmi_banded_width_slices_for.argtypes = [ci, ci, vp, vp, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_banded_width_slices_for.restype = sz
    lib.swmi_banded_width_time_device.argtypes = [ci] + head + [cu] + tail + [vp, ci, ctypes.POINTER(ctypes.c_float)]
    _lib = lib
    return lib


def last_error():
    """swmi_banded_width_last_error: the text of the calling thread's last failed swmi.banded_width call."""
    return load().swmi_banded_width_last_error().decode()


def version():
    """swmi_banded_width_version."""
    return int(load().swmi_banded_width_version())


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, last_error())
    return rc


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a mixed batch (swmi.local_full_ragged_move_offsets: there is no second function)."""
    return local_full_ragged_move_offsets(seq1_offsets, seq2_offsets)


def _host(kind, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback):
    cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
    n = len(off1) - 1
    d = _diagonals(diagonals, n)
    mo = move_offsets(off1, off2) if traceback else None
    if len(cat1) == 0:
        cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
    if len(cat2) == 0:
        cat2 = np.zeros(16, np.uint8)
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    moves = np.zeros(int(mo[-1]), np.uint64) if traceback else None
    steps = np.zeros(n, np.uint32) if traceback else None
    sm, go, ge = _affine(score_matrix, gap_open, gap_extend)
    head = (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, _ptr(d), int(band), sm.ctypes.data, go, ge)
    tail = (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps))
    if kind == GLOBAL:
        _check(load().swmi_banded_width_global(*head, _free_ends(free_ends), *tail))
    else:
        _check(load().swmi_banded_width_local(*head, *tail))
    return scores, ends, moves, mo, steps


def local(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_width_local: swmi.banded_ragged.local under a band of `band` diagonals (128, 256, 512 or 1024); the other
    arguments and the result are that function's."""
    return _host(LOCAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def global_(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_width_global: swmi.banded_ragged.global_ under a band of `band` diagonals."""
    return _host(GLOBAL, seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def _dev(x):
    """a device pointer: an int, None, or anything with data_ptr() (a torch tensor)"""
    return x.data_ptr() if hasattr(x, "data_ptr") else x


def _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend):
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    n = len(off1) - 1
    d = _diagonals(diagonals, n)
    sm, go, ge = _affine(score_matrix, gap_open, gap_extend)
    return (_dev(d_seq1s), off1.ctypes.data, _dev(d_seq2s), off2.ctypes.data, n, _ptr(d), int(band), sm.ctypes.data, go, ge), (off1, off2, d, sm)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, diagonals=None, stream=0):
    """swmi_banded_width_local_device: swmi.banded_ragged.local_device under a band of `band` diagonals."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend)
    _check(load().swmi_banded_width_local_device(*head, _dev(d_scores), _dev(d_ends), _dev(d_moves), _dev(d_steps), _dev(stream)))
    del keep


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, diagonals=None, stream=0):
    """swmi_banded_width_global_device: as local_device, under the mask free_ends."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend)
    _check(load().swmi_banded_width_global_device(*head, _free_ends(free_ends), _dev(d_scores), _dev(d_ends), _dev(d_moves),
                                                  _dev(d_steps), _dev(stream)))
    del keep


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10):
    """swmi_banded_width_time_device: average ms of `iters` device calls of `kind` (LOCAL / GLOBAL) after one untimed call;
    arguments as global_device (free_ends is ignored by the local kind)."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, band, score_matrix, gap_open, gap_extend)
    ms = ctypes.c_float()
    _check(load().swmi_banded_width_time_device(int(kind), *head, _free_ends(free_ends), _dev(d_scores), _dev(d_ends), _dev(d_moves),
                                                _dev(d_steps), _dev(stream), int(iters), ctypes.byref(ms)))
    del keep
    return float(ms.value)


def slices_for(kind, band, seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call of `kind` at width `band` cuts its batch into (swmi_banded_width_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_banded_width_slices_for, int(kind), int(band), off1.ctypes.data, off2.ctypes.data, len(off1) - 1,
                   1 if traceback else 0)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local() or
    global_(); None for an infeasible alignment."""
    scores, ends, moves, mo, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else
            local_full_expand_moves(moves[int(mo[k]):int(mo[k + 1])], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_width_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_banded_width_release_workspaces())
