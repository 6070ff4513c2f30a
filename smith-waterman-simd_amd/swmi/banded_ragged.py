"""The banded aligners on a batch of MIXED (len1, len2) in one call: the ctypes binding of libswmi_banded_ragged.so
(include/swmi_banded_ragged.h).  Reached as swmi.banded_ragged.<name>.

local() is swmi.banded.align and global_() is swmi.banded_global.align with a (len1, len2) and a diagonal of its own per
alignment, 0 .. 16384 each, and one matrix, one pair of gaps and (global_) one free_ends mask per call: alignment k's score,
ends, steps and moves are what the fixed entry gives for that pair alone.  A library of its own beside libswmi.so: it needs no
swmi.init(), runs on the calling thread's current HIP device, and keeps its own workspaces and its own last error.  The layout
of the moves (swmi.local_full_ragged_move_offsets) and the expander (swmi.local_full_expand_moves) are the package's.

An empty sequence: local() gives score 0, ends (0, 0, 0, 0) and no step; global_() gives what the one border the table then
consists of gives under the band and the mask, NO_ALIGNMENT where no finite candidate lies in the band."""
import ctypes
import os

import numpy as np

from . import (ERR_NOT_INITIALIZED, SwmiError, _affine, _free_ends, _offsets_pair, _ptr, _ragged_pair, _slices,
               local_full_expand_moves, local_full_ragged_move_offsets)
from . import load as _load_swmi
from ._banded_binding import _diagonals

LOCAL, GLOBAL = 0, 1          # SWMI_BANDED_RAGGED_LOCAL / SWMI_BANDED_RAGGED_GLOBAL
MAX_LEN = 16384
WIDTH = 128
LO, HI = -64, 63
SLOT_BYTES = 48               # SWMI_BANDED_RAGGED_SLOT_BYTES
END_ANYWHERE = 16             # SWMI_BANDED_END_ANYWHERE
NO_ALIGNMENT = -2**31         # SWMI_BANDED_NO_ALIGNMENT: the score of an infeasible alignment (global kind)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_BANDED_RAGGED_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_banded_ragged.so"))
_lib = None


def load():
    """dlopen libswmi_banded_ragged.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _load_swmi()            # libswmi.so, which the library links
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    head, tail = [vp, vp, vp, vp, sz, vp, vp, ci, ci], [vp, vp, vp, vp]
    lib.swmi_banded_ragged_last_error.restype = ctypes.c_char_p
    lib.swmi_banded_ragged_local.argtypes = head + tail
    lib.swmi_banded_ragged_global.argtypes = head + [cu] + tail
    lib.swmi_banded_ragged_local_device.argtypes = head + tail + [vp]
    lib.swmi_banded_ragged_global_device.argtypes = head + [cu] + tail + [vp]
    lib.swmi_banded_ragged_slices_for.argtypes = [ci, vp, vp, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_banded_ragged_slices_for.restype = sz
    lib.swmi_banded_ragged_time_device.argtypes = [ci] + head + [cu] + tail + [vp, ci, ctypes.POINTER(ctypes.c_float)]
    _lib = lib
    return lib


def last_error():
    """swmi_banded_ragged_last_error: the text of the calling thread's last failed swmi.banded_ragged call."""
    return load().swmi_banded_ragged_last_error().decode()


def version():
    """swmi_banded_ragged_version."""
    return int(load().swmi_banded_ragged_version())


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, last_error())
    return rc


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a mixed batch: alignment k's moves start at word move_offsets[k]
    (swmi.local_full_ragged_move_offsets: there is no second function)."""
    return local_full_ragged_move_offsets(seq1_offsets, seq2_offsets)


def _host(kind, seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback):
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
    head = (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, _ptr(d), sm.ctypes.data, go, ge)
    tail = (scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps))
    if kind == GLOBAL:
        _check(load().swmi_banded_ragged_global(*head, _free_ends(free_ends), *tail))
    else:
        _check(load().swmi_banded_ragged_local(*head, *tail))
    return scores, ends, moves, mo, steps


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True):
    """swmi_banded_ragged_local: swmi.banded.align with a (len1, len2) of its own per alignment.  seq1s and seq2s: each a list
    of 1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair; diagonals: n int32, or None for the main diagonal.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _host(LOCAL, seq1s, seq2s, score_matrix, gap_open, gap_extend, 0, diagonals, traceback)


def global_(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True):
    """swmi_banded_ragged_global: swmi.banded_global.align on a mixed batch under the one mask free_ends (0 .. 19); arguments
    and result as local().  An infeasible alignment has score NO_ALIGNMENT, ends (0, 0, 0, 0) (ends-only (0, 0, -1, -1)) and 0
    steps."""
    return _host(GLOBAL, seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends, diagonals, traceback)


def _dev(x):
    """a device pointer: an int, None, or anything with data_ptr() (a torch tensor)"""
    return x.data_ptr() if hasattr(x, "data_ptr") else x


def _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, score_matrix, gap_open, gap_extend):
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    n = len(off1) - 1
    d = _diagonals(diagonals, n)
    sm, go, ge = _affine(score_matrix, gap_open, gap_extend)
    return (_dev(d_seq1s), off1.ctypes.data, _dev(d_seq2s), off2.ctypes.data, n, _ptr(d), sm.ctypes.data, go, ge), (off1, off2, d, sm)


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, diagonals=None, stream=0):
    """swmi_banded_ragged_local_device: the sequence and result buffers are device pointers (ints or torch tensors, 16-byte
    aligned); both offset arrays AND the diagonals are host arrays, read before the call returns.  Asynchronous on `stream`;
    d_moves = d_steps = None: ends-only."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, score_matrix, gap_open, gap_extend)
    _check(load().swmi_banded_ragged_local_device(*head, _dev(d_scores), _dev(d_ends), _dev(d_moves), _dev(d_steps), _dev(stream)))
    del keep


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, diagonals=None, stream=0):
    """swmi_banded_ragged_global_device: as local_device, under the mask free_ends."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, score_matrix, gap_open, gap_extend)
    _check(load().swmi_banded_ragged_global_device(*head, _free_ends(free_ends), _dev(d_scores), _dev(d_ends), _dev(d_moves),
                                                   _dev(d_steps), _dev(stream)))
    del keep


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10):
    """swmi_banded_ragged_time_device: average ms of `iters` device calls of `kind` (LOCAL / GLOBAL) after one untimed call;
    arguments as global_device (free_ends is ignored by the local kind)."""
    head, keep = _device_head(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, diagonals, score_matrix, gap_open, gap_extend)
    ms = ctypes.c_float()
    _check(load().swmi_banded_ragged_time_device(int(kind), *head, _free_ends(free_ends), _dev(d_scores), _dev(d_ends), _dev(d_moves),
                                                 _dev(d_steps), _dev(stream), int(iters), ctypes.byref(ms)))
    del keep
    return float(ms.value)


def slices_for(kind, seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call of `kind` cuts its batch into (swmi_banded_ragged_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_banded_ragged_slices_for, int(kind), off1.ctypes.data, off2.ctypes.data, len(off1) - 1, 1 if traceback else 0)


def paths(result):
    """The (steps + 1, 2) int32 lists of (i, j) from the start cell to the end cell of a traceback result of local() or
    global_(); None for an infeasible alignment."""
    scores, ends, moves, mo, steps = result
    return [None if int(scores[k]) == NO_ALIGNMENT else
            local_full_expand_moves(moves[int(mo[k]):int(mo[k + 1])], steps[k], ends[k, 0], ends[k, 1]) for k in range(len(scores))]


def release_workspaces():
    """swmi_banded_ragged_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_banded_ragged_release_workspaces())
