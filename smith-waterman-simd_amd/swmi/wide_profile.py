"""A batch of sequences over 32 LETTERS (the database, MIXED lengths) against ONE position-specific scoring matrix of len2
columns (a PSSM; a plain query under a 32 x 32 matrix is from_sequence's special case): local, and global / fit / overlap
by the free_ends mask, affine gaps, end cell, start cell and traceback or ends-only.  The ctypes binding of
libswmi_wide_profile.so (include/swmi_wide_profile.h).  Reached as swmi.wide_profile.<name>.

A library of its own beside libswmi.so: it needs no swmi.init(), runs on the calling thread's current HIP device, and keeps
its own workspaces and its own last error.  The semantics are swmi.wide's, field for field, with the score of cell (i, j) =
profile[(j - 1) * 32 + (seq1[i-1] & 31)]; profile is an int8 array of len2 * 32 entries (or of shape (len2, 32)), position-major,
in host memory.  0 <= len1 <= 16384 per sequence, 0 <= len2 <= 4096.  The masks (swmi.ENDS_*, swmi.FREE_*) and the expander
(swmi.local_full_expand_moves) are the package's."""
import ctypes

import numpy as np

from . import (ENDS_GLOBAL, ERR_DOMAIN, ERR_NOT_INITIALIZED, SwmiError, _affine_gap, _free_ends, _ptr, _ragged_seq1s, _slices,  # noqa: F401
               local_full_expand_moves)
from ._library import Library
from ._wide_binding import results
from .wide import _sm

LETTERS = 32
MAX_LEN1 = 16384
MAX_LEN2 = 4096
LOCAL, GLOBAL = 0, 1


def _declare(lib):
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    lib.swmi_wide_profile_from_sequence.argtypes = [vp, sz, vp, vp]
    lib.swmi_wide_profile_move_offsets.argtypes = [vp, sz, sz, vp]
    lib.swmi_wide_profile_local.argtypes = [vp, vp, sz, vp, sz, ci, ci, vp, vp, vp, vp]
    lib.swmi_wide_profile_global.argtypes = [vp, vp, sz, vp, sz, ci, ci, cu, vp, vp, vp, vp]
    lib.swmi_wide_profile_local_device.argtypes = [vp, vp, sz, vp, sz, ci, ci, vp, vp, vp, vp, vp]
    lib.swmi_wide_profile_global_device.argtypes = [vp, vp, sz, vp, sz, ci, ci, cu, vp, vp, vp, vp, vp]
    lib.swmi_wide_profile_slices_for.argtypes = [vp, sz, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_wide_profile_slices_for.restype = sz
    lib.swmi_wide_profile_time_device.argtypes = [ci, vp, vp, sz, vp, sz, ci, ci, cu, vp, vp, vp, vp, vp, ci, ctypes.POINTER(ctypes.c_float)]


_library = Library("swmi_wide_profile", "libswmi_wide_profile.so", "SWMI_WIDE_PROFILE_LIB", _declare)
LIB_PATH = _library.lib_path
_check = _library.check


def load():
    """dlopen libswmi_wide_profile.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    return _library.load()


def last_error():
    """swmi_wide_profile_last_error: the text of the calling thread's last failed swmi.wide_profile call."""
    return _library.last_error()


def version():
    """swmi_wide_profile_version."""
    return _library.version()


def _profile(profile):
    """(int8 array of len2 * 32 or None when len2 = 0, len2), checked for what the cast would wrap."""
    raw = np.asarray(profile).reshape(-1)
    if raw.size % LETTERS:
        raise ValueError("profile must have len2 * 32 entries")
    if raw.size and raw.dtype != np.int8 and (raw.min() < -128 or raw.max() > 127):
        raise SwmiError(ERR_DOMAIN, "profile entries must lie in [-128, 127] (got %d..%d)" % (raw.min(), raw.max()))
    return (np.ascontiguousarray(raw, dtype=np.int8) if raw.size else None), raw.size // LETTERS


def _params(profile, gap_open, gap_extend, *mask):
    """(profile, len2, gap_open, gap_extend[, mask]), checked for what ctypes would wrap."""
    return _profile(profile) + (_affine_gap("gap_open", gap_open), _affine_gap("gap_extend", gap_extend)) + mask


def _offsets(seq1_offsets):
    off = np.ascontiguousarray(seq1_offsets, dtype=np.uint64).reshape(-1)
    if len(off) < 1:
        raise ValueError("seq1_offsets must hold n + 1 entries")
    return off


def from_sequence(query, score_matrix):
    """swmi_wide_profile_from_sequence: the profile (len2, 32) int8 of a plain query under a 32 x 32 matrix,
    profile[j, a] = score_matrix[a * 32 + (query[j] & 31)]: with it every result equals swmi.wide's on (seq1, query)."""
    q = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1)
    sm = _sm(score_matrix)
    out = np.zeros((len(q), LETTERS), np.int8)
    _check(load().swmi_wide_profile_from_sequence(_ptr(q) if len(q) else None, len(q), sm.ctypes.data, _ptr(out) if len(q) else None))
    return out


def move_offsets(seq1_offsets, len2):
    """swmi_wide_profile_move_offsets: move_offsets[n + 1], the running sum of the words of (len1_k, len2); needs no device."""
    off = _offsets(seq1_offsets)
    out = np.zeros(len(off), np.uint64)
    _check(load().swmi_wide_profile_move_offsets(off.ctypes.data, len(off) - 1, int(len2), out.ctypes.data))
    return out


def _host(entry, seqs, params, traceback):
    cat, off = _ragged_seq1s(seqs)
    n = len(off) - 1
    mo = move_offsets(off, params[1]) if traceback else None
    if len(cat) == 0:
        cat = np.zeros(16, np.uint8)        # every sequence is empty: a valid pointer the library never reads
    scores, ends, moves, steps = results(n, mo)
    _check(entry(cat.ctypes.data, off.ctypes.data, n, _ptr(params[0]), *params[1:], scores.ctypes.data, ends.ctypes.data, _ptr(moves),
                 _ptr(steps)))
    return scores, ends, moves, mo, steps


def local(seqs, profile, gap_open, gap_extend, traceback=True):
    """swmi_wide_profile_local: local alignment (Smith-Waterman / Gotoh, zero floor) of every sequence against the profile.
    seqs: a list of 1-D uint8 arrays, or a (concatenated, offsets[n + 1]) pair; profile: int8, len2 * 32 entries.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _host(load().swmi_wide_profile_local, seqs, _params(profile, gap_open, gap_extend), traceback)


def global_(seqs, profile, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_wide_profile_global: global / fit / overlap alignment (free_ends: a mask of swmi.FREE_*; index 1 is the sequence,
    index 2 the profile); arguments and result as local(), with scores that may be negative."""
    return _host(load().swmi_wide_profile_global, seqs, _params(profile, gap_open, gap_extend, _free_ends(free_ends)), traceback)


def _device(entry, d_seq1s, seq1_offsets, params, *tail):
    off = _offsets(seq1_offsets)
    return _check(entry(d_seq1s, off.ctypes.data, len(off) - 1, _ptr(params[0]), *params[1:], *tail))


def local_device(d_seq1s, seq1_offsets, profile, gap_open, gap_extend, d_scores, d_ends, d_moves=None, d_steps=None, stream=0):
    """swmi_wide_profile_local_device: d_seq1s and the results are device pointers of the current device, seq1_offsets and
    profile host arrays (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _device(load().swmi_wide_profile_local_device, d_seq1s, seq1_offsets, _params(profile, gap_open, gap_extend), d_scores, d_ends,
            d_moves, d_steps, stream)


def global_device(d_seq1s, seq1_offsets, profile, gap_open, gap_extend, free_ends, d_scores, d_ends, d_moves=None, d_steps=None,
                  stream=0):
    """swmi_wide_profile_global_device: as local_device with the mask."""
    _device(load().swmi_wide_profile_global_device, d_seq1s, seq1_offsets, _params(profile, gap_open, gap_extend, _free_ends(free_ends)),
            d_scores, d_ends, d_moves, d_steps, stream)


def slices_for(seq1_offsets, len2, traceback=True):
    """The slices a call cuts its batch into (swmi_wide_profile_slices_for; needs no device)."""
    off = _offsets(seq1_offsets)
    return _slices(load().swmi_wide_profile_slices_for, off.ctypes.data, len(off) - 1, int(len2), 1 if traceback else 0)


def time_device(kind, d_seq1s, seq1_offsets, profile, gap_open, gap_extend, free_ends, d_scores, d_ends, d_moves=None, d_steps=None,
                stream=0, iters=10):
    """swmi_wide_profile_time_device: average ms of `iters` device calls of kind LOCAL or GLOBAL, after one untimed call."""
    ms = ctypes.c_float()
    entry = load().swmi_wide_profile_time_device
    _device(lambda *args: entry(int(kind), *args), d_seq1s, seq1_offsets, _params(profile, gap_open, gap_extend, _free_ends(free_ends)),
            d_scores, d_ends, d_moves, d_steps, stream, int(iters), ctypes.byref(ms))
    return float(ms.value)


def release_workspaces():
    """swmi_wide_profile_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_wide_profile_release_workspaces())


def search(seqs, profile, gap_open, gap_extend, top, kind=LOCAL, free_ends=0):
    """An ends-only call over all sequences, then a traceback call over the `top` best by (score descending, index ascending).

    Returns (indices[t] int64, scores[t] int32, ends[t, 4] int32, paths): t = min(top, n); paths[r] is the (steps + 1, 2) int32
    list of (i, j) from the start cell to the end cell of sequence indices[r] (swmi.local_full_expand_moves)."""
    cat, off = _ragged_seq1s(seqs)
    n = len(off) - 1

    def call(which, traceback):
        if int(kind) == LOCAL:
            return local(which, profile, gap_open, gap_extend, traceback=traceback)
        return global_(which, profile, gap_open, gap_extend, free_ends=free_ends, traceback=traceback)

    all_scores = call((cat, off), False)[0]
    order = np.lexsort((np.arange(n), -all_scores.astype(np.int64)))[:max(0, min(int(top), n))]
    picked = [cat[int(off[k]):int(off[k + 1])] for k in order]
    scores, ends, moves, mo, steps = call(picked, True)
    paths = [local_full_expand_moves(moves[int(mo[r]):int(mo[r + 1])], steps[r], ends[r, 0], ends[r, 1]) for r in range(len(order))]
    return order.astype(np.int64), scores, ends, paths
