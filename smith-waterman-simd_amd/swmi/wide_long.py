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
import os

import numpy as np

from . import ENDS_GLOBAL, ERR_NOT_INITIALIZED, SwmiError, _free_ends, _offsets_pair, _ptr, _ragged_pair, _slices
from . import load as _load_swmi
from .wide import _params, embed_dna, match_matrix  # noqa: F401  (the matrices are swmi.wide's, not copies)

MAX_LEN = 65536
LOCAL, GLOBAL = 0, 1
STRIPE_WAVES = (1, 4)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SWMI_WIDE_LONG_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libswmi_wide_long.so"))

_lib = None


def load():
    """dlopen libswmi_wide_long.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _load_swmi()            # libswmi.so, which the library links
    if not os.path.exists(LIB_PATH):
        raise SwmiError(ERR_NOT_INITIALIZED, "%s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    lib.swmi_wide_long_last_error.restype = ctypes.c_char_p
    lib.swmi_wide_long_set_stripe_waves.argtypes = [ci]
    lib.swmi_wide_long_move_offsets.argtypes = [vp, vp, sz, vp]
    lib.swmi_wide_long_local.argtypes = [vp, vp, vp, vp, sz, vp, ci, ci, vp, vp, vp, vp]
    lib.swmi_wide_long_global.argtypes = [vp, vp, vp, vp, sz, vp, ci, ci, cu, vp, vp, vp, vp]
    lib.swmi_wide_long_local_device.argtypes = [vp, vp, vp, vp, sz, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.swmi_wide_long_global_device.argtypes = [vp, vp, vp, vp, sz, vp, ci, ci, cu, vp, vp, vp, vp, vp]
    lib.swmi_wide_long_slices_for.argtypes = [vp, vp, sz, ci, ctypes.POINTER(sz), sz]
    lib.swmi_wide_long_slices_for.restype = sz
    lib.swmi_wide_long_time_device.argtypes = [ci, vp, vp, vp, vp, sz, vp, ci, ci, cu, vp, vp, vp, vp, vp, ci, ctypes.POINTER(ctypes.c_float)]
    _lib = lib
    return lib


def last_error():
    """swmi_wide_long_last_error: the text of the calling thread's last failed swmi.wide_long call."""
    return load().swmi_wide_long_last_error().decode()


def version():
    """swmi_wide_long_version."""
    return int(load().swmi_wide_long_version())


def _check(rc):
    if rc < 0:
        raise SwmiError(rc, last_error())
    return rc


def set_stripe_waves(waves):
    """swmi_wide_long_set_stripe_waves: the stripe width of the process's later calls, 1 or 4 wavefronts of 1024 columns,
    or 0 for the library's own rule (the default).  Results do not depend on it."""
    _check(load().swmi_wide_long_set_stripe_waves(int(waves)))


def move_offsets(seq1_offsets, seq2_offsets):
    """move_offsets[n + 1] of a batch (swmi_wide_long_move_offsets; needs no device): the running sum of
    SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    out = np.zeros(len(off1), np.uint64)
    _check(load().swmi_wide_long_move_offsets(off1.ctypes.data, off2.ctypes.data, len(off1) - 1, out.ctypes.data))
    return out


def _host(entry, seq1s, seq2s, params, traceback):
    cat1, off1, cat2, off2 = _ragged_pair(seq1s, seq2s)
    n = len(off1) - 1
    mo = move_offsets(off1, off2) if traceback else None
    if len(cat1) == 0:
        cat1 = np.zeros(16, np.uint8)       # every seq1 is empty: a valid pointer the library never reads
    if len(cat2) == 0:
        cat2 = np.zeros(16, np.uint8)
    scores = np.zeros(n, np.int32)
    ends = np.zeros((n, 4), np.int32)
    moves = np.zeros(int(mo[-1]), np.uint64) if traceback else None
    steps = np.zeros(n, np.uint32) if traceback else None
    _check(entry(cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, params[0].ctypes.data, *params[1:],
                 scores.ctypes.data, ends.ctypes.data, _ptr(moves), _ptr(steps)))
    return scores, ends, moves, mo, steps


def local(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True):
    """swmi_wide_long_local: swmi.wide.local for 0 <= len1, len2 <= 65536.  seq1s and seq2s: each a list of 1-D uint8 arrays,
    or a (concatenated, offsets[n + 1]) pair; score_matrix: 1024 int8, row = seq1's letter.

    Returns (scores[n] int32, ends[n, 4] int32 = (end_i, end_j, start_i, start_j), moves uint64 (flat: alignment k's at
    move_offsets[k] ..), move_offsets[n + 1], steps[n] uint32); traceback=False: moves, move_offsets and steps are None and the
    start cell is (-1, -1)."""
    return _host(load().swmi_wide_long_local, seq1s, seq2s, _params(score_matrix, gap_open, gap_extend), traceback)


def global_(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=ENDS_GLOBAL, traceback=True):
    """swmi_wide_long_global: swmi.wide.global_ for 0 <= len1, len2 <= 65536, under the domain rule P (len1 + len2) <= 2^23;
    arguments and result as local(), with scores that may be negative."""
    return _host(load().swmi_wide_long_global, seq1s, seq2s, _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), traceback)


def _device(entry, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, params, *tail):
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _check(entry(d_seq1s, off1.ctypes.data, d_seq2s, off2.ctypes.data, len(off1) - 1, params[0].ctypes.data, *params[1:], *tail))


def local_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None,
                 d_steps=None, stream=0):
    """swmi_wide_long_local_device: device pointers of the current device, both offset arrays host arrays of n + 1
    (asynchronous on `stream`); d_moves = d_steps = None: ends-only."""
    _device(load().swmi_wide_long_local_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, _params(score_matrix, gap_open, gap_extend),
            d_scores, d_ends, d_moves, d_steps, stream)


def global_device(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                  d_moves=None, d_steps=None, stream=0):
    """swmi_wide_long_global_device: as local_device with the mask."""
    _device(load().swmi_wide_long_global_device, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
            _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream)


def slices_for(seq1_offsets, seq2_offsets, traceback=True):
    """The slices a call cuts its batch into (swmi_wide_long_slices_for; needs no device)."""
    off1, off2 = _offsets_pair(seq1_offsets, seq2_offsets)
    return _slices(load().swmi_wide_long_slices_for, off1.ctypes.data, off2.ctypes.data, len(off1) - 1, 1 if traceback else 0)


def time_device(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends,
                d_moves=None, d_steps=None, stream=0, iters=10):
    """swmi_wide_long_time_device: average ms of `iters` device calls of kind LOCAL or GLOBAL, after one untimed call."""
    ms = ctypes.c_float()
    entry = load().swmi_wide_long_time_device
    _device(lambda *args: entry(int(kind), *args), d_seq1s, seq1_offsets, d_seq2s, seq2_offsets,
            _params(score_matrix, gap_open, gap_extend, _free_ends(free_ends)), d_scores, d_ends, d_moves, d_steps, stream, int(iters),
            ctypes.byref(ms))
    return float(ms.value)


def release_workspaces():
    """swmi_wide_long_release_workspaces: free the current device's workspaces and host-entry buffers."""
    _check(load().swmi_wide_long_release_workspaces())
