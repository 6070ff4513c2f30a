"""The Python layer over the seven satellite libraries that link libswmi.so, after its loader moved into swmi/_library.py and
the body of swmi.wide / swmi.wide_long into swmi/_wide_binding.py: the three wide modules keep every
public name, signature, docstring and constant (listed literally, as inspect.signature printed them before the move), and all
seven hand the C ABI what their public headers list, argument by argument.  The expectations below were written from the
parameter lists of include/swmi_*.h and passed on the commit before the move; only _holder() knows where the loaded library is
kept.  A recording stand-in takes the library's place: no device, and no satellite library, is needed."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG

WIDE_CALLS = {
    "load": "()", "last_error": "()", "version": "()", "release_workspaces": "()",
    "local": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, traceback=True)",
    "global_": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, traceback=True)",
    "local_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None, "
                    "d_steps=None, stream=0)",
    "global_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends, "
                     "d_moves=None, d_steps=None, stream=0)",
    "slices_for": "(seq1_offsets, seq2_offsets, traceback=True)",
    "time_device": "(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends, "
                   "d_moves=None, d_steps=None, stream=0, iters=10)",
}
SIGNATURES = {
    "wide": dict(WIDE_CALLS, match_matrix="(match, mismatch)", embed_dna="(sm16)"),
    "wide_long": dict(WIDE_CALLS, set_stripe_waves="(waves)", move_offsets="(seq1_offsets, seq2_offsets)"),
    "wide_profile": {
        "load": "()", "last_error": "()", "version": "()", "release_workspaces": "()",
        "from_sequence": "(query, score_matrix)", "move_offsets": "(seq1_offsets, len2)",
        "local": "(seqs, profile, gap_open, gap_extend, traceback=True)",
        "global_": "(seqs, profile, gap_open, gap_extend, free_ends=0, traceback=True)",
        "local_device": "(d_seq1s, seq1_offsets, profile, gap_open, gap_extend, d_scores, d_ends, d_moves=None, d_steps=None, stream=0)",
        "global_device": "(d_seq1s, seq1_offsets, profile, gap_open, gap_extend, free_ends, d_scores, d_ends, d_moves=None, d_steps=None, "
                         "stream=0)",
        "slices_for": "(seq1_offsets, len2, traceback=True)",
        "time_device": "(kind, d_seq1s, seq1_offsets, profile, gap_open, gap_extend, free_ends, d_scores, d_ends, d_moves=None, d_steps=None, "
                       "stream=0, iters=10)",
        "search": "(seqs, profile, gap_open, gap_extend, top, kind=0, free_ends=0)",
    },
}
CONSTANTS = {
    "wide": {"LETTERS": 32, "MAX_LEN1": 16384, "MAX_LEN2": 4096, "LOCAL": 0, "GLOBAL": 1},
    "wide_long": {"MAX_LEN": 65536, "LOCAL": 0, "GLOBAL": 1, "STRIPE_WAVES": (1, 4)},
    "wide_profile": {"LETTERS": 32, "MAX_LEN1": 16384, "MAX_LEN2": 4096, "LOCAL": 0, "GLOBAL": 1},
}
LIBRARY = {"wide": ("libswmi_wide.so", "SWMI_WIDE_LIB"), "wide_long": ("libswmi_wide_long.so", "SWMI_WIDE_LONG_LIB"),
           "wide_profile": ("libswmi_wide_profile.so", "SWMI_WIDE_PROFILE_LIB"), "banded": ("libswmi_banded.so", "SWMI_BANDED_LIB"),
           "banded_global": ("libswmi_banded_global.so", "SWMI_BANDED_GLOBAL_LIB"),
           "banded_ragged": ("libswmi_banded_ragged.so", "SWMI_BANDED_RAGGED_LIB"),
           "banded_width": ("libswmi_banded_width.so", "SWMI_BANDED_WIDTH_LIB")}
MODULES = list(LIBRARY)

N = 3
LENS = [((5, 0, 6), (7, 4, 0)), ((0, 0, 0), (7, 4, 0))]                 # the second batch: every seq1 is empty
# swmi_local_full_ragged_move_offsets of the two batches: (((len1 + len2 + 31) // 32) + 1) & ~1 = 2 words each, 0 for (0, 0)
WORDS = [[0, 2, 4, 6], [0, 2, 4, 4]]
LAID_OUT = [0, 3, 5, 9]     # what the stand-in's own *_move_offsets entries answer: any layout must be taken as it comes
GO, GE, MASK, BAND = 11, 2, 10, 256
SM4 = np.array([2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2], np.int8)
SM32 = np.where(np.eye(32, dtype=bool), 2, -3).astype(np.int8).reshape(-1)
D1, D2, DS, DE, DM, DT, STREAM = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000      # device pointers: passed, never read


class Recorder:
    """Stands in for a loaded library: every symbol is a function that records its call, copies what the test asked to see
    through the pointers (while the wrapper's arrays are alive) and answers like the entry of that name would."""

    def __init__(self, see=None, rc=None):
        self.calls, self.seen, self.see, self.rc = [], {}, see or {}, rc or {}

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            for pos, (dtype, count) in self.see.get(name, {}).items():
                raw = ctypes.string_at(args[pos], count * np.dtype(dtype).itemsize)
                self.seen[name, pos] = np.frombuffer(raw, dtype).tolist()
            if name.endswith("_last_error"):
                return b"boom"
            if name.endswith("_version"):
                return 140
            if name.endswith("_move_offsets"):                  # the last argument is move_offsets[n + 1]
                out = np.array(LAID_OUT, np.uint64)
                ctypes.memmove(args[-1], out.ctypes.data, out.nbytes)
            if name.endswith("_time_device"):
                args[-1]._obj.value = 1.5                       # float *avg_ms
            if name.endswith("_slices_for"):                    # (..., size_t *sizes, size_t cap) -> the number of slices
                if args[-2] is not None:
                    args[-2][0], args[-2][1] = 2, 1
                return 2
            return self.rc.get(name, 0)
        return entry

    def names(self):
        return [c[0] for c in self.calls]


def _holder(mod):
    """The object whose _lib is the loaded library.  Before the move: the wide modules themselves, and _binding in the banded."""
    return getattr(mod, "_binding", None) or getattr(mod, "_library", None) or mod


def _inject(monkeypatch, mod, **kw):
    rec = Recorder(**kw)
    monkeypatch.setattr(_holder(mod), "_lib", rec)
    monkeypatch.setattr(_holder(mod), "_entries", {}, raising=False)       # the entries a Library has bound are the real library's
    assert mod.load() is rec
    return rec


def _batch(which):
    """(seq1s, seq2s, cat1, off1, cat2, off2) of LENS[which]: letters 1 .. 31, so that no byte equals the dummy's zero."""
    sides = []
    for salt, lens in enumerate(LENS[which]):
        seqs = [((np.arange(m) * 7 + k + salt) % 31 + 1).astype(np.uint8) for k, m in enumerate(lens)]
        sides.append((seqs, np.concatenate(seqs), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)))
    return sides[0][0], sides[1][0], sides[0][1], sides[0][2], sides[1][1], sides[1][2]


def _cat(cat):
    """What the entry must find behind a sequence pointer: the letters, or the 16 zero bytes of the dummy when there are none."""
    return cat.tolist() if len(cat) else [0] * 16


def _check_results(result, traceback, total):
    scores, ends, moves, mo, steps = result
    assert (scores.shape, scores.dtype) == ((N,), np.int32) and (ends.shape, ends.dtype) == ((N, 4), np.int32)
    if traceback:
        assert (moves.shape, moves.dtype) == ((total,), np.uint64) and (steps.shape, steps.dtype) == ((N,), np.uint32)
        assert (mo.shape, mo.dtype) == ((N + 1,), np.uint64)
    else:
        assert moves is None and mo is None and steps is None
    return scores.ctypes.data, ends.ctypes.data, (moves.ctypes.data if traceback else None), (steps.ctypes.data if traceback else None)


# ---- the names, signatures, docstrings and constants of the three wide modules

@pytest.mark.parametrize("name", ["wide", "wide_long", "wide_profile"])
def test_public_names_signatures_and_constants(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    for fn, sig in SIGNATURES[name].items():
        f = getattr(mod, fn)
        assert inspect.isfunction(f) and f.__doc__, fn
        assert f.__module__ == ("swmi.wide" if name == "wide_long" and fn in ("match_matrix", "embed_dna") else "swmi." + name), fn
        assert str(inspect.signature(f)) == sig, fn
    for const, value in CONSTANTS[name].items():
        assert getattr(mod, const) == value, const
    assert mod.SwmiError is swmi_mod.SwmiError and mod.ERR_NOT_INITIALIZED == -1


DOC_STARTS = {"load": "dlopen lib%s.so (built by smith-waterman-simd_amd/csrc/Makefile). Fails loudly when it is missing.",
              "last_error": "%s_last_error: the text of the calling thread's last failed swmi.", "version": "%s_version.",
              "local": "%s_local: ", "global_": "%s_global: ", "local_device": "%s_local_device: ", "global_device": "%s_global_device: ",
              "time_device": "%s_time_device: average ms of `iters` device calls of kind LOCAL or GLOBAL, after one untimed call.",
              "slices_for": "The slices a call cuts its batch into (%s_slices_for; needs no device).",
              "release_workspaces": "%s_release_workspaces: free the current device's workspaces and host-entry buffers."}


@pytest.mark.parametrize("name", ["wide", "wide_long", "wide_profile"])
def test_every_docstring_names_its_own_entry(swmi_mod, name):
    """A function's docstring is its own module's, not the shared body's: it names the entry of its own library."""
    mod = getattr(swmi_mod, name)
    for fn, start in DOC_STARTS.items():
        assert getattr(mod, fn).__doc__.startswith(start % ("swmi_" + name)), fn
    assert swmi_mod.wide.match_matrix.__doc__.startswith("32 x 32 matrix (flat, 1024 int8)")
    assert swmi_mod.wide.embed_dna.__doc__.startswith("A 4 x 4 matrix of the 4-letter aligners in the top-left corner")
    assert swmi_mod.wide_long.set_stripe_waves.__doc__.startswith("swmi_wide_long_set_stripe_waves: the stripe width")
    assert swmi_mod.wide_long.move_offsets.__doc__.startswith("move_offsets[n + 1] of a batch (swmi_wide_long_move_offsets;")
    assert swmi_mod.wide_profile.from_sequence.__doc__.startswith("swmi_wide_profile_from_sequence: the profile (len2, 32) int8")
    assert swmi_mod.wide_profile.move_offsets.__doc__.startswith("swmi_wide_profile_move_offsets: move_offsets[n + 1]")
    assert swmi_mod.wide_profile.search.__doc__.startswith("An ends-only call over all sequences, then a traceback call")


@pytest.mark.parametrize("name", MODULES)
def test_lib_path_is_the_variable_or_beside_libswmi(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    lib, env = LIBRARY[name]
    assert mod.LIB_PATH == os.environ.get(env, os.path.join(os.path.dirname(swmi_mod.LIB_PATH), lib))


def test_the_shared_matrices_and_checks_are_not_copies(swmi_mod):
    assert swmi_mod.wide_long.match_matrix is swmi_mod.wide.match_matrix and swmi_mod.wide_long.embed_dna is swmi_mod.wide.embed_dna
    assert swmi_mod.wide_profile._sm is swmi_mod.wide._sm
    from swmi._banded_binding import _diagonals
    assert _diagonals([4, -4], 2).tolist() == [4, -4]


# ---- what reaches the C ABI: swmi.wide and swmi.wide_long

@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("kind", ["local", "global"])
@pytest.mark.parametrize("name", ["wide", "wide_long"])
def test_wide_host_entries(swmi_mod, monkeypatch, name, kind, traceback, which):
    mod, sym = getattr(swmi_mod, name), "swmi_%s_%s" % (name, kind)
    seq1s, seq2s, cat1, off1, cat2, off2 = _batch(which)
    layout = "swmi_wide_long_move_offsets"
    rec = _inject(monkeypatch, mod, see={sym: {0: (np.uint8, len(cat1) or 16), 1: (np.uint64, N + 1), 2: (np.uint8, len(cat2)),
                                               3: (np.uint64, N + 1), 5: (np.int8, 1024)},
                                         layout: {0: (np.uint64, N + 1), 1: (np.uint64, N + 1)}})
    if kind == "local":
        result = mod.local(seq1s, seq2s, SM32, GO, GE, traceback=traceback)
    else:
        result = mod.global_(seq1s, seq2s, SM32, GO, GE, free_ends=MASK, traceback=traceback)
    long_layout = name == "wide_long" and traceback       # swmi.wide lays the moves out through libswmi.so, as every 4-letter aligner
    out = _check_results(result, traceback, LAID_OUT[-1] if long_layout else WORDS[which][-1])
    assert rec.names() == ([layout] if long_layout else []) + [sym]
    args = rec.calls[-1][1]
    assert args[4:] == (N, SM32.ctypes.data, GO, GE) + ((MASK,) if kind == "global" else ()) + out
    assert len(args) == (13 if kind == "global" else 12) and all(isinstance(p, int) and p for p in args[:4])
    assert rec.seen[sym, 0] == _cat(cat1) and rec.seen[sym, 2] == cat2.tolist()
    assert rec.seen[sym, 1] == off1.tolist() and rec.seen[sym, 3] == off2.tolist() and rec.seen[sym, 5] == SM32.tolist()
    if traceback:
        assert result[3].tolist() == (LAID_OUT if long_layout else WORDS[which])
    if long_layout:
        assert rec.calls[0][1][2:] == (N, result[3].ctypes.data)
        assert rec.seen[layout, 0] == off1.tolist() and rec.seen[layout, 1] == off2.tolist()


@pytest.mark.parametrize("name", ["wide", "wide_long"])
def test_wide_device_entries_timer_slices_and_the_rest(swmi_mod, monkeypatch, name):
    mod, pre = getattr(swmi_mod, name), "swmi_%s_" % name
    _, _, _, off1, _, off2 = _batch(0)
    see = {pre + e: {p: (np.uint64, N + 1), p + 2: (np.uint64, N + 1), p + 4: (np.int8, 1024)}
           for e, p in (("local_device", 1), ("global_device", 1), ("time_device", 2))}
    see[pre + "slices_for"] = {0: (np.uint64, N + 1), 1: (np.uint64, N + 1)}
    rec = _inject(monkeypatch, mod, see=see)
    head = lambda args: (args[0], args[2], args[4], args[5])  # noqa: E731
    assert mod.local_device(D1, off1, D2, off2, SM32, GO, GE, DS, DE, DM, DT, STREAM) is None
    assert mod.global_device(D1, off1, D2, off2, SM32, GO, GE, MASK, DS, DE) is None
    assert mod.time_device(mod.GLOBAL, D1, off1, D2, off2, SM32, GO, GE, MASK, DS, DE, DM, DT, stream=STREAM, iters=7) == 1.5
    assert mod.slices_for(off1, off2) == [2, 1] and mod.slices_for(off1, off2, traceback=False) == [2, 1]
    assert mod.release_workspaces() is None and mod.version() == 140 and mod.last_error() == "boom"
    assert rec.names() == [pre + "local_device", pre + "global_device", pre + "time_device"] + [pre + "slices_for"] * 4 + [
        pre + "release_workspaces", pre + "version", pre + "last_error"]
    local, glob, timer = (c[1] for c in rec.calls[:3])
    assert head(local) == head(glob) == head(timer[1:]) == (D1, D2, N, SM32.ctypes.data)      # pointers as given, the matrix where it lies
    assert local[6:] == (GO, GE, DS, DE, DM, DT, STREAM) and len(local) == 13
    assert glob[6:] == (GO, GE, MASK, DS, DE, None, None, 0) and len(glob) == 14               # ends-only, the default stream
    assert timer[0] == 1 and timer[7:-1] == (GO, GE, MASK, DS, DE, DM, DT, STREAM, 7) and len(timer) == 17
    for sym, p in ((pre + "local_device", 1), (pre + "global_device", 1), (pre + "time_device", 2)):
        assert rec.seen[sym, p] == off1.tolist() and rec.seen[sym, p + 2] == off2.tolist() and rec.seen[sym, p + 4] == SM32.tolist()
    count, fill, count0, fill0 = (c[1] for c in rec.calls[3:7])
    assert count[2:] == (N, 1, None, 0) and fill[2:4] == (N, 1) and fill[5] == 2 and count0[2:] == (N, 0, None, 0) and fill0[3] == 0
    assert rec.seen[pre + "slices_for", 0] == off1.tolist() and rec.seen[pre + "slices_for", 1] == off2.tolist()
    assert all(c[1] == () for c in rec.calls[7:])


def test_wide_long_stripe_waves_and_move_offsets(swmi_mod, monkeypatch):
    mod = swmi_mod.wide_long
    _, _, _, off1, _, off2 = _batch(0)
    rec = _inject(monkeypatch, mod, see={"swmi_wide_long_move_offsets": {0: (np.uint64, N + 1), 1: (np.uint64, N + 1)}})
    assert mod.set_stripe_waves(4) is None
    mo = mod.move_offsets(off1.tolist(), off2)
    assert (mo.dtype, mo.tolist()) == (np.uint64, LAID_OUT)
    assert rec.calls[0] == ("swmi_wide_long_set_stripe_waves", (4,))
    assert rec.calls[1][0] == "swmi_wide_long_move_offsets" and rec.calls[1][1][2:] == (N, mo.ctypes.data) and len(rec.calls) == 2
    assert rec.seen["swmi_wide_long_move_offsets", 0] == off1.tolist() and rec.seen["swmi_wide_long_move_offsets", 1] == off2.tolist()


# ---- ... swmi.wide_profile: one offsets array, the profile and len2 in the matrix's place

LEN2 = 7
PROFILE = ((np.arange(LEN2 * 32) % 23) - 11).astype(np.int8)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("kind", ["local", "global"])
def test_profile_host_entries(swmi_mod, monkeypatch, kind, traceback, which):
    mod, sym, layout = swmi_mod.wide_profile, "swmi_wide_profile_" + kind, "swmi_wide_profile_move_offsets"
    seqs, _, cat, off, _, _ = _batch(which)
    rec = _inject(monkeypatch, mod, see={sym: {0: (np.uint8, len(cat) or 16), 1: (np.uint64, N + 1), 3: (np.int8, LEN2 * 32)},
                                         layout: {0: (np.uint64, N + 1)}})
    if kind == "local":
        result = mod.local(seqs, PROFILE.reshape(LEN2, 32), GO, GE, traceback=traceback)
    else:
        result = mod.global_(seqs, PROFILE.reshape(LEN2, 32), GO, GE, free_ends=MASK, traceback=traceback)
    out = _check_results(result, traceback, LAID_OUT[-1])
    assert rec.names() == ([layout] if traceback else []) + [sym]
    args = rec.calls[-1][1]
    assert args[2:] == (N, PROFILE.ctypes.data, LEN2, GO, GE) + ((MASK,) if kind == "global" else ()) + out
    assert rec.seen[sym, 0] == _cat(cat) and rec.seen[sym, 1] == off.tolist()
    assert rec.seen[sym, 3] == PROFILE.tolist()
    if traceback:
        assert result[3].tolist() == LAID_OUT and rec.calls[0][1][1:] == (N, LEN2, result[3].ctypes.data)
        assert rec.seen[layout, 0] == off.tolist()


def test_profile_device_entries_timer_slices_and_the_rest(swmi_mod, monkeypatch):
    mod, pre = swmi_mod.wide_profile, "swmi_wide_profile_"
    _, _, _, off, _, _ = _batch(0)
    see = {pre + e: {p: (np.uint64, N + 1), p + 2: (np.int8, LEN2 * 32)} for e, p in (("local_device", 1), ("global_device", 1), ("time_device", 2))}
    see.update({pre + "slices_for": {0: (np.uint64, N + 1)}, pre + "move_offsets": {0: (np.uint64, N + 1)},
                pre + "from_sequence": {0: (np.uint8, 3), 2: (np.int8, 1024)}})
    rec = _inject(monkeypatch, mod, see=see)
    assert mod.local_device(D1, off, PROFILE, GO, GE, DS, DE, DM, DT, STREAM) is None
    assert mod.global_device(D1, off, PROFILE, GO, GE, MASK, DS, DE) is None
    assert mod.time_device(mod.LOCAL, D1, off, PROFILE, GO, GE, MASK, DS, DE, DM, DT, stream=STREAM, iters=7) == 1.5
    assert mod.slices_for(off, LEN2) == [2, 1] and mod.slices_for(off, LEN2, traceback=False) == [2, 1]
    mo = mod.move_offsets(off, LEN2)
    profile = mod.from_sequence([3, 1, 30], SM32)
    assert mo.tolist() == LAID_OUT and (profile.shape, profile.dtype) == ((3, 32), np.int8)
    assert mod.release_workspaces() is None and mod.version() == 140 and mod.last_error() == "boom"
    assert rec.names() == [pre + "local_device", pre + "global_device", pre + "time_device"] + [pre + "slices_for"] * 4 + [
        pre + "move_offsets", pre + "from_sequence", pre + "release_workspaces", pre + "version", pre + "last_error"]
    local, glob, timer = (c[1] for c in rec.calls[:3])
    assert local == (D1, local[1], N, PROFILE.ctypes.data, LEN2, GO, GE, DS, DE, DM, DT, STREAM)
    assert glob == (D1, glob[1], N, PROFILE.ctypes.data, LEN2, GO, GE, MASK, DS, DE, None, None, 0)
    assert timer[:-1] == (0, D1, timer[2], N, PROFILE.ctypes.data, LEN2, GO, GE, MASK, DS, DE, DM, DT, STREAM, 7) and len(timer) == 16
    for sym, p in ((pre + "local_device", 1), (pre + "global_device", 1), (pre + "time_device", 2)):
        assert rec.seen[sym, p] == off.tolist() and rec.seen[sym, p + 2] == PROFILE.tolist()
    count, fill, count0, fill0 = (c[1] for c in rec.calls[3:7])
    assert count[1:] == (N, LEN2, 1, None, 0) and fill[1:4] == (N, LEN2, 1) and fill[5] == 2 and count0[1:] == (N, LEN2, 0, None, 0)
    assert fill0[3] == 0 and rec.seen[pre + "slices_for", 0] == off.tolist()
    assert rec.calls[7][1][1:] == (N, LEN2, mo.ctypes.data) and rec.seen[pre + "move_offsets", 0] == off.tolist()
    query = rec.calls[8][1]
    assert query[1:] == (3, SM32.ctypes.data, profile.ctypes.data) and rec.seen[pre + "from_sequence", 0] == [3, 1, 30]
    assert rec.seen[pre + "from_sequence", 2] == SM32.tolist()
    assert all(c[1] == () for c in rec.calls[9:])
    empty = mod.from_sequence([], SM32)                       # no letters: no pointer to them either
    assert empty.shape == (0, 32) and rec.calls[-1][1] == (None, 0, SM32.ctypes.data, None)


# ---- ... swmi.banded_ragged and swmi.banded_width: the diagonals behind n, `band` only in the width library

DIAGONALS = np.array([3, -2, 0], np.int32)


class Pointer:
    """Anything with data_ptr(), as a torch tensor has."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("kind", ["local", "global"])
@pytest.mark.parametrize("name", ["banded_ragged", "banded_width"])
def test_banded_ragged_host_entries(swmi_mod, monkeypatch, name, kind, traceback, which):
    mod, sym = getattr(swmi_mod, name), "swmi_%s_%s" % (name, kind)
    band = (BAND,) if name == "banded_width" else ()
    seq1s, seq2s, cat1, off1, cat2, off2 = _batch(which)
    sm = 6 + len(band)
    rec = _inject(monkeypatch, mod, see={sym: {0: (np.uint8, len(cat1) or 16), 1: (np.uint64, N + 1), 2: (np.uint8, len(cat2)),
                                               3: (np.uint64, N + 1), 5: (np.int32, N), sm: (np.int8, 16)}})
    mask = {"free_ends": MASK} if kind == "global" else {}
    result = getattr(mod, kind if kind == "local" else "global_")(seq1s, seq2s, *band, SM4, GO, GE, diagonals=DIAGONALS, traceback=traceback, **mask)
    out = _check_results(result, traceback, WORDS[which][-1])
    assert rec.names() == [sym]
    args = rec.calls[0][1]
    assert args[4] == N and args[6:sm] == band and args[sm + 1:] == (GO, GE) + ((MASK,) if kind == "global" else ()) + out
    assert rec.seen[sym, 0] == _cat(cat1) and rec.seen[sym, 2] == cat2.tolist()
    assert rec.seen[sym, 1] == off1.tolist() and rec.seen[sym, 3] == off2.tolist()
    assert rec.seen[sym, 5] == DIAGONALS.tolist() and rec.seen[sym, sm] == SM4.tolist()
    if traceback:
        assert result[3].tolist() == WORDS[which]
    getattr(mod, kind if kind == "local" else "global_")(seq1s, seq2s, *band, SM4, GO, GE, traceback=False)
    assert rec.calls[1][1][5] is None                        # no diagonals: the main diagonal


@pytest.mark.parametrize("name", ["banded_ragged", "banded_width"])
def test_banded_ragged_device_entries_timer_slices_and_the_rest(swmi_mod, monkeypatch, name):
    mod, pre = getattr(swmi_mod, name), "swmi_%s_" % name
    band = (BAND,) if name == "banded_width" else ()
    b = len(band)
    _, _, _, off1, _, off2 = _batch(0)
    see = {pre + e: {p: (np.uint64, N + 1), p + 2: (np.uint64, N + 1), p + 4: (np.int32, N), p + 5 + b: (np.int8, 16)}
           for e, p in (("local_device", 1), ("global_device", 1), ("time_device", 2))}
    see[pre + "slices_for"] = {1 + b: (np.uint64, N + 1), 2 + b: (np.uint64, N + 1)}
    rec = _inject(monkeypatch, mod, see=see)
    assert mod.local_device(Pointer(D1), off1, Pointer(D2), off2, *band, SM4, GO, GE, Pointer(DS), Pointer(DE), Pointer(DM), Pointer(DT),
                            diagonals=DIAGONALS, stream=Pointer(STREAM)) is None
    assert mod.global_device(D1, off1, D2, off2, *band, SM4, GO, GE, MASK, DS, DE, diagonals=DIAGONALS) is None
    assert mod.time_device(mod.GLOBAL, D1, off1, D2, off2, *band, SM4, GO, GE, MASK, DS, DE, DM, DT, diagonals=DIAGONALS, stream=STREAM,
                           iters=7) == 1.5
    assert mod.slices_for(mod.GLOBAL, *band, off1, off2) == [2, 1] and mod.slices_for(mod.LOCAL, *band, off1, off2, traceback=False) == [2, 1]
    assert mod.release_workspaces() is None and mod.version() == 140 and mod.last_error() == "boom"
    assert rec.names() == [pre + "local_device", pre + "global_device", pre + "time_device"] + [pre + "slices_for"] * 4 + [
        pre + "release_workspaces", pre + "version", pre + "last_error"]
    local, glob, timer = (c[1] for c in rec.calls[:3])
    for args in (local, glob, timer[1:]):
        assert (args[0], args[2], args[4]) + args[6:6 + b] + args[7 + b:9 + b] == (D1, D2, N) + band + (GO, GE)
    assert local[9 + b:] == (DS, DE, DM, DT, STREAM) and glob[9 + b:] == (MASK, DS, DE, None, None, 0)
    assert timer[0] == 1 and timer[10 + b:-1] == (MASK, DS, DE, DM, DT, STREAM, 7) and len(timer) == 18 + b
    for sym, p in ((pre + "local_device", 1), (pre + "global_device", 1), (pre + "time_device", 2)):
        assert rec.seen[sym, p] == off1.tolist() and rec.seen[sym, p + 2] == off2.tolist()
        assert rec.seen[sym, p + 4] == DIAGONALS.tolist() and rec.seen[sym, p + 5 + b] == SM4.tolist()
    count, fill, count0, fill0 = (c[1] for c in rec.calls[3:7])
    assert count[:1 + b] == (1,) + band and count[3 + b:] == (N, 1, None, 0) and fill[3 + b:5 + b] == (N, 1) and fill[-1] == 2
    assert count0[:1 + b] == (0,) + band and count0[3 + b:] == (N, 0, None, 0) and fill0[4 + b] == 0
    assert rec.seen[pre + "slices_for", 1 + b] == off1.tolist() and rec.seen[pre + "slices_for", 2 + b] == off2.tolist()
    assert all(c[1] == () for c in rec.calls[7:])


# ---- ... swmi.banded and swmi.banded_global: one (len1, len2) per call, torch tensors on the device side

LEN1 = 5


class Tensor:
    """What the banded device wrappers read of a torch tensor of the device."""
    is_cuda = True

    def __init__(self, address, dtype, *shape):
        self.address, self.dtype, self.shape = address, dtype, shape

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.address


def _fixed(mod, name):
    if name == "banded":
        return mod.local, mod.local_device, "swmi_banded_local", ()
    return mod.align, mod.align_device, "swmi_banded_global", (MASK,)


@pytest.mark.parametrize("traceback", [True, False])
@pytest.mark.parametrize("name", ["banded", "banded_global"])
def test_banded_host_entries(swmi_mod, monkeypatch, name, traceback):
    mod = getattr(swmi_mod, name)
    host, _, sym, mask = _fixed(mod, name)
    a = (np.arange(N * LEN1).reshape(N, LEN1) % 4).astype(np.uint8)
    b = (np.arange(N * LEN2).reshape(N, LEN2) % 3).astype(np.uint8)
    rec = _inject(monkeypatch, mod, see={sym: {0: (np.uint8, N * LEN1), 2: (np.uint8, N * LEN2), 5: (np.int32, N), 6: (np.int8, 16)}})
    scores, ends, moves, steps = host(a, b, SM4, GO, GE, diagonals=DIAGONALS, traceback=traceback, **({"free_ends": MASK} if mask else {}))
    assert (scores.shape, scores.dtype) == ((N,), np.int32) and (ends.shape, ends.dtype) == ((N, 4), np.int32)
    if traceback:
        assert (moves.shape, moves.dtype) == ((N, 2), np.uint64) and (steps.shape, steps.dtype) == ((N,), np.uint32)     # 2 words for 5 + 7
    else:
        assert moves is None and steps is None
    assert rec.names() == [sym]
    args = rec.calls[0][1]
    assert (args[1],) + args[3:5] + args[7:] == (LEN1, LEN2, N, GO, GE) + mask + (
        scores.ctypes.data, ends.ctypes.data, moves.ctypes.data if traceback else None, steps.ctypes.data if traceback else None)
    assert rec.seen[sym, 0] == a.reshape(-1).tolist() and rec.seen[sym, 2] == b.reshape(-1).tolist()
    assert rec.seen[sym, 5] == DIAGONALS.tolist() and rec.seen[sym, 6] == SM4.tolist()
    host(a, b, SM4, GO, GE, traceback=False)
    assert rec.calls[1][1][5] is None


@pytest.mark.parametrize("name", ["banded", "banded_global"])
def test_banded_device_entries_timer_slices_and_the_rest(swmi_mod, monkeypatch, name):
    import torch
    mod, pre = getattr(swmi_mod, name), "swmi_%s_" % name
    _, device, sym, mask = _fixed(mod, name)
    sym += "_device"
    key = {"free_ends": MASK} if mask else {}
    rec = _inject(monkeypatch, mod, see={sym: {6: (np.int8, 16)}, pre + "time_device": {6: (np.int8, 16)}})
    seq1s, seq2s = Tensor(D1, torch.uint8, N, LEN1), Tensor(D2, torch.uint8, N, LEN2)
    scores, ends = Tensor(DS, torch.int32, N), Tensor(DE, torch.int32, N, 4)
    moves, steps, diagonals = Tensor(DM, torch.int64, N, 2), Tensor(DT, torch.int32, N), Tensor(0x8000, torch.int32, N)
    assert device(seq1s, seq2s, SM4, GO, GE, scores, ends, moves, steps, diagonals=diagonals, stream=STREAM, **key) is None
    assert device(seq1s, seq2s, SM4, GO, GE, scores, ends, stream=STREAM, **key) is None
    assert mod.time_device(seq1s, seq2s, SM4, GO, GE, scores, ends, moves, steps, diagonals=diagonals, stream=STREAM, iters=7, **key) == 1.5
    assert mod.slices_for(N, LEN1, LEN2) == [2, 1] and mod.slices_for(N, LEN1, LEN2, traceback=False) == [2, 1]
    assert mod.release_workspaces() is None and mod.version() == 140 and mod.last_error() == "boom"
    assert rec.names() == [sym, sym, pre + "time_device"] + [pre + "slices_for"] * 4 + [pre + "release_workspaces", pre + "version", pre + "last_error"]
    full, ends_only, timer = (c[1] for c in rec.calls[:3])
    assert full[:6] + full[7:] == (D1, LEN1, D2, LEN2, N, 0x8000, GO, GE) + mask + (DS, DE, DM, DT, STREAM)
    assert ends_only[:6] + ends_only[7:] == (D1, LEN1, D2, LEN2, N, None, GO, GE) + mask + (DS, DE, None, None, STREAM)
    assert timer[:6] + timer[7:-1] == (D1, LEN1, D2, LEN2, N, 0x8000, GO, GE) + mask + (DS, DE, DM, DT, STREAM, 7)
    assert rec.seen[sym, 6] == SM4.tolist() and rec.seen[pre + "time_device", 6] == SM4.tolist()
    count, fill, count0, fill0 = (c[1] for c in rec.calls[3:7])
    assert count == (N, LEN1, LEN2, 1, None, 0) and fill[:4] == (N, LEN1, LEN2, 1) and fill[5] == 2
    assert count0 == (N, LEN1, LEN2, 0, None, 0) and fill0[:4] == (N, LEN1, LEN2, 0)
    assert all(c[1] == () for c in rec.calls[7:])


# ---- refusals before any call, a failed call, a missing library

def _host_calls(swmi_mod, name):
    """[(a call of the host wrapper(s) with **changes applied, taking score_matrix / gap_open / free_ends / diagonals)]."""
    mod = getattr(swmi_mod, name)
    seq1s, seq2s = _batch(0)[:2]
    if name in ("wide", "wide_long"):
        return [lambda sm=SM32, go=GO, **k: mod.local(seq1s, seq2s, sm, go, GE), lambda sm=SM32, go=GO, **k: mod.global_(seq1s, seq2s, sm, go, GE, **k)]
    if name == "wide_profile":
        return [lambda sm=PROFILE, go=GO, **k: mod.local(seq1s, sm, go, GE), lambda sm=PROFILE, go=GO, **k: mod.global_(seq1s, sm, go, GE, **k)]
    if name in ("banded_ragged", "banded_width"):
        band = (BAND,) if name == "banded_width" else ()
        return [lambda sm=SM4, go=GO, free_ends=0, **k: mod.local(seq1s, seq2s, *band, sm, go, GE, **k),
                lambda sm=SM4, go=GO, **k: mod.global_(seq1s, seq2s, *band, sm, go, GE, **k)]
    a, b = np.zeros((N, LEN1), np.uint8), np.zeros((N, LEN2), np.uint8)
    if name == "banded":
        return [lambda sm=SM4, go=GO, free_ends=0, **k: mod.local(a, b, sm, go, GE, **k)]
    return [lambda sm=SM4, go=GO, **k: mod.align(a, b, sm, go, GE, **k)]


@pytest.mark.parametrize("name", MODULES)
def test_refusals_come_before_any_call(swmi_mod, monkeypatch, name):
    rec = _inject(monkeypatch, getattr(swmi_mod, name))
    calls = _host_calls(swmi_mod, name)
    what = "profile" if name == "wide_profile" else "score_matrix"
    for call in calls:
        with pytest.raises(swmi_mod.SwmiError, match=r"swmi error -5: gap_open 2147483648 is outside the supported domain \[0,127\]") as e:
            call(go=2**31)
        assert e.value.code == swmi_mod.ERR_DOMAIN == -5
        bad = np.full(7 * 32 if name == "wide_profile" else 1024 if name.startswith("wide") else 16, -3, np.int64)
        bad[5] = 200
        with pytest.raises(swmi_mod.SwmiError, match=r"swmi error -5: %s entries must lie in \[-128, 127\] \(got -3\.\.200\)" % what) as e:
            call(sm=bad)
        assert e.value.code == swmi_mod.ERR_DOMAIN == -5
    if name != "banded":                                                       # its one entry takes no mask
        with pytest.raises(ValueError, match="invalid literal for int"):       # a mask is whatever int() takes; the C side checks its bits
            calls[-1](free_ends="fit")
        with pytest.raises(TypeError):
            calls[-1](free_ends=None)
    if name == "wide_profile":
        with pytest.raises(ValueError, match=r"profile must have len2 \* 32 entries"):
            calls[0](sm=PROFILE[:-1])
    if name.startswith("banded"):
        for call in calls:
            with pytest.raises(ValueError, match="diagonals must hold one entry per alignment"):
                call(diagonals=[1, 2])
    assert rec.calls == []


@pytest.mark.parametrize("name", MODULES)
def test_a_negative_return_raises_with_the_library_s_text(swmi_mod, monkeypatch, name):
    mod = getattr(swmi_mod, name)
    rec = _inject(monkeypatch, mod, rc={"swmi_%s_release_workspaces" % name: -3})
    with pytest.raises(swmi_mod.SwmiError, match="^swmi error -3: boom$") as e:
        mod.release_workspaces()
    assert e.value.code == -3 and rec.names() == ["swmi_%s_release_workspaces" % name, "swmi_%s_last_error" % name]
    check = getattr(mod, "_check", None) or _holder(mod).check
    assert check(0) == 0 and check(5) == 5 and len(rec.calls) == 2
    with pytest.raises(swmi_mod.SwmiError, match="^swmi error -3: boom$"):
        check(-3)


@pytest.mark.parametrize("name", MODULES)
def test_a_missing_library_is_an_error_of_load_not_of_import(name):
    """A fresh process whose variable names no file: the package imports, and load() raises with the path it looked at."""
    lib, env = LIBRARY[name]
    missing = "/nonexistent/" + lib
    code = ("import swmi\n"
            "assert swmi.%s.LIB_PATH == %r\n"
            "try:\n"
            "    swmi.%s.load()\n"
            "except swmi.SwmiError as e:\n"
            "    print(e.code == swmi.ERR_NOT_INITIALIZED, e)\n" % (name, missing, name))
    run = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=PKG, **{env: missing}), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout == ("True swmi error -1: %s not built: run __graft_entry__.build() or make -C smith-waterman-simd_amd/csrc\n" % missing)
