"""swmi.banded and swmi.banded_global after their bodies moved into swmi/_banded_binding.py: every public
name they had is still there with the signature it had (listed literally, as inspect.signature printed them before the move),
slices_for gives what it gave, and the shared _diagonals refuses what it refused.  Likewise swmi.banded_ragged and swmi.banded_width
after their bodies moved into swmi/_banded_ragged_binding.py (section 39), `band` directly before score_matrix.  No device needed."""
import inspect
import os

import numpy as np
import pytest

COMMON = {
    "last_error": "()",
    "load": "()",
    "move_words": "(len1, len2)",
    "paths": "(result)",
    "release_workspaces": "()",
    "slices_for": "(n, len1, len2, traceback=True)",
    "version": "()",
}
SIGNATURES = {
    "banded": dict(COMMON, **{
        "local": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True)",
        "local_device": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, "
                        "stream=None)",
        "time_device": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, diagonals=None, "
                       "stream=None, iters=10)",
    }),
    "banded_global": dict(COMMON, **{
        "align": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True)",
        "align_device": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, "
                        "diagonals=None, stream=None)",
        "time_device": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, scores, ends, moves=None, steps=None, free_ends=0, "
                       "diagonals=None, stream=None, iters=10)",
    }),
}
CONSTANTS = {
    "banded": {"ERR_NOT_INITIALIZED": -1, "HI": 63, "LO": -64, "MAX_LEN": 16384, "WIDTH": 128},
    "banded_global": {"ERR_NOT_INITIALIZED": -1, "HI": 63, "LO": -64, "MAX_LEN": 16384, "WIDTH": 128, "END_ANYWHERE": 16,
                      "ENDS_EXTEND": 16, "NO_ALIGNMENT": -2147483648},
}
LIBRARY = {"banded": "libswmi_banded.so", "banded_global": "libswmi_banded_global.so"}
# (n, len1, len2, traceback) -> the slices, recorded before the move; the two libraries cut alike
SLICES = [(((2 << 20) + 7, 1, 1, False), [1048576, 1048576, 7]),
          ((37, 70, 33, True), [37]),
          ((5000, 16384, 128, True), [4084, 916])]


RAGGED_COMMON = {
    "last_error": "()",
    "load": "()",
    "move_offsets": "(seq1_offsets, seq2_offsets)",
    "paths": "(result)",
    "release_workspaces": "()",
    "version": "()",
}
RAGGED_SIGNATURES = {
    "banded_ragged": dict(RAGGED_COMMON, **{
        "local": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True)",
        "global_": "(seq1s, seq2s, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True)",
        "local_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, d_scores, d_ends, d_moves=None, "
                        "d_steps=None, diagonals=None, stream=0)",
        "global_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends, "
                         "d_moves=None, d_steps=None, diagonals=None, stream=0)",
        "time_device": "(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends, "
                       "d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10)",
        "slices_for": "(kind, seq1_offsets, seq2_offsets, traceback=True)",
    }),
    "banded_width": dict(RAGGED_COMMON, **{
        "local": "(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, diagonals=None, traceback=True)",
        "global_": "(seq1s, seq2s, band, score_matrix, gap_open, gap_extend, free_ends=0, diagonals=None, traceback=True)",
        "local_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, d_scores, d_ends, "
                        "d_moves=None, d_steps=None, diagonals=None, stream=0)",
        "global_device": "(d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, d_ends, "
                         "d_moves=None, d_steps=None, diagonals=None, stream=0)",
        "time_device": "(kind, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, band, score_matrix, gap_open, gap_extend, free_ends, d_scores, "
                       "d_ends, d_moves=None, d_steps=None, diagonals=None, stream=0, iters=10)",
        "slices_for": "(kind, band, seq1_offsets, seq2_offsets, traceback=True)",
    }),
}
RAGGED_SHARED = {"ERR_NOT_INITIALIZED": -1, "LOCAL": 0, "GLOBAL": 1, "MAX_LEN": 16384, "SLOT_BYTES": 48, "END_ANYWHERE": 16,
                 "NO_ALIGNMENT": -2147483648}
RAGGED_CONSTANTS = {
    "banded_ragged": dict(RAGGED_SHARED, WIDTH=128, LO=-64, HI=63),
    "banded_width": dict(RAGGED_SHARED, WIDTHS=(128, 256, 512, 1024)),
}
RAGGED_LIBRARY = {"banded_ragged": ("libswmi_banded_ragged.so", "SWMI_BANDED_RAGGED_LIB"),
                  "banded_width": ("libswmi_banded_width.so", "SWMI_BANDED_WIDTH_LIB")}
# (n, len1, len2, traceback) of a uniform batch -> the slices at band 128 (the ragged library's), 256, 512 and 1024, recorded
# before the move; the two kinds cut alike here
RAGGED_SLICES = [(((2 << 20) + 7, 1, 1, False), [[1048576, 1048576, 7]] * 4),
                 ((37, 70, 33, True), [[37]] * 4),
                 ((5000, 16384, 128, True), [[4084, 916], [2061, 2061, 878], [1036] * 4 + [856], [519] * 9 + [329]])]


@pytest.mark.parametrize("name", ["banded_ragged", "banded_width"])
def test_ragged_public_names_and_signatures(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    for fn, sig in RAGGED_SIGNATURES[name].items():
        f = getattr(mod, fn)
        assert inspect.isfunction(f) and f.__module__ == "swmi." + name and f.__doc__, fn
        assert str(inspect.signature(f)) == sig, fn
    for const, value in RAGGED_CONSTANTS[name].items():
        assert getattr(mod, const) == value, const
    assert mod.SwmiError is swmi_mod.SwmiError and mod.local_full_expand_moves is swmi_mod.local_full_expand_moves
    assert mod.local_full_ragged_move_offsets is swmi_mod.local_full_ragged_move_offsets
    lib, env = RAGGED_LIBRARY[name]
    assert mod.LIB_PATH == os.environ.get(env, mod.LIB_PATH) and (env in os.environ or mod.LIB_PATH.endswith("/lib/" + lib))
    assert not hasattr(swmi_mod.banded_ragged, "WIDTHS") and not hasattr(swmi_mod.banded_width, "WIDTH")


@pytest.mark.parametrize("name", ["banded_ragged", "banded_width"])
def test_ragged_slices_for_gives_the_recorded_slices(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    for (n, len1, len2, traceback), want in RAGGED_SLICES:
        off1, off2 = np.arange(n + 1, dtype=np.uint64) * len1, np.arange(n + 1, dtype=np.uint64) * len2
        for kind in (mod.LOCAL, mod.GLOBAL):
            if name == "banded_ragged":
                assert mod.slices_for(kind, off1, off2, traceback=traceback) == want[0]
            else:
                for band, slices in zip(mod.WIDTHS, want):
                    assert mod.slices_for(kind, band, off1, off2, traceback=traceback) == slices, band


@pytest.mark.parametrize("name", ["banded", "banded_global"])
def test_public_names_and_signatures(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    for fn, sig in SIGNATURES[name].items():
        f = getattr(mod, fn)
        assert inspect.isfunction(f) and f.__module__ == "swmi." + name and f.__doc__, fn
        assert str(inspect.signature(f)) == sig, fn
    for const, value in CONSTANTS[name].items():
        assert getattr(mod, const) == value, const
    assert mod.SwmiError is swmi_mod.SwmiError and mod.local_full_expand_moves is swmi_mod.local_full_expand_moves
    assert mod.LIB_PATH.endswith("/lib/" + LIBRARY[name])


@pytest.mark.parametrize("name", ["banded", "banded_global"])
def test_slices_for_gives_the_recorded_slices(swmi_mod, name):
    mod = getattr(swmi_mod, name)
    for (n, len1, len2, traceback), want in SLICES:
        assert mod.slices_for(n, len1, len2, traceback=traceback) == want


def test_diagonals_refuses_a_wrong_shape_and_a_value_outside_int32(swmi_mod):
    from swmi._banded_binding import _diagonals
    assert _diagonals(None, 3) is None
    d = _diagonals([1, -2, 3], 3)
    assert d.dtype == np.int32 and d.tolist() == [1, -2, 3]
    assert _diagonals(np.array([-2**31, 2**31 - 1], np.int64), 2).tolist() == [-2**31, 2**31 - 1]
    for bad in ([1, 2], [[1, 2, 3]], 5):
        with pytest.raises(ValueError, match="one entry per alignment"):
            _diagonals(bad, 3)
    for bad in ([0, 2**31, 0], [-2**31 - 1, 0, 0]):
        with pytest.raises(ValueError, match="must be int32"):
            _diagonals(bad, 3)
