"""The local aligner with traceback (swmi_local_*, include/swmi.h) without a device: the fixture F7 (what the reference's
SmithWaterman_111_long returned) against the C restatement tests/native/local_oracle.c, the restatement's scores against
F1/F4, the C ABI surface, its argument errors, the moves expander, the slicing rule and the C++ header."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_support import LocalOracle, f7_by_length, load_f7, move_words, moves_to_path, path_to_moves

NEW_SYMBOLS = ("swmi_local_align", "swmi_local_align_device", "swmi_local_slices_for", "swmi_local_expand_moves",
               "swmi_local_time_device")


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def test_f7_covers_every_length_and_kind():
    f7 = load_f7()
    assert {v["len1"] for v in f7} == {1, 2, 63, 64, 127, 128, 129, 300, 1000, 4096, 16384}
    assert {v["kind"] for v in f7} == {"random", "similar85", "identical", "mismatch", "homopolymer", "tandem", "indel"}
    assert any(v["score"] == 0 for v in f7) and max(v["score"] for v in f7) == 128


def test_restatement_reproduces_f7_field_for_field(loracle):
    """Score, end cell, start cell and the whole path of every F7 vector (the reference's own (1,1,1) function)."""
    for len1, (a, b, scores, paths) in f7_by_length().items():
        sc, ends, moves, steps = loracle.align(a, b, match_matrix(1, -1), 1)
        for k in range(len(scores)):
            want = paths[k]
            assert sc[k] == scores[k], (len1, k)
            assert tuple(ends[k, :2]) == tuple(want[-1]) and tuple(ends[k, 2:]) == tuple(want[0]), (len1, k)
            assert steps[k] + 1 == len(want), (len1, k)
            assert np.array_equal(moves_to_path(moves[k], steps[k], ends[k, 0], ends[k, 1]), want), (len1, k)


@pytest.mark.parametrize("name", ["f1_random", "f4_param_sweep"])
def test_restatement_scores_equal_the_128x128_fixtures(loracle, golden, name):
    """At len1 = 128 the local score is the 128 x 128 scorer's score, for every parameter set of F1 / F4.  (Ends and paths
    for matrices other than (1,1,1) rest on the stated tie rule alone: the reference has no such function.)"""
    f = golden(name)
    for p in range(len(f["gap"])):
        sc, _, _, _ = loracle.align(f["seq1"], f["seq2"], f["sm"][p], int(f["gap"][p]))
        assert np.array_equal(sc, f["scores"][p]), (name, p)


def test_every_new_symbol_is_declared_and_exported():
    import re
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def test_argument_errors_without_a_device(swmi_mod):
    lib = swmi_mod.load()
    sm = match_matrix(1, -1)
    a = np.zeros((2, 128), np.uint8)
    b = np.zeros((2, 128), np.uint8)
    sc = np.zeros(2, np.int32)
    ends = np.zeros((2, 4), np.int32)
    mv = np.zeros((2, move_words(128)), np.uint64)
    st = np.zeros(2, np.uint32)
    P = lambda x: x.ctypes.data  # noqa: E731

    def call(len1=128, s1=P(a), gap=1, moves=P(mv), steps=P(st), m=P(sm), scores=P(sc)):
        return lib.swmi_local_align(s1, len1, P(b), 2, m, gap, scores, P(ends), moves, steps)
    assert call(len1=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len1=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(gap=-1) == swmi_mod.ERR_DOMAIN
    assert call(s1=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(m=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(scores=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(steps=None) == swmi_mod.ERR_INVALID_ARGUMENT            # moves without steps
    assert call(moves=None) == swmi_mod.ERR_INVALID_ARGUMENT            # steps without moves
    assert lib.swmi_local_align_device(P(a), 0, P(b), 2, P(sm), 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert lib.swmi_local_align_device(P(a), 128, P(b), 2, P(sm), -3, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert lib.swmi_local_align_device(P(a), 128, P(b), 2, P(sm), 1, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_align(a, b, sm, 300)                             # ctypes would wrap it to an int8
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_expand_moves_round_trips_f7_paths(swmi_mod):
    for v in load_f7():
        path = v["path"]
        row = path_to_moves(path, move_words(v["len1"]))
        got = swmi_mod.local_expand_moves(row, len(path) - 1, path[-1][0], path[-1][1])
        assert np.array_equal(got, path)
        head = swmi_mod.local_expand_moves(row, len(path) - 1, path[-1][0], path[-1][1], cap=1)
        assert np.array_equal(head, path[:1])
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.local_expand_moves(np.full(2, 0xFFFFFFFF, np.uint64), 40, 3, 3)     # would leave the matrix


@pytest.mark.parametrize("len1", [1, 128, 1000, 16384])
@pytest.mark.parametrize("traceback", [True, False])
def test_slices_cover_every_alignment_within_the_bound(swmi_mod, len1, traceback):
    per = len1 + 128 + 4 + 16
    if traceback:
        per += 4 * 64 * ((len1 + 15 + 7) // 8) + 8 * move_words(len1) + 4
    for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
        sizes = swmi_mod.local_slices_for(n, len1, traceback)
        assert sum(sizes) == n and all(s >= 1 for s in sizes)
        assert all(s * per <= 256 << 20 for s in sizes)
        assert all(s == sizes[0] for s in sizes[:-1]) and (not sizes or sizes[-1] <= sizes[0])
    assert swmi_mod.local_slices_for(10, 0) == [] and swmi_mod.local_slices_for(10, 16385) == []
    assert len(swmi_mod.local_slices_for(600, 16384, True)) > 1


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local.cpp"), "-o", str(tmp_path / "compat_local"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
