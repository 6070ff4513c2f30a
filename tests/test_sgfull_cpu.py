"""The exact semi-global aligner (swmi_semiglobal_full*, include/swmi.h) without a device: the fixture F8 (what the
reference's SemiGlobal_111 returned) against the C restatement tests/native/sgfull_oracle.c, the restatement against an
independent numpy formulation, the exact-vs-X-drop scores F8 pins, the C ABI surface, its argument errors, the slicing
rule, the moves expander on F8's paths and the C++ header."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT, match_matrix
from local_support import PARAMS
from sgfull_support import K111, SgFullOracle, load_f8, move_words, moves_to_path, numpy_sgfull, path_to_moves

NEW_SYMBOLS = ("swmi_semiglobal_full", "swmi_semiglobal_full_device", "swmi_semiglobal_full_slices_for",
               "swmi_semiglobal_full_release_workspaces", "swmi_semiglobal_full_time_device")


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


def test_f8_holds_the_f6_inputs_and_every_kind(golden):
    f8, f6 = load_f8(), golden("f6_semiglobal")
    assert np.array_equal(f8["seq1"][:16], f6["seq1"]) and np.array_equal(f8["seq2"][:16], f6["seq2"])
    assert set(f8["kind"]) == {"f6", "identical", "mismatch", "homopolymer", "shifted", "deletion20", "deletion60",
                               "deletion100", "deletion400", "insertion100", "random"}
    # where the X-drop aligner found the exact answer its score is F6's
    assert np.array_equal(f8["xdrop_scores"][:16], f6["scores"])


def test_restatement_reproduces_f8_field_for_field(sgoracle):
    f8 = load_f8()
    sc, ends, moves, lengths = sgoracle.align(f8["seq1"], f8["seq2"], K111, 1)
    for k in range(len(f8["scores"])):
        assert sc[k] == f8["scores"][k], k
        assert tuple(ends[k]) == tuple(f8["ends"][k]) == tuple(f8["paths"][k][-1]), k
        assert lengths[k] == f8["lengths"][k] == len(f8["paths"][k]), k
        assert np.array_equal(moves_to_path(moves[k], lengths[k], ends[k, 0], ends[k, 1]), f8["paths"][k]), k
    mm = f8["kind"].index("mismatch")
    assert sc[mm] == 0 and tuple(ends[mm]) == (0, 0) and lengths[mm] == 1


def test_restatement_matches_numpy_on_small_sizes(sgoracle):
    rng = np.random.default_rng(31)
    for p, (match, mismatch, gap) in enumerate(PARAMS):
        sm = match_matrix(match, mismatch)
        for len1, len2 in ((1, 1), (1, 7), (9, 1), (5, 13), (17, 17), (40, 23)):
            a = rng.integers(0, 4, (6, len1), dtype=np.uint8)
            b = rng.integers(0, 4, (6, len2), dtype=np.uint8)
            b[0, : min(len1, len2)] = a[0, : min(len1, len2)]              # one similar pair
            a[1] = 0
            b[1] = 1                                                      # one all-mismatch pair
            sc, ends, moves, lengths = sgoracle.align(a, b, sm, gap)
            sc2, ends2, _, _ = sgoracle.align(a, b, sm, gap, traceback=False)
            assert np.array_equal(sc, sc2) and np.array_equal(ends, ends2)
            for k in range(6):
                want_score, want_end, want_path = numpy_sgfull(a[k], b[k], sm, gap)
                assert sc[k] == want_score and tuple(ends[k]) == want_end, (p, len1, len2, k)
                assert np.array_equal(moves_to_path(moves[k], lengths[k], ends[k, 0], ends[k, 1]), want_path), (p, len1, len2, k)


def test_exact_scores_bound_the_xdrop_scores_of_f8():
    """The exact table can only score at least as high as the adaptive band; one indel longer than the band costs the band
    a large part of its score."""
    f8 = load_f8()
    assert np.all(f8["scores"] >= f8["xdrop_scores"])
    for kind in ("deletion60", "deletion100", "deletion400"):
        k = f8["kind"].index(kind)
        assert f8["scores"][k] > f8["xdrop_scores"][k], kind
    k = f8["kind"].index("deletion20")
    assert f8["scores"][k] == f8["xdrop_scores"][k] == 16344


def test_every_new_symbol_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "swmi.h")).read()
    declared = set(re.findall(r"SWMI_API\s+[^;(]*?\b(swmi_\w+)\s*\(", text))
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libswmi.so"))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name), name


def test_argument_errors_without_a_device(swmi_mod):
    lib = swmi_mod.load()
    sm = match_matrix(1, -1)
    a = np.zeros((2, 64), np.uint8)
    b = np.zeros((2, 64), np.uint8)
    sc = np.zeros(2, np.int32)
    ends = np.zeros((2, 2), np.int32)
    mv = np.zeros((2, move_words(64, 64)), np.uint64)
    ln = np.zeros(2, np.uint32)
    P = lambda x: x.ctypes.data  # noqa: E731

    def call(len1=64, len2=64, s1=P(a), s2=P(b), gap=1, moves=P(mv), lengths=P(ln), m=P(sm), scores=P(sc), e=P(ends)):
        return lib.swmi_semiglobal_full(s1, len1, s2, len2, 2, m, gap, scores, e, moves, lengths)
    assert call(len1=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=0) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len1=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(len2=16385) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(gap=-1) == swmi_mod.ERR_DOMAIN
    assert call(s1=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(s2=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(m=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(scores=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(e=None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert call(lengths=None) == swmi_mod.ERR_INVALID_ARGUMENT          # moves without lengths
    assert call(moves=None) == swmi_mod.ERR_INVALID_ARGUMENT            # lengths without moves
    dev = lib.swmi_semiglobal_full_device
    assert dev(P(a), 0, P(b), 64, 2, P(sm), 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 16385, 2, P(sm), 1, P(sc), P(ends), None, None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    assert dev(P(a), 64, P(b), 64, 2, P(sm), -3, P(sc), P(ends), None, None, None) == swmi_mod.ERR_DOMAIN
    assert dev(P(a), 64, P(b), 64, 2, P(sm), 1, P(sc), P(ends), P(mv), None, None) == swmi_mod.ERR_INVALID_ARGUMENT
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.semiglobal_full(a, b, sm, 300)                        # ctypes would wrap it to an int8
    # valid arguments and no device: an error, never a CPU answer
    if lib.swmi_num_gpus() == 0:
        assert call() in (swmi_mod.ERR_NOT_INITIALIZED, swmi_mod.ERR_NO_DEVICE)


def test_slices_for(swmi_mod):
    full = lambda n, tb=True: swmi_mod.semiglobal_full_slices_for(n, 16384, 16384, tb)  # noqa: E731
    assert full(0) == [] and full(1) == [1] and full(256) == [256] and full(257) == [256, 1]
    assert full(1000) == [256, 256, 256, 232]
    # ends-only slices are bounded by their inputs only (256 MiB)
    per = 16384 + 16384 + 12
    sizes = full(100000, False)
    assert sum(sizes) == 100000 and sizes[0] == (256 << 20) // per and all(s <= sizes[0] for s in sizes)
    for len1, len2 in ((1, 1), (63, 65), (1000, 1000), (4096, 777), (16384, 1)):
        for tb in (True, False):
            for n in (0, 1, 3, 4097, 1 << 20, 3 * (1 << 20) + 5):
                s = swmi_mod.semiglobal_full_slices_for(n, len1, len2, tb)
                assert sum(s) == n and all(x >= 1 for x in s) and all(x == s[0] for x in s[:-1])
                assert all(x <= 1 << 20 for x in s)
    assert swmi_mod.semiglobal_full_slices_for(10, 0, 5) == [] and swmi_mod.semiglobal_full_slices_for(10, 5, 16385) == []


def test_expand_moves_rebuilds_f8_paths(swmi_mod):
    f8 = load_f8()
    for k, path in enumerate(f8["paths"]):
        row = path_to_moves(path, move_words(16384, 16384))
        assert np.array_equal(swmi_mod.semiglobal_expand_moves(row, len(path)), path), k
        assert np.array_equal(moves_to_path(row, len(path), path[-1][0], path[-1][1]), path), k


def test_cpp_header_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_sgfull.cpp"), "-o", str(tmp_path / "compat_sgfull"),
                            "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
