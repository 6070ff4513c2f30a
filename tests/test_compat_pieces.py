"""include/swmi_compat.hpp's batch overloads over stub C entries, no device and no library: tests/native/compat_pieces.cpp,
compiled with g++ and ASan + UBSan, defines the aligners, expanders and swmi_last_error the overloads call, with results
derived from an index in each seq2.  For each overload it checks every result over several pieces, the pieces and moves
buffers the aligner sees, and that a failing aligner call or expansion (on 3 host threads for the semi-global overloads)
surfaces as std::runtime_error with the stub's message while the program goes on.  For the overloads with one (len1, len2)
per batch (long, long_affine, nw, sg_affine) also that a piece is capped at the slice their *_slices_for reports, that nw's
mask reaches every piece, and that a length the library refuses surfaces with its message before any piece is aligned."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

OVERLOADS = ["local", "affine", "ragged", "affine_ragged", "long_ragged", "xdrop", "sgfull", "long", "long_affine", "nw", "sg_affine"]


@pytest.fixture(scope="module")
def pieces_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("compat_pieces")
    exe = str(tmp / "compat_pieces")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-I", os.path.join(ROOT, "include"), "-o", exe,
                                          os.path.join(ROOT, "tests", "native", "compat_pieces.cpp"), "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


@pytest.mark.parametrize("overload", OVERLOADS)
def test_batch_overload_pieces(pieces_exe, overload):
    r = subprocess.run([pieces_exe, overload], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "compat pieces ok" in r.stdout
    assert r.stdout.count(": ok") == 5
