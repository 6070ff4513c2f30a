"""The host side of the three kinds of ragged aligner on the wavefront-tiled sweep -- local (swmi_local_full[_affine]_ragged*),
global / fit / overlap (swmi_global_full[_affine]_ragged*) and exact semi-global (swmi_semiglobal_full[_affine]_ragged*):
csrc/tile_ragged_api.cpp through the slice pipeline of csrc/swmi_table.cpp -- on a fake GPU, no device needed: the real host
sources (every csrc/swmi_*.cpp, table_api.cpp and tile_ragged_api.cpp), compiled once with g++ and ASan + UBSan as a
stand-alone program against tests/native/fake_hip.cpp and tests/native/tile_ragged_host_fake.cpp, which holds the stand-ins for
the six ragged launchers and the checks, and runs one kind per invocation: every result at its caller position, with the
kind's four or two ends per alignment and a sentinel pair behind them that survives; zero-length slots in the W = 1 launch
with the kind's stated result, no code words and their move words inside their rows; the global kind's mask folded into every
score; a slice's launches in descending wave count covering each slot once, and no fixed-length launcher; one move copy per
slice of exactly its words; the device entry growing its workspace on two streams; and the plan alone, with the real code
words, for 300 alignments of 16384 x 16384 with affine traceback (code bases past 2^32)."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def fake_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("tile_ragged_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "tile_ragged_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [
        os.path.join(PKG, "csrc", name) for name in ("table_api.cpp", "tile_ragged_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "tile_ragged_host_fake.cpp"),
                                          os.path.join(native, "fake_hip.cpp")] + host_sources + ["-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


@pytest.mark.parametrize("kind", ["local", "global", "semiglobal"])
def test_tile_ragged_host_paths(fake_exe, kind):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([fake_exe, kind], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "tile ragged host fake ok: %s\n" % kind in r.stdout
    # the plan-only case, 16 + 1 host cases, 6 device cases, then 1 host case after the release
    assert r.stdout.count(": ok") == 25
