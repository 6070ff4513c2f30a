"""The host side of the ragged local aligners (local_ragged_api.cpp through the slice pipeline of swmi_table.cpp) on a fake GPU,
no device needed: the real host sources compiled with g++ and ASan + UBSan against tests/native/fake_hip.cpp, with the ragged
launchers' stand-ins in tests/native/ragged_host_fake.cpp.  It checks every result at its caller position, the slots of every
launch (longest first, each alignment once, its seq1 where the slot says), one move copy per slice of exactly its alignments'
words, both buffer sets in flight, and the device entry growing its workspace on two streams."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def ragged_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("ragged_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "ragged_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [
        os.path.join(PKG, "csrc", "table_api.cpp"), os.path.join(PKG, "csrc", "local_ragged_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "ragged_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


def test_ragged_host_paths(ragged_exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([ragged_exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ragged host fake ok" in r.stdout
    assert r.stdout.count(": ok") == 7
