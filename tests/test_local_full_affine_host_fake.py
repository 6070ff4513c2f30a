"""The host side of the any-length affine local aligner (swmi_local_full_affine*: local_full_affine_api.cpp through the slice
pipeline of swmi_table.cpp) on a fake GPU, no device needed: the real host sources (every csrc/swmi_*.cpp and
local_full_affine_api.cpp), compiled with g++ and ASan + UBSan against tests/native/fake_hip.cpp and
tests/native/local_full_affine_host_fake.cpp, which holds the stand-in for the launcher that fake_hip.cpp does not know and the
checks: the argument checks in the header's order, n = 0 and the slice sizes worked out by hand before any device exists, the
host entry (traceback and ends-only at n = 1, one slice,
one slice + 1 and two and a half slices: every result, the move words each slice copies back, the launches and their
streams), the device entry on two streams with a workspace that grows, the timer, the release of the workspaces and the entries after swmi_shutdown.  And the C++ overloads compile and link."""
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
    tmp = tmp_path_factory.mktemp("local_full_affine_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "local_full_affine_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [os.path.join(PKG, "csrc", "local_full_affine_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "local_full_affine_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


def test_local_full_affine_host_paths(fake_exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([fake_exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "local_full_affine host fake ok" in r.stdout
    # 2 lines before a device exists, 8 host cases, 5 device cases, the timer, then 1 device case, 1 host case, the release
    # line and the one after the shutdown
    assert r.stdout.count(": ok") == 20


def test_cpp_overloads_compile_and_link(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "compat_local_full_affine.cpp")
    syntax = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert syntax.returncode == 0, syntax.stdout
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o",
                            str(tmp_path / "compat_local_full_affine"), "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
