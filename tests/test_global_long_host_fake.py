"""The host side of the long global / fit / overlap aligners (swmi_global_long*, swmi_global_long_affine*: global_long_api.cpp
and global_long_affine_api.cpp through the slice pipeline of swmi_table.cpp) on a fake GPU, no device needed: the real host
sources (every csrc/swmi_*.cpp, the two fixed-length global api files that the long ones build on, and the two long ones),
compiled with g++ as a stand-alone program under ASan + UBSan against tests/native/fake_hip.cpp and
tests/native/global_long_host_fake.cpp, which holds the stand-ins for the four launchers and the checks: the refusals before
anything is launched (lengths 0 and 65537, a mask of 16, NULLs, one of moves / steps, the domain rule from both sides of its
edge), linear and affine host entries with n across a slice boundary, the mask, the launcher and the carry pointer in every
slice's launch, the carry's size (the stand-in touches its last dword), and the device entry's workspace with the carry
counted."""
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
    tmp = tmp_path_factory.mktemp("global_long_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "global_long_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [
        os.path.join(PKG, "csrc", name) for name in ("global_full_api.cpp", "global_full_affine_api.cpp", "global_long_api.cpp",
                                                     "global_long_affine_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "global_long_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


def test_global_long_host_paths(fake_exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([fake_exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "global_long host fake ok" in r.stdout
    assert "refused, nothing launched" in r.stdout and "accepted" in r.stdout
    # per family 8 host cases and 4 device cases, then 2 host cases and the release line
    assert r.stdout.count(": ok") == 2 * 12 + 3
