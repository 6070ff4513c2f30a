"""The host side of the affine global / free-end-gap aligner (swmi_global_full_affine*: global_full_affine_api.cpp through the
slice pipeline of swmi_table.cpp) on a fake GPU, no device needed: the real host sources (every csrc/swmi_*.cpp and
global_full_affine_api.cpp), compiled with g++ as a stand-alone program under ASan + UBSan against tests/native/fake_hip.cpp and
tests/native/global_full_affine_host_fake.cpp, which holds the stand-in for the launcher that fake_hip.cpp does not know and
the checks: every refusal (a mask of 16, lengths of 0 and 16385, an open of -1 or 128, an extend of 128, NULL buffers, one of
moves / steps) before anything is launched, the host entry (traceback and ends-only at n = 1, 256, 257 and 640: every result,
the slice sizes, the move words each slice copies back, the launches, their streams and open, extend and the mask in every
slice), the device entry on two streams with a workspace that grows, the timer and the release of the workspaces."""
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
    tmp = tmp_path_factory.mktemp("global_full_affine_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "global_full_affine_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [os.path.join(PKG, "csrc", "global_full_affine_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "global_full_affine_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


def test_global_full_affine_host_paths(fake_exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([fake_exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "global_full_affine host fake ok" in r.stdout
    assert "refused, nothing launched" in r.stdout
    # 16 host cases, 5 device cases, the timer, then 1 device case, 1 host case and the release line
    assert r.stdout.count(": ok") == 25
