"""The host side of the two long semi-global aligners (csrc/semiglobal_long_api.cpp over table_api.cpp's one body per kind of entry
and the slice pipeline of csrc/swmi_table.cpp) on a fake GPU, no device needed: the real host sources (every csrc/swmi_*.cpp,
table_api.cpp and semiglobal_long_api.cpp), compiled once with g++ and ASan + UBSan as a stand-alone program against the unchanged
tests/native/fake_hip.cpp and tests/native/fake_semiglobal_long.cpp, which holds the stand-ins of the two striped launchers and
their code sizes.  tests/native/semiglobal_long_host_fake.cpp runs one family per invocation: the refusals (the domain rule and
a traceback given by half among them), the domain's edge at 65536 x 65536 accepted, which launcher a shape reaches and the carry
it is handed per slice, the host entry at n = 1, S, S + 1 and 2.5 S, the device entry on two streams with a growing workspace, the
timer's launches, and the release."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

# ": ok" lines: refusals, the domain's edge, 8 routing cases, 8 host cases, 7 device cases, timer, release (1 + a device and a host case)
OK_LINES = 1 + 1 + 8 + 8 + 7 + 1 + 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++") is not None, "g++ not available"
    tmp = tmp_path_factory.mktemp("semiglobal_long_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    out = str(tmp / "semiglobal_long_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [os.path.join(PKG, "csrc", "table_api.cpp"),
                                                                                os.path.join(PKG, "csrc", "semiglobal_long_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", out, os.path.join(native, "semiglobal_long_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(native, "fake_semiglobal_long.cpp")] + host_sources + ["-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    return out


@pytest.mark.parametrize("family", ["linear", "affine"])
def test_semiglobal_long_host_paths(exe, family):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe, family], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "semiglobal long host fake ok: %s\n" % family in r.stdout
    assert r.stdout.count(": ok") == OK_LINES
