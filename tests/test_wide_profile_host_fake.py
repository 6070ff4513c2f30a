"""The host side of the profile aligners (csrc/wide_api.cpp compiled with -DSWMI_WIDE_PROFILE_LIBRARY, all of the host code of
libswmi_wide_profile.so) on a fake GPU, no device needed: the real source compiled with g++ and ASan + UBSan as a stand-alone
program against tests/native/fake_hip.cpp and tests/native/wide_profile_host_fake.cpp; nothing is loaded into Python.  The
driver holds the stand-in for the launcher and the checks: the profile in "device" memory is the call's in the kernels'
transposed layout with -128 at exactly the columns past len2, at len2 = 1, 17, 1025 and 4096; the gaps, the mask and the wave
count; a traceback batch split by the byte budget into at least 3 slices and an ends-only one split by the count cap; the
zero-length slots in a launch of their own; every result at its caller position with sentinels behind ends and moves that
survive; every buffer access inside its block (ASan on the fake's malloc'ed device memory); the device entry on two streams
with different profiles and a growing workspace, the timer and the release.  test_wide_host_fake.py runs the same source's two
other builds."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_wide_profile_host_paths(tmp_path):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "wide_profile_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-DSWMI_WIDE_PROFILE_LIBRARY"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "wide_profile_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(PKG, "csrc", "wide_api.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "wide profile host fake ok\n" in r.stdout
    # the refusals, 8 + 3 host cases at the four lengths, no columns, the count cap, 5 device cases, 1 host case after the release
    assert r.stdout.count(": ok") == 20, r.stdout
