"""The host side of the wide-alphabet aligners (csrc/wide_api.cpp, all of libswmi_wide.so's host code) on a fake GPU, no device
needed: the real source compiled with g++ and ASan + UBSan as a stand-alone program against tests/native/fake_hip.cpp and
tests/native/wide_host_fake.cpp, which holds the stand-ins for the kernels' launcher and the checks: a traceback batch split by
the byte budget into at least 3 slices and an ends-only one split by the count cap; every slice's launches widest first, then
longest seq1 first, each alignment launched once; every result at its caller position with sentinels behind ends and moves
that survive; every buffer access inside its block (ASan on the fake's malloc'ed device memory); the device entry on two
streams with a growing workspace, the timer and the release."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_wide_host_paths(tmp_path):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "wide_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "wide_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(PKG, "csrc", "wide_api.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "wide host fake ok\n" in r.stdout
    # the refusals, 5 host cases, 4 device cases, then 1 host case after the release
    assert r.stdout.count(": ok") == 11, r.stdout
