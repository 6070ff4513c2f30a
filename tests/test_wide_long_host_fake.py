"""The host side of the long wide-alphabet aligners (csrc/wide_long_api.cpp, all of libswmi_wide_long.so's host code) on a fake
GPU, no device needed: the real source compiled with g++ and ASan + UBSan as a stand-alone program against
tests/native/fake_hip.cpp and tests/native/wide_long_host_fake.cpp, which holds the stand-ins for the two launchers and the
checks: a traceback batch split by the byte budget into at least 3 slices and an ends-only one split by the count cap; in every
slice the striped launch first, then the unstriped ones widest first, each alignment launched once and by the kernel its shape
asks for; every striped slot's carry block inside the workspace (ASan on the fake's malloc'ed device memory) and disjoint from
the others of its launch; the stripe width the rule or the setter names; every result at its caller position with sentinels
behind ends and moves that survive; the device entry on two streams with a growing workspace, the timer and the release."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_wide_long_host_paths(tmp_path):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "wide_long_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "wide_long_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(PKG, "csrc", "wide_long_api.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "wide long host fake ok\n" in r.stdout
    # the refusals, 5 host cases, 2 with a forced width, 4 device cases, then 1 host case after the release
    assert r.stdout.count(": ok") == 13, r.stdout
