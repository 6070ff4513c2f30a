"""The host side of the wide-alphabet aligners (csrc/wide_api.cpp, all of the host code of libswmi_wide.so and, compiled with
-DSWMI_WIDE_LONG_LIBRARY, of libswmi_wide_long.so) on a fake GPU, no device needed: the real source compiled with g++ and
ASan + UBSan as a stand-alone program against tests/native/fake_hip.cpp and tests/native/wide_host_fake.cpp, once per library
with the library's define on every file.  The driver holds the stand-ins for the launchers and the checks: a traceback batch
split by the byte budget into at least 3 slices and an ends-only one split by the count cap; every slice's launches widest
first, then longest seq1 first, each alignment launched once; every result at its caller position with sentinels behind ends
and moves that survive; every buffer access inside its block (ASan on the fake's malloc'ed device memory); the device entry on
two streams with a growing workspace, the timer and the release.  For the long library also: in every slice the striped
launch first and each alignment launched by the kernel its shape asks for; every striped slot's carry block inside the
workspace and disjoint from the others of its launch; the stripe width the rule or the setter names; the global kind's
domain rule."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


# the refusals, 5 host cases, 4 device cases, then 1 host case after the release; the long library: 2 more with a forced width
@pytest.mark.parametrize("defines,last_line,oks", [([], "wide host fake ok\n", 11),
                                                   (["-DSWMI_WIDE_LONG_LIBRARY"], "wide long host fake ok\n", 13)],
                         ids=["wide", "wide_long"])
def test_wide_host_paths(tmp_path, defines, last_line, oks):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "wide_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + defines + ["-o", exe, os.path.join(native, "wide_host_fake.cpp"),
                                                    os.path.join(native, "fake_hip.cpp"), os.path.join(PKG, "csrc", "wide_api.cpp"),
                                                    "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert last_line in r.stdout
    assert r.stdout.count(": ok") == oks, r.stdout
