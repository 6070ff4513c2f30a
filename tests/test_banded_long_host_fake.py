"""What is new in the host side of libswmi_banded_long.so (csrc/banded_ragged_api.cpp compiled with -DSWMI_BANDED_LONG_LIBRARY,
DESIGN.md section 41) on a fake GPU, no device needed: the real source compiled with g++ and ASan + UBSan as a stand-alone
program against the unchanged tests/native/fake_hip.cpp and tests/native/banded_long_host_fake.cpp; nothing is loaded into
Python.  The driver holds the stand-in for the launcher and the checks: the length bound of 65536 and the tenth export's values;
the planner's key by hand for 65536-long pairs; and a traceback call of 131 alignments of 65536 x 65536 at band 1024 in two
slices by the byte budget, whose code offsets are a running sum, disjoint, aligned and past 2^32 bytes (arithmetic: the codes
are not touched), whose diagonal of 65536 + 511 reaches the launcher unclamped and whose INT32_MAX arrives as 131072, with every
result at its caller position.  What the three builds share is driven by tests/test_banded_ragged_host_fake.py."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_banded_long_host_paths(tmp_path):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "banded_long_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-DSWMI_BANDED_LONG_LIBRARY"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "banded_long_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(PKG, "csrc", "banded_ragged_api.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "banded long host fake ok\n" in r.stdout
    assert r.stdout.count(": ok") == 3, r.stdout
