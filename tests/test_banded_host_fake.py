"""The host side of the banded aligners (csrc/banded_api.cpp, all of the host code of libswmi_banded.so and, compiled with
-DSWMI_BANDED_GLOBAL_LIBRARY, of libswmi_banded_global.so) on a fake GPU, no device needed: the real source compiled with g++ and
ASan + UBSan as a stand-alone program against the unchanged tests/native/fake_hip.cpp and tests/native/banded_host_fake.cpp, once
per library with the library's define on every file; nothing is loaded into Python.  The driver holds the stand-in for the
launcher and the checks: an ends-only host call cut by the count cap into three slices on two buffer sets in turn, the copies of
every slice, traceback calls with and without diagonals, every result at its caller position with sentinels behind the arrays
that survive, every operand of every launch inside one live device block for the bytes the library's kernel touches, the gaps
and the matrix as given, buffer sets that are kept; the device entry on two streams with a workspace per stream that grows, the
timer and the release.  For the global library also: free_ends reaches every launch as given, and a refused mask reaches no
launch and touches no device."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


# the refusals, five host cases, the device entry
@pytest.mark.parametrize("defines,last_line,oks", [([], "banded host fake ok\n", 7),
                                                   (["-DSWMI_BANDED_GLOBAL_LIBRARY"], "banded global host fake ok\n", 7)],
                         ids=["banded", "banded_global"])
def test_banded_host_paths(tmp_path, defines, last_line, oks):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "banded_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + defines + ["-o", exe, os.path.join(native, "banded_host_fake.cpp"),
                                                    os.path.join(native, "fake_hip.cpp"), os.path.join(PKG, "csrc", "banded_api.cpp"),
                                                    "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert last_line in r.stdout
    assert r.stdout.count(": ok") == oks, r.stdout
