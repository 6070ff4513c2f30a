"""The host side of the banded global / fit / overlap / extension aligner (csrc/banded_api.cpp compiled with
-DSWMI_BANDED_GLOBAL_LIBRARY, all of the host code of libswmi_banded_global.so) on a fake GPU, no device needed: the real source
compiled with g++ and ASan + UBSan as a stand-alone program against the unchanged tests/native/fake_hip.cpp and
tests/native/banded_global_host_fake.cpp; nothing is loaded into Python.  The driver runs the checks of the local library's
driver (slices on two buffer sets in turn, the copies of every slice, every result at its caller position with sentinels that
survive, every operand of every launch inside one live device block for the bytes the global kernel touches, workspaces per
stream that grow, the timer, the release) and two more: free_ends reaches every launch as given, and a refused mask reaches no
launch and touches no device."""
import os
import shutil
import subprocess

from conftest import PKG, ROOT


def test_banded_global_host_paths(tmp_path):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "banded_global_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-DSWMI_BANDED_GLOBAL_LIBRARY", "-I/opt/rocm/include",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "banded_global_host_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(PKG, "csrc", "banded_api.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "banded global host fake ok\n" in r.stdout
    # the refusals, five host cases, the device entry
    assert r.stdout.count(": ok") == 7, r.stdout
