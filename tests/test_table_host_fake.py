"""The host sides of the two table aligners (local: swmi_local_*, exact semi-global: swmi_semiglobal_full*) on a fake GPU, no
device needed: the real host sources (every csrc/swmi_*.cpp), compiled with g++ and ASan + UBSan against
tests/native/fake_hip.cpp, whose launcher stand-ins write results derived from each alignment's index and abort on any copy
or launch that leaves its device block.  tests/native/table_host_fake.cpp checks, for each aligner, the host entry
(traceback and ends-only at n = 1, one slice, one slice + 1 and two and a half slices: every result, the move words each
slice copies back, the launches and their streams), the device entry on two streams with a workspace that grows, the timer,
and for the semi-global aligner the release of its workspaces."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def table_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("table_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "table_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp")))
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "table_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


@pytest.mark.parametrize("aligner", ["local", "sgfull"])
def test_table_aligner_host_paths(table_exe, aligner):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([table_exe, aligner], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "table host fake ok" in r.stdout
    assert r.stdout.count(": ok") == (17 if aligner == "sgfull" else 14)
