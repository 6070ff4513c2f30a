"""The host sides of the fourteen fixed-shape table aligners (csrc/table_api.cpp through the slice pipeline of csrc/swmi_table.cpp)
on a fake GPU, no device needed: the real host sources (every csrc/swmi_*.cpp and table_api.cpp), compiled once with g++ and
ASan + UBSan against tests/native/fake_hip.cpp, whose launcher stand-ins write results derived from each alignment's index,
log what they were handed and abort on any copy or launch that leaves its device block.  tests/native/table_host_fake.cpp runs
one family per invocation: the refusals with their codes and texts (without a device and with one), the order of the timer's
checks, the slice sizes, the host entry (traceback and ends-only at n = 1, one slice, one slice + 1 and two and a half slices:
every result, the move words each slice copies back, the launches, their streams and parameters), the device entry on two
streams with a workspace that grows, the timer, the release of the workspaces where there is one, the entries after
swmi_shutdown, and for the six striped families the top of their range (the domain rule's edge, or for the long local pair,
which has no rule, the int8 extremes at 65536 x 65536), the launcher a shape reaches and the carry."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

# ": ok" lines per family: refusals, timer order, slices_for, 8 host and 5 device cases, timer, shutdown = 18; the release
# adds 3 (a device case, a host case, its own line); a mask runs every host case twice (+ 8); a striped family adds the top
# of its range (the domain rule, or that it has none), 8 routing host cases and 6 device cases (+ 15)
OK_LINES = {"local": 18, "sgfull": 21, "local_affine": 18, "sgfull_affine": 21, "local_full": 21, "local_full_affine": 21,
            "global_full": 29, "global_full_affine": 29, "global_long": 44, "global_long_affine": 44, "local_long": 36,
            "local_long_affine": 36, "semiglobal_long": 36, "semiglobal_long_affine": 36}


@pytest.fixture(scope="module")
def table_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("table_host_fake")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "table_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    host_sources = sorted(glob.glob(os.path.join(PKG, "csrc", "swmi_*.cpp"))) + [os.path.join(PKG, "csrc", "table_api.cpp")]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "table_host_fake.cpp"), os.path.join(native, "fake_hip.cpp")]
                       + host_sources + ["-ldl", "-lpthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


@pytest.mark.parametrize("family", sorted(OK_LINES))
def test_table_aligner_host_paths(table_exe, family):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([table_exe, family], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "table host fake ok: %s\n" % family in r.stdout
    assert r.stdout.count(": ok") == OK_LINES[family]


def test_cpp_overloads_compile_and_link(tmp_path):
    """The C++ overloads of the any-length affine local aligner (include/swmi_compat.hpp) compile and link against the library."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "compat_local_full_affine.cpp")
    syntax = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert syntax.returncode == 0, syntax.stdout
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o",
                            str(tmp_path / "compat_local_full_affine"), "-L", lib, "-lswmi", "-lpthread", "-Wl,-rpath," + lib],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
