"""The host side of the mixed-shape banded aligners (csrc/banded_ragged_api.cpp, all of the host code of libswmi_banded_ragged.so
and, compiled with -DSWMI_BANDED_WIDTH_LIBRARY, of libswmi_banded_width.so) on a fake GPU, no device needed: the real source
compiled with g++ and ASan + UBSan as a stand-alone program against the unchanged tests/native/fake_hip.cpp and
tests/native/banded_ragged_host_fake.cpp, once per library with the library's define on every file; nothing is loaded into
Python.  The driver holds the stand-in for the launcher and the checks.  Per launch: the band as given (128 in the ragged
build); every slot's sequence ranges, code range at the width's size, move range and result index inside live blocks of the
sizes the kernels touch, code ranges that do not overlap and are aligned to a lane's whole stores, the slots in the planner's
order (the width's swept rows descending, ties in caller order), each slot's diagonal the caller's, clamped, and the kind, the
mask, the gaps and the matrix as given.  Its cases: the refusals in the header's order, in the width build the band first, with
nothing logged; the planner's key against values worked out by hand at every width; traceback calls of both kinds and a pair
that changes place only at band 1024, at every width of the build; three and two ends-only slices cut by the count cap and two
cut by the byte budget, each with a ragged last slice, on two buffer sets in turn; a call without diagonals; empty sequences on
either side, on both, and a side that is empty throughout; every result at its caller position with sentinels behind every
output array; buffer sets that are kept; the device entries on two streams with a workspace per stream that is reused with no
second allocation; the timer's 1 + iters launches; the release; and no leak."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


# the refusals, the key by hand, then per width of the build 2 traceback cases, a planner-key pair (not at 256) and the device
# entries, and 10 cases at one width each: 2 + 4 * 1 + 10 and 2 + 4 * 4 - 1 + 10
@pytest.mark.parametrize("defines,last_line,oks", [([], "banded ragged host fake ok\n", 16),
                                                   (["-DSWMI_BANDED_WIDTH_LIBRARY"], "banded width host fake ok\n", 27)],
                         ids=["banded_ragged", "banded_width"])
def test_banded_ragged_host_paths(tmp_path, defines, last_line, oks):
    assert shutil.which("g++") is not None
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "banded_ragged_host_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + defines + ["-o", exe, os.path.join(native, "banded_ragged_host_fake.cpp"),
                                                    os.path.join(native, "fake_hip.cpp"), os.path.join(PKG, "csrc", "banded_ragged_api.cpp"),
                                                    "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert last_line in r.stdout
    assert r.stdout.count(": ok") == oks, r.stdout
