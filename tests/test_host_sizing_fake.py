"""The host-batch pipeline's buffer sizing (swmi_api.cpp score_host_batch) on fake GPUs, no device needed: the real host code,
compiled with g++ and ASan + UBSan against tests/native/fake_hip.cpp, whose fake device aborts on any copy or launch that
leaves its allocation.  tests/native/host_sizing_fake.cpp finds the batch sizes whose LAST score group has a larger granule
than the first (the 2-bit packed entry's balanced schedule) and scores them on fresh contexts: the production-like group of
1M pairs (SWMI_TEST_SCORE_GROUP; 1 703 935 pairs is one such size), small groups with a small steady granule
(SWMI_HOST_MIN_GRANULE) under one and two issuing threads and the serial order, and swmi_score_batch_packed_multi on three
fake GPUs."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def sizing_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("host_sizing_fake")
    csrc = os.path.join(PKG, "csrc")
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp / "host_sizing_fake")
    flags = ["-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    b = subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(native, "host_sizing_fake.cpp"), os.path.join(native, "fake_hip.cpp"),
                                          os.path.join(csrc, "swmi_api.cpp"), os.path.join(csrc, "swmi_multi.cpp"), "-ldl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and "asan" in b.stdout.lower() and "cannot find" in b.stdout.lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stdout[-3000:]
    return exe


def _run(exe, mode, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("SWMI_")}
    r = subprocess.run([exe, mode], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(clean, ASAN_OPTIONS="detect_leaks=1", FAKE_HIP_DEVICES="3", **env))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "host sizing fake ok" in r.stdout
    return r.stdout


def test_every_entry_at_a_one_million_pair_group_with_bad_tails(sizing_exe):
    out = _run(sizing_exe, "group", SWMI_TEST_SCORE_GROUP="1048576")
    assert "entry 1  n 1703935:" in out          # the worst tail at this group is 655 359 pairs (a granule of 135 167)


@pytest.mark.parametrize("threads", [{}, {"SWMI_HOST_THREADS": "1"}, {"SWMI_HOST_SERIAL": "1"}], ids=["two_threads", "one_thread", "serial"])
@pytest.mark.parametrize("group,steady", [(65536, 8192), (32768, 4096)])
def test_small_groups_with_a_small_steady_granule(sizing_exe, group, steady, threads):
    _run(sizing_exe, "small", SWMI_TEST_SCORE_GROUP=str(group), SWMI_HOST_MIN_GRANULE=str(steady), **threads)


def test_packed_multi_on_three_fake_gpus_with_a_bad_tail_per_shard(sizing_exe):
    _run(sizing_exe, "multi", SWMI_TEST_SCORE_GROUP="1048576")
