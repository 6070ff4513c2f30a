"""The profile aligners (libswmi_wide_profile.so, swmi.wide_profile) on the GPU.  Every comparison is exact integer equality.
Both kinds, with a traceback and ends-only, against the C restatement tests/native/wide_profile_oracle.c: one call per len2 at
the lane (16 columns) and wave (1024) edges and at the last column the profile holds (4096) -- where the row stride 64 W and
the padding inside the last lane and the last wave can go wrong -- on sequences at the chunk (32 rows) and staging (128 rows)
edges, zero and 16384 among them, in caller order and permuted, under a scoring profile, a random int8 one and the extremes;
the global kind under four masks everywhere and all 16 at the small len2; len2 = 0 with no profile; from_sequence profiles
against the merged wide kernels on the replicated query, field by field and move by move; two profiles back to back on one
stream; a host call of two slices; search with the boundary of `top` inside a tie; the C++ overloads.
test_wide_profile_cpu.py shows that the batch is not trivial."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from wide_profile_support import (GAPS, LONG_LEN2, PROFILES, ProfileOracle, noisy, all_len2s, profile_for, scoring_profile, sequences_for)
from wide_support import ALL_MASKS, GLOBAL, LOCAL, assert_same, concat, offsets, scoring_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poracle(tmp_path_factory):
    return ProfileOracle(tmp_path_factory.mktemp("wide_profile_gpu_oracle"))


@pytest.fixture(scope="module")
def wp(swmi_mod):
    """The library needs no swmi.init(): it runs on the current device."""
    swmi_mod.wide_profile.load()
    return swmi_mod.wide_profile


def _run(wp, kind, seqs, profile, gaps, mask, traceback):
    if kind == LOCAL:
        return wp.local(seqs, profile, gaps[0], gaps[1], traceback=traceback)
    return wp.global_(seqs, profile, gaps[0], gaps[1], mask, traceback=traceback)


@pytest.mark.parametrize("len2", all_len2s())
def test_every_field_equals_the_restatement(wp, poracle, len2):
    seqs = sequences_for(len2)
    assert (16384 in [len(x) for x in seqs]) == (len2 == LONG_LEN2)
    perm = np.random.default_rng(8 + len2).permutation(len(seqs))
    permuted = [seqs[k] for k in perm]
    for name in PROFILES:
        profile, gaps = profile_for(name, len2), GAPS[name]
        for kind in (LOCAL, GLOBAL):
            for mask in ([0] if kind == LOCAL else ALL_MASKS if len2 <= 17 else [0, 5, 10, 15]):
                want = poracle.align(kind, seqs, profile, gaps[0], gaps[1], mask)
                assert_same(_run(wp, kind, seqs, profile, gaps, mask, True), want, (len2, name, kind, mask, "traceback"))
                ends_only = poracle.align(kind, seqs, profile, gaps[0], gaps[1], mask, traceback=False)
                assert_same(_run(wp, kind, seqs, profile, gaps, mask, False), ends_only, (len2, name, kind, mask, "ends-only"), traceback=False)
            # permuted: every result follows its sequence
            mask = 0 if kind == LOCAL else 10
            assert_same(_run(wp, kind, permuted, profile, gaps, mask, True), poracle.align(kind, permuted, profile, gaps[0], gaps[1], mask),
                        (len2, name, kind, "permuted"))


def test_no_columns_and_no_profile(wp, poracle):
    seqs = sequences_for(17)
    for kind, masks in ((LOCAL, [0]), (GLOBAL, ALL_MASKS)):
        for mask in masks:
            for tb in (True, False):
                got = _run(wp, kind, seqs, np.zeros((0, 32), np.int8), (4, 1), mask, tb)
                assert_same(got, poracle.align(kind, seqs, np.zeros(0, np.int8), 4, 1, mask, traceback=tb), ("len2 0", kind, mask, tb), traceback=tb)
    lens = np.array([len(x) for x in seqs])
    assert np.array_equal(wp.global_(seqs, np.zeros(0, np.int8), 4, 1, 0)[0], np.where(lens > 0, -(4 + (lens - 1)), 0))


def _related(rng, query, len1s):
    """Sequences that hold a noisy copy of a stretch of the query (all three kinds of move), junk in bits 5 - 7."""
    out = []
    for len1 in len1s:
        x = rng.integers(0, 32, len1, dtype=np.uint8)
        if len1 >= 40 and len(query) >= 40:
            w = min(len1 - 8, len(query), 300)
            lo = int(rng.integers(0, len(query) - w + 1))
            piece = noisy(rng, query[lo:lo + w] & 31)
            x[4:4 + len(piece)] = piece[:len1 - 4]
        out.append((x | (rng.integers(0, 8, len1, dtype=np.uint8) << 5)).astype(np.uint8))
    return out


@pytest.mark.parametrize("len2", [700, 1500, 2500, 4000])
def test_from_sequence_profiles_equal_the_merged_wide_kernels(wp, swmi_mod, len2):
    """The identity that ties the new kernels to merged ones, at 1, 2, 3 and 4 wavefronts, under an asymmetric matrix."""
    wide = swmi_mod.wide
    rng = np.random.default_rng(70 + len2)
    sm = scoring_matrix(21)
    assert not np.array_equal(sm.reshape(32, 32), sm.reshape(32, 32).T)
    query = rng.integers(0, 256, len2, dtype=np.uint8)
    seqs = _related(rng, query, [0, 1, 40, 64, 129, 333, 700, 90, 257, 1200])
    # the last one also ends in a copy of the query's end, the last columns the profile holds
    seqs[-1][-60:] = query[-60:]
    profile = wp.from_sequence(query, sm)
    replicated = [query] * len(seqs)
    for tb in (True, False):
        want = wide.local(seqs, replicated, sm, 7, 2, traceback=tb)
        assert_same(wp.local(seqs, profile, 7, 2, traceback=tb), want, ("identity local", len2, tb), traceback=tb)
        assert want[0].max() > 200
        for mask in (0, 6, 9, 15):
            want = wide.global_(seqs, replicated, sm, 7, 2, mask, traceback=tb)
            assert_same(wp.global_(seqs, profile, 7, 2, mask, traceback=tb), want, ("identity global", len2, mask, tb), traceback=tb)


def test_two_profiles_back_to_back_on_one_stream(wp, poracle):
    """Four device calls, two per stream, each with a profile of its own, none waited for before all are issued: the stream's
    one workspace and pinned block serve both of its calls, and each result must match its own profile."""
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(41)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    jobs = []
    # (stream, kind, traceback, mask, len2): one stream's two calls share len2 = 1025 and differ in the scores alone; the other's
    # differ in the wave count too
    for x, (which, kind, tb, mask, len2) in enumerate(((0, LOCAL, True, 0, 1025), (0, LOCAL, True, 0, 1025), (1, GLOBAL, True, 15, 300),
                                                       (1, GLOBAL, False, 10, 2100))):
        profile = scoring_profile(len2, seed=30 + x)
        cons = np.argmax(profile, axis=1).astype(np.uint8)
        seqs = _related(rng, cons, [int(v) for v in rng.integers(0, 400, 60)] + [0, 1, 129])
        if x == 1:
            seqs = jobs[0][5]                       # the very same sequences under another profile
        off = offsets(seqs)
        mo = wp.move_offsets(off, len2)
        m = len(seqs)
        t = dict(a=torch.from_numpy(concat(seqs)).to(dev), sc=torch.zeros(m, dtype=torch.int32, device=dev),
                 ends=torch.zeros((m, 4), dtype=torch.int32, device=dev), mv=torch.zeros(int(mo[-1]) + 2, dtype=torch.int64, device=dev),
                 st=torch.zeros(m, dtype=torch.int32, device=dev))
        jobs.append((streams[which], kind, tb, mask, profile, seqs, off, mo, t))
    torch.cuda.synchronize()
    for s, kind, tb, mask, profile, seqs, off, mo, t in jobs:
        bufs = (t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr() if tb else None, t["st"].data_ptr() if tb else None)
        if kind == LOCAL:
            wp.local_device(t["a"].data_ptr(), off, profile, 7, 1, *bufs, stream=s.cuda_stream)
        else:
            wp.global_device(t["a"].data_ptr(), off, profile, 7, 1, mask, *bufs, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    results = []
    for s, kind, tb, mask, profile, seqs, off, mo, t in jobs:
        want = poracle.align(kind, seqs, profile, 7, 1, mask, traceback=tb)
        got = (t["sc"].cpu().numpy(), t["ends"].cpu().numpy(), t["mv"].cpu().numpy().view(np.uint64) if tb else None, mo if tb else None,
               t["st"].cpu().numpy().view(np.uint32) if tb else None)
        assert_same(got, want, ("device", kind, tb), traceback=tb)
        assert np.any(want[0] != 0)
        results.append(want[0])
    assert not np.array_equal(results[0], results[1])          # the two profiles tell the same sequences apart
    # the timer runs the same launches
    s, kind, tb, mask, profile, seqs, off, mo, t = jobs[2]
    ms = wp.time_device(wp.GLOBAL, t["a"].data_ptr(), off, profile, 7, 1, mask, t["sc"].data_ptr(), t["ends"].data_ptr(), t["mv"].data_ptr(),
                        t["st"].data_ptr(), stream=s.cuda_stream, iters=2)
    assert ms > 0
    wp.release_workspaces()


def test_host_call_of_two_slices_by_the_count_cap(wp, poracle):
    """2^20 + 5 sequences of one letter, ends-only: two slices, the profile uploaded to both buffer sets, results at the
    caller's positions."""
    rng = np.random.default_rng(21)
    n = (1 << 20) + 5
    off = np.arange(n + 1, dtype=np.uint64)
    cat = rng.integers(0, 256, n + 16, dtype=np.uint8)
    assert wp.slices_for(off, 3, traceback=False) == [1 << 20, 5]
    profile = rng.integers(-20, 21, (3, 32)).astype(np.int8)
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0), (GLOBAL, 15)):
        want = poracle.align(kind, (cat, off), profile, 3, 1, mask, traceback=False)
        sc, ends, moves, mo, steps = _run(wp, kind, (cat, off), profile, (3, 1), mask, False)
        assert moves is None and mo is None and steps is None
        assert np.array_equal(sc, want[0]) and np.array_equal(ends, want[1]), (kind, mask)
        assert want[0].max() > 0 and (kind == LOCAL or mask or want[0].min() < 0)
        assert len(np.unique(want[0][-5:])) > 1 or len(np.unique(want[0][:64])) > 1


def test_search_with_the_top_boundary_inside_a_tie(wp, swmi_mod, poracle):
    rng = np.random.default_rng(91)
    len2 = 1100
    profile = scoring_profile(len2, seed=77)
    cons = np.argmax(profile, axis=1).astype(np.uint8)
    base = _related(rng, cons, [int(v) for v in rng.integers(40, 300, 24)])
    seqs = base + [base[3].copy(), base[3].copy(), base[7].copy()] + _related(rng, cons, [0, 1, 50])
    seqs = [seqs[k] for k in np.random.default_rng(92).permutation(len(seqs))]
    for kind, mask in ((LOCAL, 0), (GLOBAL, 10)):
        scores = poracle.align(kind, seqs, profile, 6, 1, mask, traceback=False)[0]
        order = sorted(range(len(seqs)), key=lambda k: (-int(scores[k]), k))
        # a `top` whose boundary falls between two equal scores
        tops = [t for t in range(1, len(seqs)) if scores[order[t - 1]] == scores[order[t]]]
        assert tops, "no tie in the database"
        full = _run(wp, kind, seqs, profile, (6, 1), mask, True)
        for top in (tops[0], tops[-1], 1, len(seqs) + 3):
            idx, sc, ends, paths = wp.search(seqs, profile, 6, 1, top, kind=kind, free_ends=mask)
            want = order[:top]
            assert list(idx) == want, (kind, top)
            assert np.array_equal(sc, full[0][want]) and np.array_equal(ends, full[1][want])
            assert len(paths) == len(want)
            for r, k in enumerate(want):
                row = full[2][int(full[3][k]):int(full[3][k + 1])]
                assert np.array_equal(paths[r], swmi_mod.local_full_expand_moves(row, full[4][k], full[1][k, 0], full[1][k, 1])), (kind, top, k)
        assert wp.search(seqs, profile, 6, 1, 0, kind=kind, free_ends=mask)[0].size == 0


def test_cpp_overloads_on_a_mixed_batch(wp, poracle, swmi_mod, tmp_path):
    """tests/native/compat_wide_profile.cpp, built by g++ against libswmi_wide_profile.so and libswmi.so: 40 sequences in pieces
    of 16 against a profile of 2049 columns; it prints score, path length, start cell, end cell and a path checksum, which the
    restatement confirms."""
    assert shutil.which("g++") is not None
    rng = np.random.default_rng(61)
    len2 = 2049
    profile = scoring_profile(len2, seed=62)
    cons = np.argmax(profile, axis=1).astype(np.uint8)
    seqs = _related(rng, cons, [int(x) for x in rng.integers(0, 900, 37)] + [0, 1, 700])
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.int32(len2).tobytes() + np.ascontiguousarray(profile, np.int8).tobytes() + np.int32(len(seqs)).tobytes())
        for x in seqs:
            fh.write(np.int32(len(x)).tobytes() + x.tobytes())
    exe = str(tmp_path / "compat_wide_profile")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_wide_profile.cpp"), "-o", exe, "-L", lib, "-lswmi_wide_profile", "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, str(data)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "mismatches 0", lines[-1]

    def checksum(path):
        want = 0
        for i, j in path:
            want = (want * 1000003 + int(i) * 32771 + int(j)) % (1 << 64)
        return want

    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == 3 * len(seqs)
    at = 0
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0), (GLOBAL, 10)):
        sc, ends, moves, mo, steps = poracle.align(kind, seqs, profile, 7, 2, mask)
        for k in range(len(seqs)):
            row = moves[int(mo[k]):int(mo[k + 1])]
            path = swmi_mod.local_full_expand_moves(row, steps[k], ends[k, 0], ends[k, 1]) if steps[k] else ends[k, 2:].reshape(1, 2)
            assert rows[at + k] == (int(sc[k]), int(steps[k]) + 1, int(ends[k, 2]), int(ends[k, 3]), int(ends[k, 0]), int(ends[k, 1]),
                                    checksum(path)), (at, k)
        at += len(seqs)
