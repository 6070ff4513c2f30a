#!/usr/bin/env python3
"""Generate tests/golden/f8_sgfull.npz from the REAL reference's SemiGlobal_111 (source.cpp:1776-1834), with the score
of its SemiGlobal_AdaptiveBanded_XDrop_111_32_70 (:1836-1976) on the same inputs beside it.

Run by hand where the reference sources lie (SWREF_SOURCE, default /root/reference/source.cpp):

    python tests/golden/make_golden_sgfull.py

It compiles ref_sgfull_shim.cpp into a temporary directory outside the tree and calls the reference's own functions
(SemiGlobal_111 takes about 2 s and 1 GiB per call).  No build step, test, smoke() or bench.py uses this script or the
shim.  The fixture is DATA: the inputs, and what the reference returned.

Fields (n vectors, all 16384 x 16384, match 1 / mismatch -1 / gap 1):
  seq1[n, 16384], seq2[n, 16384]   uint8 bases 0..3; vectors 0..15 are the 16 input pairs of F6
  kinds[n] (index into kind_names)
  scores[n], lengths[n], ends[n, 2]  SemiGlobal_111: score, path length (steps + 1), best cell
  moves (uint8, F6's encoding: 1 = (+1, +1), 2 = (+1, 0), 3 = (0, +1), from (0,0) to the best cell), move_offsets[n + 1]
  xdrop_scores[n], xdrop_ends[n, 2]   SemiGlobal_AdaptiveBanded_XDrop_111_32_70 on the same pair
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.environ.get("SWREF_SOURCE", "/root/reference/source.cpp")
N = 16384
KINDS = ("f6", "identical", "mismatch", "homopolymer", "shifted", "deletion20", "deletion60", "deletion100", "deletion400",
         "insertion100", "random")


def build_shim(tmp):
    so = os.path.join(tmp, "libswref_sgfull.so")
    subprocess.check_call(["g++", "-std=c++1y", "-O2", "-mavx2", "-w", "-shared", "-fPIC", '-DSWREF_SOURCE="%s"' % SOURCE,
                           "-o", so, os.path.join(HERE, "ref_sgfull_shim.cpp")])
    return ctypes.CDLL(so)


def pairs(rng):
    f6 = np.load(os.path.join(HERE, "f6_semiglobal.npz"))
    for k in range(len(f6["scores"])):
        yield "f6", f6["seq1"][k], f6["seq2"][k]
    a = rng.integers(0, 4, N, dtype=np.uint8)
    yield "identical", a, a.copy()
    yield "mismatch", np.zeros(N, np.uint8), np.ones(N, np.uint8)            # every cell a mismatch: best cell (0,0)
    yield "homopolymer", np.full(N, 2, np.uint8), np.full(N, 2, np.uint8)   # ties everywhere
    b = np.concatenate([rng.integers(0, 4, 37, dtype=np.uint8), a[:-37]])
    yield "shifted", a, b
    for d in (20, 60, 100, 400):                                          # a run of d bases deleted at position 8000
        yield "deletion%d" % d, a, np.concatenate([a[:8000], a[8000 + d:], rng.integers(0, 4, d, dtype=np.uint8)])
    yield "insertion100", a, np.concatenate([a[:8000], rng.integers(0, 4, 100, dtype=np.uint8), a[8000:N - 100]])
    for _ in range(2):
        yield "random", rng.integers(0, 4, N, dtype=np.uint8), rng.integers(0, 4, N, dtype=np.uint8)


def main():
    rng = np.random.default_rng(8)
    cap = 2 * N + 1
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_shim(tmp)
        rows = []
        for kind, a, b in pairs(rng):
            a = np.ascontiguousarray(a, np.uint8)
            b = np.ascontiguousarray(b, np.uint8)
            out = {}
            for name, fn in (("full", ref.swref_sgfull_111), ("xdrop", ref.swref_sgxdrop_111)):
                buf = np.zeros((cap, 2), np.int32)
                length = ctypes.c_size_t()
                sc = fn(a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p),
                        ctypes.c_size_t(cap), ctypes.byref(length))
                assert length.value <= cap
                out[name] = (sc, buf[: length.value].copy())
            path = out["full"][1]
            d = np.diff(path, axis=0)
            moves = np.where((d[:, 0] == 1) & (d[:, 1] == 1), 1, np.where(d[:, 0] == 1, 2, 3)).astype(np.uint8)
            rows.append((KINDS.index(kind), a, b, out["full"][0], len(path), path[-1], moves, out["xdrop"][0], out["xdrop"][1][-1]))
            print("%-13s exact %6d at (%5d, %5d)  x-drop %6d" % (kind, out["full"][0], path[-1][0], path[-1][1], out["xdrop"][0]))
    out = os.path.join(HERE, "f8_sgfull.npz")
    np.savez_compressed(out, seq1=np.stack([r[1] for r in rows]), seq2=np.stack([r[2] for r in rows]),
                        kinds=np.array([r[0] for r in rows], np.int32), kind_names=np.array(KINDS),
                        scores=np.array([r[3] for r in rows], np.int32), lengths=np.array([r[4] for r in rows], np.int32),
                        ends=np.stack([r[5] for r in rows]).astype(np.int32), moves=np.concatenate([r[6] for r in rows]),
                        move_offsets=np.cumsum([0] + [len(r[6]) for r in rows]).astype(np.int64),
                        xdrop_scores=np.array([r[7] for r in rows], np.int32),
                        xdrop_ends=np.stack([r[8] for r in rows]).astype(np.int32))
    print("wrote %s: %d alignments" % (out, len(rows)))


if __name__ == "__main__":
    sys.exit(main())
