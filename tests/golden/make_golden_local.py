#!/usr/bin/env python3
"""Generate tests/golden/f7_local.npz from the REAL reference's SmithWaterman_111_long (source.cpp:1526-1576).

Run by hand where the reference sources lie (SWREF_SOURCE, default /root/reference/source.cpp):

    python tests/golden/make_golden_local.py

It compiles ref_local_shim.cpp into a temporary directory outside the tree and calls the reference's own function.  No
build step, test, smoke() or bench.py uses this script or the shim.  The fixture is DATA: the inputs, and the score and the
full (i, j) path (start cell to end cell) that the reference returned.

Fields: lens[n] (len1 of each vector), kinds[n] (index into KINDS), seq1 (all seq1 concatenated), seq1_off[n + 1],
seq2[n, 128], scores[n], path (all paths concatenated, (total, 2) int32), path_off[n + 1].
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.environ.get("SWREF_SOURCE", "/root/reference/source.cpp")
LENGTHS = (1, 2, 63, 64, 127, 128, 129, 300, 1000, 4096, 16384)
KINDS = ("random", "similar85", "identical", "mismatch", "homopolymer", "tandem", "indel")


def build_shim(tmp):
    so = os.path.join(tmp, "libswref_local.so")
    subprocess.check_call(["g++", "-std=c++1y", "-O2", "-mavx2", "-w", "-shared", "-fPIC", '-DSWREF_SOURCE="%s"' % SOURCE,
                           "-o", so, os.path.join(HERE, "ref_local_shim.cpp")])
    return ctypes.CDLL(so)


def make_pair(rng, kind, len1):
    """(seq1 of len1 bases, seq2 of 128 bases) of one input kind."""
    seq2 = rng.integers(0, 4, 128, dtype=np.uint8)
    if kind == "random":
        seq1 = rng.integers(0, 4, len1, dtype=np.uint8)
    elif kind in ("similar85", "identical", "indel"):
        # seq2 (or a window of it) planted at a random offset of a random seq1
        seq1 = rng.integers(0, 4, len1, dtype=np.uint8)
        w = min(len1, 128)
        src = seq2[:w].copy()
        if kind == "similar85":
            flip = rng.random(w) < 0.15
            src[flip] = (src[flip] + rng.integers(1, 4, int(flip.sum()), dtype=np.uint8)) & 3
        if kind == "indel" and w > 8:
            cut = int(rng.integers(2, w - 2))
            src = np.concatenate([src[:cut], src[cut + 1:]]) if rng.random() < 0.5 else \
                np.concatenate([src[:cut], rng.integers(0, 4, 1, dtype=np.uint8), src[cut:]])
            src = src[:len1]
        at = int(rng.integers(0, len1 - len(src) + 1))
        seq1[at:at + len(src)] = src
    elif kind == "mismatch":
        # every base of seq1 differs from every base of seq2: score 0
        seq2 = np.full(128, int(rng.integers(0, 4)), np.uint8)
        seq1 = np.full(len1, (int(seq2[0]) + 1 + int(rng.integers(0, 3))) & 3, np.uint8)
    elif kind == "homopolymer":
        base = int(rng.integers(0, 4))
        seq1 = np.full(len1, base, np.uint8)
        seq2 = np.where(rng.random(128) < 0.9, base, rng.integers(0, 4, 128)).astype(np.uint8)
    elif kind == "tandem":
        unit = rng.integers(0, 4, int(rng.integers(2, 6)), dtype=np.uint8)
        seq1 = np.resize(unit, len1).astype(np.uint8)
        seq2 = np.resize(np.roll(unit, int(rng.integers(0, len(unit)))), 128).astype(np.uint8)
        seq2[rng.random(128) < 0.05] = rng.integers(0, 4, dtype=np.uint8)
    else:
        raise ValueError(kind)
    return seq1.astype(np.uint8), seq2.astype(np.uint8)


def main():
    rng = np.random.default_rng(7)
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_shim(tmp)
        lens, kinds, s1s, s2s, scores, paths = [], [], [], [], [], []
        for len1 in LENGTHS:
            reps = 1 if len1 >= 4096 else 2 if len1 >= 1000 else 4
            for kind_index, kind in enumerate(KINDS):
                for _ in range(reps):
                    a, b = make_pair(rng, kind, len1)
                    cap = len1 + 130
                    buf = np.zeros((cap, 2), np.int32)
                    length = ctypes.c_size_t()
                    sc = ref.swref_local_111(a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len1),
                                             b.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.c_size_t(cap), ctypes.byref(length))
                    assert length.value <= cap
                    lens.append(len1)
                    kinds.append(kind_index)
                    s1s.append(a)
                    s2s.append(b)
                    scores.append(sc)
                    paths.append(buf[: length.value].copy())
    off1 = np.concatenate([[0], np.cumsum([len(a) for a in s1s])]).astype(np.int64)
    offp = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    out = os.path.join(HERE, "f7_local.npz")
    np.savez_compressed(out, lens=np.array(lens, np.int32), kinds=np.array(kinds, np.int32), kind_names=np.array(KINDS),
                        seq1=np.concatenate(s1s), seq1_off=off1, seq2=np.stack(s2s), scores=np.array(scores, np.int32),
                        path=np.concatenate(paths).astype(np.int32), path_off=offp)
    print("wrote %s: %d alignments, scores %d..%d, %d zero" % (out, len(lens), min(scores), max(scores), scores.count(0)))


if __name__ == "__main__":
    sys.exit(main())
