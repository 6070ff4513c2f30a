"""The banded aligners with a band width per call on the GPU (libswmi_banded_width.so, include/swmi_banded_width.h, DESIGN.md
section 38).  Expected values are the two existing C restatements called with lo = -band / 2, hi = band / 2 - 1
(banded_width_support.WidthOracle), unconditionally: score, the four ends, steps, and the moves word for word up to steps.  Every
test runs all four kernels of a kind -- with a traceback and ends-only, gap_open >= gap_extend and gap_open < gap_extend -- and
every test of the global kind runs the masks 0 .. 19 or spreads them over its cases.  The shapes are the smallest that hold the
traps of section 38: the lane's 2 K cells and their two seams, the band's edge diagonals, trips at every remainder, the walk
window's lane borders."""
import os
import subprocess

import numpy as np
import pytest
import torch

from banded_width_support import (ALL_MASKS, FORMS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_SLICE, NO_ALIGNMENT, WIDTHS, Batch, WidthOracle,
                                  assert_same, differs, drift_batch, moves_of, path_from, related_batch, related_pairs, unbounded_for)
from conftest import PKG, ROOT, match_matrix

pytestmark = pytest.mark.gpu

GUARD = 16                                  # guard words behind every output array
PATTERN = 0x5A5A5A5A5A5A5A5A
SM = match_matrix(2, -3)


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return WidthOracle(tmp_path_factory.mktemp("banded_width_oracle"))


@pytest.fixture(scope="module")
def bw(swmi_mod):
    swmi_mod.banded_width.load()
    return swmi_mod.banded_width


def _dev_bytes(cat):
    """a side's bytes on the device; a side that is empty throughout passes a buffer the library never reads"""
    host = np.ascontiguousarray(cat) if len(cat) else np.full(16, 255, np.uint8)
    return torch.from_numpy(host).to("cuda:0")


class DeviceCall:
    """One device call on fresh tensors with GUARD words behind every output array and the moves pre-filled with PATTERN;
    result() waits and returns numpy arrays in the host entry's layout after checking the guards.  `lib` is swmi.banded_width,
    or swmi.banded_ragged with band = None."""

    def __init__(self, lib, kind, batch, band, sm, go, ge, mask=0, traceback=True):
        n, words = batch.n, int(batch.move_offsets[-1])
        self.batch, self.traceback = batch, traceback
        self.keep = (_dev_bytes(batch.cat1), _dev_bytes(batch.cat2))
        self.scores = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.ends = torch.full((4 * n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.moves = torch.full((words + GUARD,), PATTERN, dtype=torch.int64, device="cuda:0") if traceback else None
        self.steps = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0") if traceback else None
        args = (self.keep[0], batch.off1, self.keep[1], batch.off2) + (() if band is None else (band,)) + (sm, go, ge)
        tail = (self.scores, self.ends, self.moves, self.steps, batch.diagonals, 0)
        if kind == GLOBAL:
            lib.global_device(*args, mask, *tail)
        else:
            lib.local_device(*args, *tail)

    def result(self):
        torch.cuda.synchronize()
        n, words = self.batch.n, int(self.batch.move_offsets[-1])
        scores, ends = self.scores.cpu().numpy(), self.ends.cpu().numpy()
        assert (scores[n:] == -7).all() and (ends[4 * n:] == -7).all(), "a guard word behind scores or ends was written"
        if not self.traceback:
            return scores[:n], ends[:4 * n].reshape(n, 4), None, None
        moves, steps = self.moves.cpu().numpy().view(np.uint64), self.steps.cpu().numpy()
        assert (steps[n:] == -7).all() and (moves[words:] == np.uint64(PATTERN)).all(), "a guard word behind steps or moves was written"
        return scores[:n], ends[:4 * n].reshape(n, 4), moves[:words], steps[:n].view(np.uint32)


def both_ways(bw, kind, batch, band, sm, go, ge, mask, want, what):
    """with a traceback and ends-only against `want`; returns the traceback result"""
    got = DeviceCall(bw, kind, batch, band, sm, go, ge, mask).result()
    assert_same(got, want, batch, what)
    eo = DeviceCall(bw, kind, batch, band, sm, go, ge, mask, traceback=False).result()
    assert_same(eo, want, batch, (what, "ends-only"), traceback=False)
    return got


def against_oracle(bw, orc, kind, batch, band, sm, go, ge, mask, what):
    return both_ways(bw, kind, batch, band, sm, go, ge, mask, orc.align(kind, batch, band, sm, go, ge, mask), what)


def kinds_and_masks(spread=None):
    """the local kind and every mask of the global kind; spread = (turn, per): `per` masks a turn, all twenty over four turns of 5"""
    masks = ALL_MASKS if spread is None else [(spread[0] * spread[1] + x) % 20 for x in range(spread[1])]
    return [(LOCAL, 0)] + [(GLOBAL, m) for m in masks]


def mixed_batch(rng):
    """about 40 alignments: lengths 0 .. 700, diagonals of both signs, empty sequences on either side and on both"""
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 701, 34), rng.integers(1, 701, 34))]
    shapes[:3] = [(700, 690), (1, 1), (63, 127)]
    diags = [int(x) for x in rng.integers(-90, 91, 34)]
    diags[2] = 64
    batch = related_batch(rng, shapes, diags)
    e, five = np.zeros(0, np.uint8), rng.integers(0, 4, 5, dtype=np.uint8)
    for d in (0, 64, -65):
        batch = batch + Batch([e, five, e], [five, e, e], [d, d, d])
    return batch


def test_band_128_equals_the_ragged_library_on_a_mixed_batch(bw, swmi_mod):
    rng = np.random.default_rng(1)
    batch = mixed_batch(rng)
    assert batch.n == 43 and batch.n % 4 != 0
    br = swmi_mod.banded_ragged
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            for traceback in (True, False):
                want = DeviceCall(br, kind, batch, None, SM, go, ge, mask, traceback=traceback).result()
                got = DeviceCall(bw, kind, batch, 128, SM, go, ge, mask, traceback=traceback).result()
                assert_same(got, want, batch, (kind, mask, go, ge, traceback), traceback=traceback)
                assert np.array_equal(got[1], want[1])
    assert (want[0] != 0).any()


def test_a_band_that_does_not_bind_equals_the_full_table_aligners(bw, swmi_mod, gpu):
    """Lengths up to 400 at band 1024 and diagonal 0: the whole table lies in the band, so every field and move equals
    swmi.local_full_affine_ragged / swmi.global_ragged.global_full_affine_ragged on the GPU (masks 0 .. 15: the full aligner has no
    END_ANYWHERE)."""
    rng = np.random.default_rng(2)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 401, 24), rng.integers(1, 401, 24))]
    shapes[:4] = [(400, 400), (400, 1), (1, 400), (399, 257)]
    batch = related_batch(rng, shapes, [0] * 24)
    batch = Batch(batch.seq1s, batch.seq2s, None)
    for go, ge in FORMS:
        sc, ends, moves, mo, steps = swmi_mod.local_full_affine_ragged(batch.seq1s, batch.seq2s, SM, go, ge)
        both_ways(bw, LOCAL, batch, 1024, SM, go, ge, 0, (sc, ends, moves, steps), ("local", go, ge))
        for mask in range(16):
            sc, ends, moves, mo, steps = swmi_mod.global_ragged.global_full_affine_ragged(batch.seq1s, batch.seq2s, SM, go, ge, free_ends=mask)
            both_ways(bw, GLOBAL, batch, 1024, SM, go, ge, mask, (sc, ends, moves, steps), ("global", mask, go, ge))
    assert int(steps.max()) > 400


@pytest.mark.parametrize("band", WIDTHS)
def test_drift_that_leaves_half_the_band_and_stays_in_it(bw, orc, band):
    """Pairs of 700 bases whose inserted (even k) or deleted (odd k) runs sum to 3 band / 8: the path ends beyond band / 4,
    the edge of a band half as wide, and inside band / 2.  At width `band` every case equals the unbounded restatement; at
    band / 2 (CPU only) every global case and at least 15 of 20 local cases differ from it, so the family binds.  The gaps are
    (4, 1) and (0, 1), not FORMS: a LOCAL path crosses a run only if the run costs less than the stretch beside it gains, about
    1.6 a base; at band 1024 a run is 96 bases beside 140, which (1, 3) prices at 286 against 224."""
    rng = np.random.default_rng(30 + band)
    runs = 3 if band < 1024 else 4
    batch = drift_batch(rng, 20, 700, runs, 3 * band // 8 // runs)
    unbounded = unbounded_for(batch)
    for turn, (go, ge) in enumerate(((4, 1), (0, 1))):
        free_l = orc.align(LOCAL, batch, unbounded, SM, go, ge)
        assert int(differs(orc.align(LOCAL, batch, band // 2, SM, go, ge), free_l).sum()) >= 15
        against_oracle(bw, orc, LOCAL, batch, band, SM, go, ge, 0, ("local", band, go, ge))
        assert_same(orc.align(LOCAL, batch, band, SM, go, ge), free_l, batch, ("the band is free", band))
        for mask in (0, 3, 12, 15, 19) if turn == 0 else (1, 6, 10, 16):
            free_g = orc.align(GLOBAL, batch, unbounded, SM, go, ge, mask)
            assert differs(orc.align(GLOBAL, batch, band // 2, SM, go, ge, mask), free_g).all(), mask
            got = against_oracle(bw, orc, GLOBAL, batch, band, SM, go, ge, mask, ("global", band, mask, go, ge))
            assert_same(got, free_g, batch, ("the band is free", band, mask))


@pytest.mark.parametrize("band", WIDTHS)
def test_lane_seams_and_the_bands_two_edges(bw, orc, band):
    """Related pairs along the band's lowest and highest diagonal and the ones beside them (lane 0's left and lane 63's upper
    neighbour are outside the band), and single gap runs of 2 K - 1, 2 K and 2 K + 1 bases that take the path across the borders
    of lanes 0 / 1, 31 / 32 and 62 / 63 in both directions."""
    rng = np.random.default_rng(40 + band)
    half, cells = band // 2, band // 64
    s1, s2, diags = [], [], []
    for off in (-half - 1, -half, -half + 1, half - 2, half - 1, half):          # the path's diagonal minus the band's centre
        a, b = related_pairs(rng, 1, 300, 300, 0)
        s1.append(a[0]), s2.append(b[0]), diags.append(-off)
    for border in (1, 32, 63):                                                   # the first diagonal of lane `border`
        for run in (cells - 1, cells, cells + 1):
            for insert in (True, False):
                # the path starts `run // 2 + 1` diagonals on one side of the lane border and crosses it with one gap run
                start = border * cells - half + (-(run // 2) - 1 if insert else run // 2)
                a = rng.integers(0, 4, 260, dtype=np.uint8)
                b = a.copy()
                b = np.concatenate([b[:130], rng.integers(0, 4, run, dtype=np.uint8), b[130:]]) if insert else np.concatenate([b[:130], b[130 + run:]])
                s1.append(a), s2.append(b), diags.append(-start)
    batch = Batch(s1, s2, diags)
    crossed = 0
    for turn, (go, ge) in enumerate(FORMS):
        for kind, mask in kinds_and_masks((turn, 10)):
            got = against_oracle(bw, orc, kind, batch, band, SM, go, ge, mask, (kind, band, mask, go, ge))
            if kind == LOCAL:
                crossed += int((got[3][6:] > 250).sum())
    assert crossed >= 30                                                         # the gapped paths were found whole


@pytest.mark.parametrize("band", WIDTHS)
def test_edge_diagonals_of_the_table(bw, orc, band):
    """The last diagonal that touches the table and the first that misses it on both sides, INT32_MIN / INT32_MAX, and
    all-match pairs of unequal lengths at gap costs 0 and 1."""
    rng = np.random.default_rng(50 + band)
    half = band // 2
    len1, len2 = 90, 70
    # cell (i, j) with j - i - d in [-half, half - 1]: j - i spans -len1 .. len2 with the borders, 1 - len1 .. len2 - 1 inside
    diags = [len2 + half, len2 + half + 1, len2 + half - 1, len2 + half - 2, -len1 - half + 1, -len1 - half, -len1 - half + 2, -len1 - half - 1,
             INT32_MIN, INT32_MAX, half, half + 1, -half + 1, -half]
    a, b = related_pairs(rng, len(diags), len1, len2)
    batch = Batch(list(a), list(b), diags)
    same = rng.integers(0, 4, 200, dtype=np.uint8)
    uneven = Batch([same, same[:150], same, same[:199]], [same[:150], same, same[:199], same], [0, 0, 0, 0])
    for turn, (go, ge) in enumerate(FORMS):
        for kind, mask in kinds_and_masks():
            against_oracle(bw, orc, kind, batch, band, SM, go, ge, mask, (kind, band, mask, go, ge))
    for turn, (go, ge) in enumerate(((0, 0), (1, 1), (0, 1), (1, 0))):
        for kind, mask in kinds_and_masks((turn, 5)):
            against_oracle(bw, orc, kind, uneven, band, SM, go, ge, mask, ("uneven", kind, band, mask, go, ge))


@pytest.mark.parametrize("band", WIDTHS)
def test_trips_move_word_seams_and_one_workgroup_of_unequal_wavefronts(bw, orc, band):
    """Swept rows at every remainder of the trip, paths of 31, 32, 33 and 64 steps, one workgroup whose four wavefronts run
    very different trip counts; DeviceCall holds the guard words."""
    rng = np.random.default_rng(60 + band)
    parts = [related_batch(rng, [(65, 70), (66, 71), (67, 69), (68, 70)], [0, 3, -3, 1])]
    same = [rng.integers(0, 4, L, dtype=np.uint8) for L in (31, 32, 33, 64)]
    parts.append(Batch(same, same, [0, 0, 0, 0]))
    parts.append(related_batch(rng, [(700, 690), (1, 1), (650, 700), (3, 500)], [0, 0, 40, -37]))
    batch = parts[0] + parts[1] + parts[2]
    seams = set()
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            got = against_oracle(bw, orc, kind, batch, band, SM, go, ge, mask, (kind, band, mask, go, ge))
            if kind == LOCAL or mask == 0:
                seams |= {int(got[3][k]) for k in range(4, 8)}
    assert seams == {31, 32, 33, 64}


@pytest.mark.parametrize("band", (512, 1024))
def test_the_walk_window_across_lane_borders(bw, orc, band):
    """A path longer than one window of 64 iterations with a horizontal run of 6 K + 1 bases -- three lane borders within a few
    iterations -- and a vertical one of the same length further on."""
    rng = np.random.default_rng(70 + band)
    run = 6 * (band // 128) + 1
    s1, s2 = [], []
    for k in range(6):
        a = rng.integers(0, 4, 600, dtype=np.uint8)
        b = np.concatenate([a[:200], rng.integers(0, 4, run, dtype=np.uint8), a[200:400 + 3 * k], a[400 + 3 * k + run:]])
        s1.append(a), s2.append(b)
    batch = Batch(s1, s2, [0, 5, -5, band // 4, -band // 4, 1])
    longest = 0
    for turn, (go, ge) in enumerate(((3, 1), (1, 2))):
        for kind, mask in kinds_and_masks((turn, 10)):
            got = against_oracle(bw, orc, kind, batch, band, match_matrix(3, -4), go, ge, mask, (kind, band, mask, go, ge))
            longest = max(longest, int(got[3].max()))
    assert longest > 600


def test_max_length(bw, orc):
    """16384 x 16384: one local alignment at band 1024 and one global one at band 256, with a traceback."""
    rng = np.random.default_rng(8)
    a, b = related_pairs(rng, 1, 16384, 16384)
    batch = Batch(list(a), list(b), [0])
    got = against_oracle(bw, orc, LOCAL, batch, 1024, SM, 5, 1, 0, "local 1024")
    assert got[3][0] > 16000
    against_oracle(bw, orc, GLOBAL, batch, 256, SM, 1, 3, 0, "global 256")


def test_the_host_entries_in_two_slices_and_the_module(bw, orc):
    """The count cap cuts 2^20 + 5 tiny alignments into two slices; the results land at caller positions.  Then the module on
    lists with a traceback, and its paths."""
    rng = np.random.default_rng(9)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 4, 101), rng.integers(1, 4, 101))]
    base = Batch([rng.integers(0, 4, x, dtype=np.uint8) for x, _ in shapes], [rng.integers(0, 4, y, dtype=np.uint8) for _, y in shapes],
                 rng.integers(-2, 3, 101))
    n = MAX_SLICE + 5
    reps = -(-n // 101)
    len1, len2 = np.tile(np.diff(base.off1.astype(np.int64)), reps)[:n], np.tile(np.diff(base.off2.astype(np.int64)), reps)[:n]
    off1, off2 = np.concatenate([[0], np.cumsum(len1)]).astype(np.uint64), np.concatenate([[0], np.cumsum(len2)]).astype(np.uint64)
    cat1, cat2 = np.tile(base.cat1, reps)[:int(off1[-1])], np.tile(base.cat2, reps)[:int(off2[-1])]
    d = np.tile(base.diagonals, reps)[:n]
    sm = match_matrix(2, -1)
    for band, (go, ge), (kind, mask) in zip(WIDTHS, FORMS + FORMS, [(LOCAL, 0), (GLOBAL, 0), (GLOBAL, 19), (LOCAL, 0)]):
        assert bw.slices_for(kind, band, off1, off2, traceback=False) == [MAX_SLICE, 5]
        want = orc.align(kind, base, band, sm, go, ge, mask, traceback=False)
        if kind == GLOBAL:
            got = bw.global_((cat1, off1), (cat2, off2), band, sm, go, ge, free_ends=mask, diagonals=d, traceback=False)
        else:
            got = bw.local((cat1, off1), (cat2, off2), band, sm, go, ge, diagonals=d, traceback=False)
        assert got[2] is None and got[3] is None and got[4] is None
        assert np.array_equal(got[0], np.tile(want[0], reps)[:n]) and np.array_equal(got[1], np.tile(want[1], (reps, 1))[:n]), (kind, mask, band)
    second = related_batch(rng, [(10, 600), (350, 350), (63, 127), (1, 1), (500, 90), (90, 500), (200, 210)], [30, 0, 64, 0, -300, 300, 2])
    for band in WIDTHS:
        for kind, mask in ((LOCAL, 0), (GLOBAL, 5)):
            want = orc.align(kind, second, band, SM, 5, 1, mask)
            if kind == GLOBAL:
                sc, ends, moves, mo, steps = bw.global_(second.seq1s, second.seq2s, band, SM, 5, 1, free_ends=mask, diagonals=second.diagonals)
            else:
                sc, ends, moves, mo, steps = bw.local(second.seq1s, second.seq2s, band, SM, 5, 1, diagonals=second.diagonals)
            assert np.array_equal(mo, second.move_offsets)
            assert_same((sc, ends, moves, steps), want, second, ("module", kind, band))
            paths = bw.paths((sc, ends, moves, mo, steps))
            for k in range(second.n):
                if sc[k] == NO_ALIGNMENT:
                    assert paths[k] is None
                else:
                    assert np.array_equal(paths[k], path_from(want[2][int(mo[k]):], want[3][k], want[1][k, 0], want[1][k, 1])), k
    bw.release_workspaces()


@pytest.mark.parametrize("kind,mask", [(LOCAL, 0), (GLOBAL, 10)], ids=["local", "global"])
def test_the_cpp_overloads(bw, orc, tmp_path, kind, mask):
    exe = str(tmp_path / "compat_banded_width")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_banded_width.cpp"), "-o", exe, "-L", lib, "-lswmi_banded_width", "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    rng = np.random.default_rng(12)
    batch = related_batch(rng, [(210, 190), (30, 300), (1, 1), (190, 210), (64, 70), (50, 50), (9, 1)], [0, 10, 0, 200, -3, 600, 0])
    batch = Batch(batch.seq1s[:6] + [batch.seq1s[6]], batch.seq2s[:6] + [np.zeros(0, np.uint8)], batch.diagonals)
    for name, arr in (("a", batch.cat1), ("b", batch.cat2), ("o1", batch.off1), ("o2", batch.off2), ("d", batch.diagonals)):
        arr.tofile(str(tmp_path / (name + ".bin")))
    for band, (go, ge) in zip((512, 256), FORMS):
        out = subprocess.run([exe, str(tmp_path), str(batch.n), str(kind), str(band), "2", "-3", str(go), str(ge), str(mask)], stdout=subprocess.PIPE,
                             text=True, check=True, timeout=120).stdout
        want = orc.align(kind, batch, band, SM, go, ge, mask)
        lines = out.strip().splitlines()
        assert len(lines) == batch.n
        for k, line in enumerate(lines):
            f = [int(x) for x in line.split()]
            path = path_from(want[2][int(batch.move_offsets[k]):], want[3][k], want[1][k, 0], want[1][k, 1])
            assert f[0] == want[0][k] and f[1:5] == list(want[1][k]) and f[5] == len(path), k
            assert f[6:] == [int(x) for x in path.reshape(-1)], k
        assert moves_of(want[2], want[3][0]).size > 100
        assert want[0][5] == (NO_ALIGNMENT if kind == GLOBAL else 0)
