"""The banded aligners for sequences up to 65536 long on the GPU (libswmi_banded_long.so, include/swmi_banded_long.h, DESIGN.md
section 41).  Up to 16384 the expected values are swmi.banded_width's; beyond, the two existing C restatements called with lo =
-band / 2, hi = band / 2 - 1 (banded_long_support), and once the full-table aligners for long sequences on the GPU: score, the
four ends, steps, and the moves word for word up to steps.  The shapes are the smallest that hold what is new: a best cell whose
column passes 32768 (the 16384 kernels pack i << 15 | j), ties across that edge, diagonals between 65536 and 65536 + band / 2
(which a clamp at 65536 moves), values at the int8 extremes over 65536 rows, and every width past row 16384."""
import os
import subprocess

import numpy as np
import pytest
import torch

from banded_long_support import (FORMS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_LEN, MOTIF, NO_ALIGNMENT, WIDTHS, Batch, WidthOracle, align_each,
                                 assert_same, drifting_pair, path_from, planted, related_batch)
from conftest import PKG, ROOT, match_matrix

pytestmark = pytest.mark.gpu

GUARD = 16                                  # guard words behind every output array
PATTERN = 0x5A5A5A5A5A5A5A5A
SM = match_matrix(2, -3)
OVERLAP = 15                                # SWMI_ENDS_OVERLAP


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return WidthOracle(tmp_path_factory.mktemp("banded_long_oracle"))


@pytest.fixture(scope="module")
def bl(swmi_mod):
    swmi_mod.banded_long.load()
    return swmi_mod.banded_long


def _dev_bytes(cat):
    host = np.ascontiguousarray(cat) if len(cat) else np.full(16, 255, np.uint8)
    return torch.from_numpy(host).to("cuda:0")


class DeviceCall:
    """One device call on fresh tensors with GUARD words behind every output array and the moves pre-filled with PATTERN;
    result() waits and returns numpy arrays in the host entry's layout after checking the guards.  `lib` is swmi.banded_long or
    swmi.banded_width."""

    def __init__(self, lib, kind, batch, band, sm, go, ge, mask=0, traceback=True):
        n, words = batch.n, int(batch.move_offsets[-1])
        self.batch, self.traceback = batch, traceback
        self.keep = (_dev_bytes(batch.cat1), _dev_bytes(batch.cat2))
        self.scores = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.ends = torch.full((4 * n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.moves = torch.full((words + GUARD,), PATTERN, dtype=torch.int64, device="cuda:0") if traceback else None
        self.steps = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0") if traceback else None
        args = (self.keep[0], batch.off1, self.keep[1], batch.off2, band, sm, go, ge)
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


def both_ways(bl, kind, batch, band, sm, go, ge, mask, want, what):
    """with a traceback and ends-only against `want`; returns the traceback result"""
    got = DeviceCall(bl, kind, batch, band, sm, go, ge, mask).result()
    assert_same(got, want, batch, what)
    eo = DeviceCall(bl, kind, batch, band, sm, go, ge, mask, traceback=False).result()
    assert_same(eo, want, batch, (what, "ends-only"), traceback=False)
    return got


# ---- 1. the old domain ----
@pytest.mark.parametrize("band", WIDTHS)
def test_up_to_16384_every_result_is_the_width_librarys(bl, swmi_mod, band):
    """43 mixed alignments of lengths 0 .. 700, diagonals of both signs, empty sequences on either side and on both: every
    field and move equals swmi.banded_width's, both kinds, masks 0, 5, 10, 15 and 16 .. 19, with a traceback and ends-only."""
    rng = np.random.default_rng(1)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 701, 34), rng.integers(1, 701, 34))]
    shapes[:3] = [(700, 690), (1, 1), (63, 127)]
    diags = [int(x) for x in rng.integers(-90, 91, 34)]
    batch = related_batch(rng, shapes, diags)
    e, five = np.zeros(0, np.uint8), rng.integers(0, 4, 5, dtype=np.uint8)
    for d in (0, band // 2, -band // 2 - 1):
        batch = batch + Batch([e, five, e], [five, e, e], [d, d, d])
    assert batch.n == 43
    bw = swmi_mod.banded_width
    for go, ge in FORMS:
        for kind, mask in [(LOCAL, 0)] + [(GLOBAL, m) for m in (0, 5, 10, 15, 16, 17, 18, 19)]:
            for traceback in (True, False):
                want = DeviceCall(bw, kind, batch, band, SM, go, ge, mask, traceback=traceback).result()
                got = DeviceCall(bl, kind, batch, band, SM, go, ge, mask, traceback=traceback).result()
                assert_same(got, want, batch, (kind, mask, go, ge, traceback), traceback=traceback)
                assert np.array_equal(got[1], want[1])
    assert (want[0] != 0).any()


# ---- 2. the position field ----
def test_a_best_cell_on_both_sides_of_column_32768(bl, orc):
    """Local kind, band 128: an all-mismatch background with one planted identical 40-mer whose end cell is known.  At j = 32768
    a position packed as i << 15 | j carries the column into the row."""
    cells = [(16385, 16385), (32767, 32767), (32768, 32768), (32769, 32770), (40000, 40050), (65536, 65536)]
    s1, s2, diags = [], [], []
    for i, j in cells:
        a, b = planted(MAX_LEN, MAX_LEN, [(i, j)])
        s1.append(a), s2.append(b), diags.append(50 if (i, j) == (40000, 40050) else j - i)
    for (len1, len2), (i, j) in (((100, MAX_LEN), (100, MAX_LEN)), ((MAX_LEN, 100), (MAX_LEN, 100))):      # about 160 rows swept
        a, b = planted(len1, len2, [(i, j)])
        s1.append(a), s2.append(b), diags.append(j - i)
        cells.append((i, j))
    batch = Batch(s1, s2, diags)
    for go, ge in FORMS:
        want = orc.align(LOCAL, batch, 128, SM, go, ge)
        assert [tuple(x) for x in want[1]] == [(i, j, i - MOTIF, j - MOTIF) for i, j in cells]       # the known cells
        assert (want[0] == 2 * MOTIF).all() and (want[3] == MOTIF).all()
        both_ways(bl, LOCAL, batch, 128, SM, go, ge, 0, want, ("planted", go, ge))


# ---- 3. first in row-major order across the field's edge ----
def test_the_first_cell_in_row_major_order_wins_across_the_fields_edge(bl, orc):
    first_row = planted(MAX_LEN, MAX_LEN, [(20000, 20000), (50000, 50000)])
    # (rows ten apart: two 10-mers of different letters, so that neither overwrites or matches the other)
    larger_column = planted(MAX_LEN, MAX_LEN, [(33000, 33050), (33010, 32990)], motif=10, distinct=True)
    batch = Batch([first_row[0], larger_column[0]], [first_row[1], larger_column[1]], [0, 0])
    one_row = planted(40000, 40000, [(30000, 29900), (30000, 30100)])                   # band 512: lanes 19 and 44 of row 30000
    wide = Batch([one_row[0]], [one_row[1]], [0])
    for go, ge in FORMS:
        want = orc.align(LOCAL, batch, 128, SM, go, ge)
        assert [tuple(x[:2]) for x in want[1]] == [(20000, 20000), (33000, 33050)] and list(want[0]) == [2 * MOTIF, 20]
        both_ways(bl, LOCAL, batch, 128, SM, go, ge, 0, want, ("two motifs", go, ge))
        want = orc.align(LOCAL, wide, 512, SM, go, ge)
        assert tuple(want[1][0][:2]) == (30000, 29900) and want[0][0] == 2 * MOTIF           # the left one
        both_ways(bl, LOCAL, wide, 512, SM, go, ge, 0, want, ("one row", go, ge))


# ---- 4. extremes at full length ----
@pytest.mark.parametrize("band", (128, 256))
def test_the_int8_extremes_over_65536_rows(bl, orc, band):
    """65536 x 65536, n = 2: all-match pairs, the second one's corner outside the band.  Global kind under GLOBAL, OVERLAP and
    END_ANYWHERE with a matrix of -128 everywhere and gaps (127, 127), and with +127 on the diagonal; local kind with +127: the
    score is 127 * 65536.  No domain rule: every value stays in int32 and -2^29 stays minus infinity."""
    rng = np.random.default_rng(4)
    a = rng.integers(0, 4, MAX_LEN, dtype=np.uint8)
    batch = Batch([a, a], [a, a], [0, band])                                     # band 2: diagonals band / 2 .. 3 band / 2 - 1 miss the corner
    low = np.full(16, -128, np.int8)
    high = low.copy()
    high[[0, 5, 10, 15]] = 127
    for sm, name in ((low, "low"), (high, "high")):
        for mask in (0, OVERLAP, 16):
            want = align_each(orc, GLOBAL, batch, band, sm, 127, 127, mask)
            got = DeviceCall(bl, GLOBAL, batch, band, sm, 127, 127, mask).result()
            assert_same(got, want, batch, (name, mask))
            if mask == 0:
                assert got[3][0] >= MAX_LEN and got[0][1] == NO_ALIGNMENT and got[3][1] == 0
                assert got[0][0] == (127 * MAX_LEN if name == "high" else -128 * MAX_LEN)
    want = align_each(orc, LOCAL, batch, band, high, 127, 127)
    got = both_ways(bl, LOCAL, batch, band, high, 127, 127, 0, want, "local high")
    assert got[0][0] == 127 * MAX_LEN and got[3][0] == MAX_LEN and tuple(got[1][0]) == (MAX_LEN, MAX_LEN, 0, 0)


# ---- 5. diagonals ----
def _diagonals(len1, len2, half):
    # j - i spans -len1 .. len2 with the borders; the band is d - half .. d + half - 1
    return [len2 + half, len2 + half + 1, len2 + half - 1, -len1 - half + 1, -len1 - half, -len1 - half + 2, 65536, -65536, 65537, -65537,
            INT32_MIN, INT32_MAX, len2 - len1]


@pytest.mark.parametrize("long_side", (1, 2))
@pytest.mark.parametrize("band", WIDTHS)
def test_diagonals_at_and_beyond_the_tables_edge(bl, orc, band, long_side):
    """The long side 65536, the short side 80: the last diagonal that touches the table and the first that misses it on both
    sides, +-65536 and +-65537, INT32_MIN and INT32_MAX.  With len2 = 65536 the diagonals in (65536, 65536 + band / 2] touch
    the table, and a clamp at 65536 moves them."""
    rng = np.random.default_rng(50 + band + long_side)
    len1, len2 = (MAX_LEN, 80) if long_side == 1 else (80, MAX_LEN)
    diags = _diagonals(len1, len2, band // 2)
    long_ = rng.integers(0, 4, MAX_LEN, dtype=np.uint8)
    s1, s2 = [], []
    for d in diags:
        at = int(np.clip(-d if long_side == 1 else d, 0, MAX_LEN - 80))          # the short side is related to the long one where the band lies
        short = np.where(rng.random(80) < 0.1, rng.integers(0, 4, 80, dtype=np.uint8), long_[at:at + 80]).astype(np.uint8)
        s1.append(long_ if long_side == 1 else short), s2.append(short if long_side == 1 else long_)
    batch = Batch(s1, s2, diags)
    go, ge = FORMS[(band // 128 + long_side) % 2]
    want = align_each(orc, LOCAL, batch, band, SM, go, ge)
    assert want[0][-1] > 100 and want[0][1] == 0 and want[0][4] == 0
    both_ways(bl, LOCAL, batch, band, SM, go, ge, 0, want, ("local", band))
    # (the global restatement fills 24 bytes a band cell of len1 + 1 rows before it starts: with len1 = 65536 fewer masks run)
    for mask in (0, OVERLAP, 19) if long_side == 2 else (OVERLAP, 19) if band <= 256 else (19,):
        want = align_each(orc, GLOBAL, batch, band, SM, go, ge, mask)
        assert want[0][1] == NO_ALIGNMENT and want[0][4] == NO_ALIGNMENT and want[0][10] == NO_ALIGNMENT
        assert (want[0][-1] != NO_ALIGNMENT) == (mask != 0)                      # (the origin is outside the band: no global path)
        if mask == 19 and long_side == 2:
            assert want[0][0] != NO_ALIGNMENT                                    # 65536 + band / 2 holds cell (0, 65536)
        both_ways(bl, GLOBAL, batch, band, SM, go, ge, mask, want, ("global", band, mask))


# ---- 6. every width past the old limit ----
@pytest.mark.parametrize("band", (256, 512, 1024))
def test_every_width_past_row_16384(bl, orc, band):
    """Lengths 16385 .. 17000: related pairs with one run of 3 band / 8 bases inserted or deleted behind row 16384, in either
    sequence, gap runs of 6 K + 1 bases in both directions there, and a plain pair of 16385; both kinds with a traceback against
    the restatement.  The global paths cross the run whole: the corner lies 3 band / 8 diagonals from the main one."""
    rng = np.random.default_rng(60 + band)
    run = 6 * (band // 128) + 1
    s1, s2 = [], []
    for k, length in enumerate((16990, 17000, 16900, 16800)):
        a, b = drifting_pair(rng, length, 16390, 1, 3 * band // 8, insert=k % 2 == 0)
        s1.append(a if k < 2 else b[:17000]), s2.append(b[:17000] if k < 2 else a)
    for insert in (True, False):
        a, b = drifting_pair(rng, 16800, 16500, 1, run, insert)
        s1.append(a), s2.append(b)
    a, b = drifting_pair(rng, 16385, 16385, 0, 0, True)
    s1.append(a), s2.append(b)
    batch = Batch(s1, s2, [0] * 7)
    assert all(16385 <= len(x) <= 17000 for x in batch.seq1s + batch.seq2s)
    for turn, (go, ge) in enumerate(((4, 1), (1, 2))):
        want = align_each(orc, LOCAL, batch, band, SM, go, ge)
        got = both_ways(bl, LOCAL, batch, band, SM, go, ge, 0, want, ("local", band, go, ge))
        assert (got[3] > 16000).all()
        mask = (0, OVERLAP)[turn]
        want = align_each(orc, GLOBAL, batch, band, SM, go, ge, mask)
        assert (want[0] != NO_ALIGNMENT).all()
        both_ways(bl, GLOBAL, batch, band, SM, go, ge, mask, want, ("global", band, mask))


# ---- 7. against the full table on the GPU ----
def test_paths_inside_512_diagonals_equal_the_full_table_aligners(bl, swmi_mod, orc, gpu):
    """Four related pairs of 20000 x 20000 whose inserted and deleted runs keep the path within +-200 diagonals: at band 512 and
    1024 every field and move equals swmi.local_long.local_long_affine's and swmi.global_long.global_long_affine's.  That all
    four qualify is held here: the full table's own path stays within 200 diagonals of the main one, and the restatement at
    band 512 on the CPU gives the full table's result."""
    rng = np.random.default_rng(7)
    s1, s2 = [], []
    for k in range(4):
        a = rng.integers(0, 4, 20000, dtype=np.uint8)
        b = np.where(rng.random(20000) < 0.04, rng.integers(0, 4, 20000, dtype=np.uint8), a).astype(np.uint8)
        ins = rng.integers(0, 4, 40 + 30 * k, dtype=np.uint8)
        b = np.concatenate([b[:5000], ins, b[5000:12000], b[12000 + len(ins):]])         # drifts up by the run, and back
        assert len(b) == 20000
        s1.append(a), s2.append(b)
    batch = Batch(s1, s2, [0] * 4)
    go, ge = 5, 1
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0)):
        if kind == LOCAL:
            sc, ends, moves, steps = swmi_mod.local_long.local_long_affine(np.stack(s1), np.stack(s2), SM, go, ge)
        else:
            sc, ends, moves, steps = swmi_mod.global_long.global_long_affine(np.stack(s1), np.stack(s2), SM, go, ge, free_ends=mask)
        full = (sc, ends, np.ascontiguousarray(moves).reshape(-1), steps)
        for k in range(4):
            path = path_from(full[2][int(batch.move_offsets[k]):], steps[k], ends[k, 0], ends[k, 1])
            assert len(path) > 19000 and int(np.abs(path[:, 1] - path[:, 0]).max()) <= 200, k       # all four qualify
        assert_same(align_each(orc, kind, batch, 512, SM, go, ge, mask), full, batch, ("the restatement at 512", kind))
        for band in (512, 1024):
            both_ways(bl, kind, batch, band, SM, go, ge, mask, full, ("band", band, kind))
    swmi_mod.local_long.local_long_affine_release_workspaces()
    swmi_mod.global_long.global_long_affine_release_workspaces()


# ---- 8. the host entries in two slices by the byte budget ----
def test_the_host_entries_in_two_slices_by_the_byte_budget_and_the_module(bl, orc):
    """Band 1024 with a traceback, shape (65536, 600): the codes are sized by len1, 33 587 200 bytes an alignment, so a slice
    holds 130 and 131 alignments take two; about 1100 rows are swept.  Results at caller positions, guard words behind every
    output."""
    rng = np.random.default_rng(9)
    n = 131
    long_ = rng.integers(0, 4, MAX_LEN, dtype=np.uint8)
    base = []
    for k in range(3):
        at = 1000 + 30000 * k
        base.append((at, np.where(rng.random(600) < 0.08, rng.integers(0, 4, 600, dtype=np.uint8), long_[at:at + 600]).astype(np.uint8)))
    s2 = [base[k % 3][1] for k in range(n)]
    diags = np.array([-base[k % 3][0] + (k % 2) for k in range(n)], np.int32)
    off1, off2 = MAX_LEN * np.arange(n + 1, dtype=np.uint64), 600 * np.arange(n + 1, dtype=np.uint64)
    assert bl.slices_for(LOCAL, 1024, off1, off2) == bl.slices_for(GLOBAL, 1024, off1, off2) == [130, 1]
    cat1, cat2 = np.tile(long_, n), np.concatenate(s2)
    few = Batch([long_] * 6, s2[:6], diags[:6])                                   # every (k % 3, k % 2) once
    lib = bl.load()
    mo = bl.move_offsets(off1, off2)
    words = int(mo[-1])
    for kind, mask in ((LOCAL, 0), (GLOBAL, 19)):
        want = align_each(orc, kind, few, 1024, SM, 5, 1, mask)
        scores, ends = np.full(n + GUARD, -7, np.int32), np.full(4 * n + GUARD, -7, np.int32)
        moves, steps = np.full(words + GUARD, PATTERN, np.uint64), np.full(n + GUARD, 77, np.uint32)
        sm = np.ascontiguousarray(SM, np.int8)
        head = (cat1.ctypes.data, off1.ctypes.data, cat2.ctypes.data, off2.ctypes.data, n, diags.ctypes.data, 1024, sm.ctypes.data, 5, 1)
        tail = (scores.ctypes.data, ends.ctypes.data, moves.ctypes.data, steps.ctypes.data)
        rc = lib.swmi_banded_long_global(*head, mask, *tail) if kind == GLOBAL else lib.swmi_banded_long_local(*head, *tail)
        assert rc == 0, bl.last_error()
        assert (scores[n:] == -7).all() and (ends[4 * n:] == -7).all() and (steps[n:] == 77).all() and (moves[words:] == np.uint64(PATTERN)).all()
        assert (want[3] > 500).all()
        for k in range(n):
            w = k % 6
            assert scores[k] == want[0][w] and tuple(ends[4 * k:4 * k + 4]) == tuple(want[1][w]) and steps[k] == want[3][w], (kind, k)
            got_path = path_from(moves[int(mo[k]):], steps[k], ends[4 * k], ends[4 * k + 1])
            assert np.array_equal(got_path, path_from(want[2][int(few.move_offsets[w]):], want[3][w], want[1][w, 0], want[1][w, 1])), (kind, k)
    # the module on lists, and its paths through the long expander
    sc, en, mv, mo3, st = bl.local(few.seq1s[:3], few.seq2s[:3], 1024, SM, 5, 1, diagonals=few.diagonals[:3])
    assert np.array_equal(mo3, few.move_offsets[:4]) and (st > 500).all()
    paths = bl.paths((sc, en, mv, mo3, st))
    for k in range(3):
        assert paths[k].shape == (int(st[k]) + 1, 2) and tuple(paths[k][-1]) == (en[k, 0], en[k, 1]) and tuple(paths[k][0]) == (en[k, 2], en[k, 3])
    bl.release_workspaces()


@pytest.mark.parametrize("kind,mask", [(LOCAL, 0), (GLOBAL, 10)], ids=["local", "global"])
def test_the_cpp_overloads(bl, orc, tmp_path, kind, mask):
    exe = str(tmp_path / "compat_banded_long")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_banded_long.cpp"), "-o", exe, "-L", lib, "-lswmi_banded_long", "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    rng = np.random.default_rng(12)
    batch = related_batch(rng, [(210, 190), (30, 300), (1, 1), (16500, 16450), (64, 70), (50, 50), (9, 1)], [0, 10, 0, -20, -3, 600, 0])
    batch = Batch(batch.seq1s[:6] + [batch.seq1s[6]], batch.seq2s[:6] + [np.zeros(0, np.uint8)], batch.diagonals)
    for name, arr in (("a", batch.cat1), ("b", batch.cat2), ("o1", batch.off1), ("o2", batch.off2), ("d", batch.diagonals)):
        arr.tofile(str(tmp_path / (name + ".bin")))
    band, (go, ge) = 512, FORMS[0]
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
    assert want[3][3] > 16000 and want[0][5] == (NO_ALIGNMENT if kind == GLOBAL else 0)
