"""Helpers of the long local aligners' tests (test_local_long_gpu.py, test_local_long_affine_gpu.py, test_local_long_cpu.py): the
shapes at the kernels' stripe edges, the planted pairs and the parameter sets are the long global aligners'
(global_long_support.py), by import.  The definitions stay the two C restatements tests/native/local_full_oracle.c and
local_full_affine_oracle.c, which take any lengths."""
import numpy as np

from global_long_support import (AFFINE_PARAMS, LEN1S, LEN2S, LINEAR_PARAMS, MAX_LEN, STRIPE, crosses, noisy_copy, plant,  # noqa: F401
                                 planted_batch)
from local_full_affine_support import LocalFullAffineOracle  # noqa: F401
from local_full_support import LocalFullOracle, assert_same, move_words, moves_of, path_from  # noqa: F401

DIAG, UP, LEFT = 3, 2, 1


def local_batch(len1, len2, seed):
    """planted_batch's four pairs and two quiet ones: seq1 over {0, 1}, seq2 over {2, 3} but for one exact copy of seq1 across
    column 16384 (pair 4) and across column 32768 where len2 reaches it (pair 5; else across 16384, a column further).  A local
    path of a seq1 of one or three bases ends on the first best cell, which in a random seq2 lies near column 1; in a quiet
    pair the copy holds the only matches, so its path crosses the boundary whatever len1 is."""
    a4, b4 = planted_batch(len1, len2, seed)
    rng = np.random.default_rng(seed + 1)
    a = rng.integers(0, 2, (2, len1), dtype=np.uint8)
    b = rng.integers(2, 4, (2, len2), dtype=np.uint8)
    plant(b[0], a[0], STRIPE)
    plant(b[1], a[1], 2 * STRIPE if len2 > 2 * STRIPE else STRIPE + 1)
    return np.concatenate([a4, a]), np.concatenate([b4, b])


def two_copies(s, len2=40000, ends=(10000, 30000), fill=3):
    """A seq2 of `fill` that holds s ending at each column of `ends`."""
    b = np.full(len2, fill, np.uint8)
    for e in ends:
        b[e - len(s):e] = s
    return b


def checksum(path):
    s = 0
    for i, j in path:
        s = (s * 1000003 + int(i) * 32771 + int(j)) & 0xFFFFFFFFFFFFFFFF
    return s


# ---- what the linear and the affine test files share: one body per check, the family as an argument -----------------------

class Family:
    """The linear (gaps = (gap,)) or the affine (gaps = (open, extend)) long local aligner: its Python entries, its fixed-length
    twin, its restatement and its parameter sets."""

    def __init__(self, affine):
        self.affine = affine
        self.params = [(sm, (go, ge)) for sm, go, ge in AFFINE_PARAMS] if affine else [(sm, (g,)) for sm, g in LINEAR_PARAMS]
        self.name = "local_long_affine" if affine else "local_long"

    def oracle(self, tmpdir):
        return (LocalFullAffineOracle if self.affine else LocalFullOracle)(tmpdir)

    def align(self, gpu, a, b, sm, gaps, traceback=True):
        return getattr(gpu.local_long, self.name)(a, b, sm, *gaps, traceback=traceback)

    def fixed(self, gpu, a, b, sm, gaps):
        return (gpu.local_full_affine if self.affine else gpu.local_full)(a, b, sm, *gaps)

    def device(self, gpu, *args, **kw):
        return getattr(gpu.local_long, self.name + "_device")(*args, **kw)

    def release(self, gpu):
        getattr(gpu.local_long, self.name + "_release_workspaces")()

    def gaps(self, gap):
        """The gap of a hand-built linear case for this family: affine with open == extend is the linear recurrence."""
        return (gap, gap) if self.affine else (gap,)

    def both(self, gpu, oracle, a, b, sm, gaps, what):
        """The host entry with traceback and ends-only against the restatement; returns the restatement's results."""
        want = oracle.align(a, b, sm, *gaps)
        assert_same(self.align(gpu, a, b, sm, gaps), want, what)
        sc, ends, mv, st = self.align(gpu, a, b, sm, gaps, traceback=False)
        assert mv is None and st is None
        assert_same((sc, ends, None, None), want, (what, "ends-only"), traceback=False)
        return want

    def one(self, gpu, oracle, a, b, sm, gaps, what):
        """One pair, traceback and ends-only, bit-exact against the restatement: (score, ends[4], the walk's codes) of the
        restatement, for the caller's hand-worked values."""
        sc, ends, mv, st = self.both(gpu, oracle, a[None], b[None], sm, gaps, what)
        return int(sc[0]), [int(x) for x in ends[0]], list(moves_of(mv[0], st[0]))


def check_stripe_edges(fam, gpu, oracle, len2, len1):
    """One (len2, len1) of the grid: two parameter sets, rotating over the shapes; planted_batch's pairs and two quiet ones.
    Some path of the case crosses column 16384, and where len2 > 32768 some path crosses column 32768 (asserted on the
    restatement's results)."""
    a, b = local_batch(len1, len2, 1000 * LEN2S.index(len2) + len1)
    over1 = over2 = False
    for r in range(2):
        sm, gaps = fam.params[(2 * r + LEN1S.index(len1) + LEN2S.index(len2)) % len(fam.params)]
        want = fam.both(gpu, oracle, a, b, sm, gaps, (len1, len2, gaps))
        over1 |= bool(crosses(want[1], STRIPE).any())
        over2 |= bool(crosses(want[1], 2 * STRIPE).any())
    assert over1
    assert over2 or len2 <= 2 * STRIPE


def check_long_seq1(fam, gpu, oracle, len1, len2):
    rng = np.random.default_rng(len1)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    b[0] = a[0, len1 // 2: len1 // 2 + len2]
    for sm, gaps in fam.params[:4]:
        fam.both(gpu, oracle, a, b, sm, gaps, (len1, len2, gaps))


def check_both_long(fam, gpu, oracle, sm, gaps):
    """(20000, 40000): seq1's tail is a noisy copy of a stretch of seq2 that starts in stripe 0 and ends in stripe 2."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 40000), dtype=np.uint8)
    src = a[0, 1000:]
    noisy = np.where(rng.random(len(src)) < 0.1, rng.integers(0, 4, len(src)), src).astype(np.uint8)
    noisy = np.concatenate([noisy[:7000], noisy[7005:], rng.integers(0, 4, 5, dtype=np.uint8)])
    b[0, 15000:15000 + len(noisy)] = noisy
    want = oracle.align(a, b, sm, *gaps)
    assert crosses(want[1], STRIPE).all() and crosses(want[1], 2 * STRIPE).all()
    assert_same(fam.align(gpu, a, b, sm, gaps), want, "both long")


def tie_lower_row_later_stripe():
    """seq1 = s, 80 x `2`, u (s, u random 0/1 60-mers); seq2 all `3` with u at columns 9941 .. 10000 and s at 29941 .. 30000."""
    rng = np.random.default_rng(6)
    s, u = rng.integers(0, 2, 60, dtype=np.uint8), rng.integers(0, 2, 60, dtype=np.uint8)
    a = np.concatenate([s, np.full(80, 2, np.uint8), u])
    b = np.full(40000, 3, np.uint8)
    b[9940:10000] = u
    b[29940:30000] = s
    return a, b


def check_full_size_identical(fam, gpu, match, gaps):
    """Identical sequences of 65536: the diagonal scores 65536 match, the most a local score can be (the top of the key range),
    and its last cell is the only one that holds it."""
    a = np.random.default_rng(9).integers(0, 4, (1, MAX_LEN), dtype=np.uint8)
    sm = np.full((4, 4), -match, np.int8)
    np.fill_diagonal(sm, match)
    sm = sm.reshape(16)
    sc, ends, mv, st = fam.align(gpu, a, a, sm, gaps)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, 0, 0] and int(st[0]) == MAX_LEN
    assert np.all(moves_of(mv[0], st[0]) == DIAG)
    sc, ends, _, _ = fam.align(gpu, a, a, sm, gaps, traceback=False)
    assert int(sc[0]) == match * MAX_LEN and [int(x) for x in ends[0]] == [MAX_LEN, MAX_LEN, -1, -1]


def check_equals_fixed(fam, gpu, len1, len2):
    rng = np.random.default_rng(len1 + len2)
    a = rng.integers(0, 4, (2, len1), dtype=np.uint8)
    b = rng.integers(0, 4, (2, len2), dtype=np.uint8)
    w = min(len1, len2)
    b[0, len2 - w:] = np.where(rng.random(w) < 0.1, rng.integers(0, 4, w), a[0, len1 - w:])
    for sm, gaps in fam.params:
        assert_same(fam.align(gpu, a, b, sm, gaps), fam.fixed(gpu, a, b, sm, gaps), (len1, len2, gaps))


def check_host_entry_and_expand(fam, gpu, oracle, sm, gaps):
    """n = 5 of (129, 32769), host to host with a traceback; expand_moves rebuilds each path from its start cell to its end
    cell, and the path equals the one the moves spell in numpy."""
    a4, b4 = planted_batch(129, 32769, 77)
    a, b = np.concatenate([a4, a4[:1]]), np.concatenate([b4, b4[1:2]])
    want = oracle.align(a, b, sm, *gaps)
    got = fam.align(gpu, a, b, sm, gaps)
    assert_same(got, want, "host n = 5")
    sc, ends, mv, st = got
    for k in range(5):
        pos = gpu.local_long.expand_moves(mv[k], st[k], ends[k, 0], ends[k, 1])
        assert pos.shape == (int(st[k]) + 1, 2)
        assert tuple(pos[0]) == (int(ends[k, 2]), int(ends[k, 3])) and tuple(pos[-1]) == (int(ends[k, 0]), int(ends[k, 1]))
        assert np.array_equal(pos, path_from(mv[k], st[k], ends[k, 0], ends[k, 1]))


def check_device_entry(fam, gpu, oracle, sm, gaps):
    """The _device entry on torch buffers, traceback and ends-only, at a shape with a carry (len2 > 16384); then release."""
    import torch
    a, b = planted_batch(64, 16400, 31)
    n, mw = 4, gpu.local_long.move_words(64, 16400)
    want = oracle.align(a, b, sm, *gaps)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    ends = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    fam.device(gpu, da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, *gaps, sc.data_ptr(), ends.data_ptr(), mv.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32)), want, "device")
    fam.device(gpu, da.data_ptr(), 64, db.data_ptr(), 16400, n, sm, *gaps, sc.data_ptr(), ends.data_ptr())
    torch.cuda.synchronize()
    assert_same((sc.cpu().numpy(), ends.cpu().numpy(), None, None), want, "device ends-only", traceback=False)
    fam.release(gpu)


# ---- hand-built cases: the values are worked out in the docstrings, and the restatement has to give them too ---------------

def _mm(match, mismatch):
    sm = np.full((4, 4), mismatch, np.int8)
    np.fill_diagonal(sm, match)
    return sm.reshape(16)


def check_tie_lower_row_in_the_later_stripe(fam, gpu, oracle):
    """Both 60-mers score 60 * 3: u ends on (200, 10000) in stripe 0, s on (60, 30000) in stripe 1.  The first cell in row-major
    order is the one in row 60, in the LATER stripe: a fold that prefers the earlier stripe fails here."""
    a, b = tie_lower_row_later_stripe()
    score, ends, codes = fam.one(gpu, oracle, a, b, _mm(3, -3), fam.gaps(2), "tie, lower row later")
    assert score == 180 and ends == [60, 30000, 0, 29940] and codes == [DIAG] * 60


def check_tie_on_one_row(fam, gpu, oracle, gap):
    """seq1 = s, seq2 holds s ending at 10000 and at 30000: both cells of row 60 hold 180 and the earlier column wins; with gap
    0 the value also fills the row right of column 10000."""
    s = np.random.default_rng(6).integers(0, 2, 60, dtype=np.uint8)
    score, ends, codes = fam.one(gpu, oracle, s, two_copies(s), _mm(3, -3), fam.gaps(gap), ("tie on one row", gap))
    assert score == 180 and ends == [60, 10000, 0, 9940] and codes == [DIAG] * 60


def check_start_at_the_boundary(fam, gpu, oracle, first):
    """An 80-mer over {0, 1} whose first column is `first`, in a seq2 over {2, 3}: 80 * 5, from (0, first - 1)."""
    rng = np.random.default_rng(first)
    s = rng.integers(0, 2, 80, dtype=np.uint8)
    b = rng.integers(2, 4, 17000, dtype=np.uint8)
    b[first - 1:first + 79] = s
    score, ends, codes = fam.one(gpu, oracle, s, b, _mm(5, -4), fam.gaps(3), ("start at", first))
    assert score == 400 and ends == [80, first + 79, 0, first - 1] and codes == [DIAG] * 80


def check_left_run_across_the_boundary(fam, gpu, oracle):
    """seq2 = 16184 foreign bases, s[:100], 200 foreign bases over columns 16285 .. 16484, s[100:], a foreign tail; gap 1:
    100 diagonals (500), 200 left moves (300 > 0), 100 diagonals: 800."""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 2, 200, dtype=np.uint8)
    b = np.concatenate([rng.integers(2, 4, 16184, dtype=np.uint8), s[:100], rng.integers(2, 4, 200, dtype=np.uint8), s[100:],
                        rng.integers(2, 4, 300, dtype=np.uint8)])
    score, ends, codes = fam.one(gpu, oracle, s, b, _mm(5, -4), fam.gaps(1), "left run")
    assert score == 800 and ends == [200, 16584, 0, 16184]
    assert codes == [DIAG] * 100 + [LEFT] * 200 + [DIAG] * 100


def check_up_run_in_stripe_1(fam, gpu, oracle):
    """seq1 = 200 bases, 120 foreign ones, 200 bases; seq2 holds the 400 from column 17001 on; gap 1.  The values are the
    restatement's; the path is 200 diagonals, 120 up moves, 200 diagonals."""
    rng = np.random.default_rng(4)
    s = rng.integers(0, 2, 400, dtype=np.uint8)
    a = np.concatenate([s[:200], rng.integers(2, 4, 120, dtype=np.uint8), s[200:]])
    b = np.concatenate([rng.integers(2, 4, 17000, dtype=np.uint8), s, rng.integers(2, 4, 50, dtype=np.uint8)])
    score, ends, codes = fam.one(gpu, oracle, a, b, _mm(5, -4), fam.gaps(1), "up run")
    assert score == 2000 - 120 and ends == [520, 17400, 0, 17000]
    assert codes == [DIAG] * 200 + [UP] * 120 + [DIAG] * 200


def check_all_mismatch(fam, gpu, oracle):
    """(40, 16385), seq1 all 0 and seq2 all 1: no cell is above 0, so the score is 0 at (0, 0) with an empty walk; ends-only
    the start cell is (-1, -1)."""
    a, b = np.zeros(40, np.uint8), np.ones(16385, np.uint8)
    score, ends, codes = fam.one(gpu, oracle, a, b, _mm(2, -3), fam.gaps(1), "all mismatch")
    assert score == 0 and ends == [0, 0, 0, 0] and codes == []
    sc, e, _, _ = fam.align(gpu, a[None], b[None], _mm(2, -3), fam.gaps(1), traceback=False)
    assert int(sc[0]) == 0 and [int(x) for x in e[0]] == [0, 0, -1, -1]


def check_last_stripe_of_one_column(fam, gpu, oracle, len2):
    """The last column is the only valid one of the last stripe (16385) or of its last wavefront (17409): seq1 = 50 bases that
    end seq2, then 30 foreign ones: 50 * 4 at (50, len2)."""
    s = np.random.default_rng(len2).integers(0, 2, 50, dtype=np.uint8)
    a = np.concatenate([s, np.full(30, 2, np.uint8)])
    b = np.full(len2, 3, np.uint8)
    b[len2 - 50:] = s
    score, ends, codes = fam.one(gpu, oracle, a, b, _mm(4, -5), fam.gaps(3), ("one column", len2))
    assert score == 200 and ends == [50, len2, 0, len2 - 50] and codes == [DIAG] * 50


def check_walk_straddles_the_boundary(fam, gpu, oracle):
    """A 3000-base noisy copy across column 16384: the walk takes more than 20 staging blocks of 128 rows and crosses the
    boundary inside one."""
    rng = np.random.default_rng(8)
    a = rng.integers(0, 4, (1, 3000), dtype=np.uint8)
    b = rng.integers(0, 4, (1, 20000), dtype=np.uint8)
    b[0, 14900:17900] = np.where(rng.random(3000) < 0.1, rng.integers(0, 4, 3000), a[0])
    want = oracle.align(a, b, _mm(5, -4), *fam.gaps(3))
    assert crosses(want[1], STRIPE).all() and int(want[1][0, 0] - want[1][0, 2]) > 20 * 128
    assert_same(fam.align(gpu, a, b, _mm(5, -4), fam.gaps(3)), want, "straddle")


def check_bytes_0_to_255(fam, gpu, oracle):
    """Bases are taken modulo 4: a batch of arbitrary bytes equals the batch of their low two bits."""
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (2, 129), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 17409), dtype=np.uint8)
    b[0, 16300:16429] = a[0]
    sm, gaps = fam.params[3]
    want = oracle.align(a & 3, b & 3, sm, *gaps)
    assert_same(fam.align(gpu, a, b, sm, gaps), want, "bytes")


def check_cpp_overloads(fam, gpu, oracle, tmp_path):
    """tests/native/compat_local_long.cpp on five pairs of (129, 17409): SmithWaterman_xlong_mi355x one by one and its batch form
    in pieces of 2 (with a fourth argument: the affine pair at open == extend == that gap): score, path length, end cell and
    a checksum of every path against the restatement."""
    import os
    import shutil
    import subprocess

    from conftest import PKG, ROOT
    assert shutil.which("g++") is not None, "g++ not available"
    exe = str(tmp_path / "compat_local_long")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_local_long.cpp"), "-o", exe, "-L", lib, "-lswmi", "-lpthread",
                            "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    a4, b4 = planted_batch(129, 17409, 91)
    a, b = np.concatenate([a4, a4[:1]]), np.concatenate([b4, b4[1:2]])
    sm = fam.params[3][0]
    data = tmp_path / "batch.bin"
    with open(data, "wb") as fh:
        fh.write(np.array([5, 129, 17409, 3], np.int32).tobytes() + np.asarray(sm, np.int8).tobytes())
        for k in range(5):
            fh.write(a[k].tobytes() + b[k].tobytes())
    sc, ends, mv, st = oracle.align(a, b, sm, *fam.gaps(3))
    run = subprocess.run([exe, str(data), "2"] + (["3"] if fam.affine else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "single 0", lines[-1]
    rows = [tuple(map(int, line.split())) for line in lines[:-1]]
    assert len(rows) == 5
    for k in range(5):
        path = path_from(mv[k], st[k], ends[k, 0], ends[k, 1])
        assert rows[k] == (int(sc[k]), len(path), int(ends[k, 0]), int(ends[k, 1]), checksum(path)), k
