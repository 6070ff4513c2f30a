"""Helpers of the X-drop semi-global sweeps' edge tests (test_sg_edges_cpu.py, test_sg_edges_gpu.py): the structured,
deterministic batch of 16384-mer pairs that puts sg_forward_split_kernel / sg_forward_lane_kernel, the character pre-pass and
the walk at the X-drop threshold, the calm predicate's margin, the matrix edges, ties, non-base bytes and the records'
seams; and tests/native/sg_xdrop_profile.c compiled into a temporary directory, which says window by window what the
reference's recurrence goes through on an input.  Expected results always come from oracle/sg_oracle.c (conftest's
`oracle.semiglobal`); the hand-worked values kept here are asserted on top of that."""
import ctypes
import functools
import os
import subprocess
from collections import namedtuple

import numpy as np

from conftest import ROOT

LEN = 16384
XDROP = 70
WINDOW = 8
FULL = dict(score=None, length=LEN + 1, end=(LEN, LEN))     # (a template: the pure diagonal to the last cell)

STRETCH_AT = (3000, 8000, 12000)
STRETCHES = (69, 70, 71, 72)
PREFIXES = (1, 7, 8, 9, 15, 16, 17, 100)
SHIFTS = (1, 8, 15, 16, 17, 24, 30, 31)
NON_BASES = (0x04, 0x7C, 0x7F, 0x80, 0x83, 0xFC, 0xFF)
# where the non-base bytes go: the positions the character streams' words, tiles and top-ups begin and end at, then one in
# each byte of a 32-bit word of the pre-pass (1000 = byte 0, 1101 = byte 1, ...), a whole word and two neighbours in one word
NON_BASE_AT = (0, 15, 16, 17, 127, 128, 129, 16383, 1000, 1101, 1202, 1303, 2000, 2001, 2002, 2003, 2101, 2102)
ALL_MAPPINGS = (4, 2, 1, 41, 42, 43, 44, 21, 22, 23, 11, 12)

Case = namedtuple("Case", "name a b hand")      # hand: dict(score, length, end) worked out by hand, or None


def _random(seed, n=LEN):
    return np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)


def _substituted(a, seed, rate):
    rng = np.random.default_rng(seed)
    b = a.copy()
    at = rng.random(len(a)) < rate
    b[at] = (b[at] + rng.integers(1, 4, int(at.sum()), dtype=np.uint8)) & 3
    return b


def stretch_pair(seed, runs_at):
    """A random identical pair with stretches that match at no offset: seq1 = 0, seq2 = 1 over [lo, lo + run)."""
    a = _random(seed)
    b = a.copy()
    for lo, run in runs_at:
        a[lo: lo + run], b[lo: lo + run] = 0, 1
    return a, b


def _full(score):
    return dict(FULL, score=score)


def _threshold_cases():
    out = []
    for run in STRETCHES:
        a, b = stretch_pair(7000 + run, [(lo, run) for lo in STRETCH_AT])
        # `run` mismatches cost 2 each against the matches they replace; 71 take the diagonal below best - 70 with nothing
        # else alive: the alignment ends where the first stretch begins
        hand = _full(LEN - 2 * run * 3) if run <= XDROP else dict(score=STRETCH_AT[0], length=STRETCH_AT[0] + 1, end=(STRETCH_AT[0],) * 2)
        out.append(Case("stretch%d" % run, a, b, hand))
    # 70 mismatches, one match, one more mismatch: at the threshold, off it, at it again.  (The seed is one at which no
    # path with a gap beside the lone match does better than the diagonal: the hand value below.)
    a, b = stretch_pair(7108, [(lo, XDROP) for lo in STRETCH_AT])
    for lo in STRETCH_AT:
        b[lo + XDROP] = a[lo + XDROP]
        b[lo + XDROP + 1] = (a[lo + XDROP + 1] + 2) & 3
    out.append(Case("stretch70_match_mismatch", a, b, _full(LEN - 2 * (XDROP + 1) * 3)))
    for run in (45, 60):                    # windows whose start margin is exactly 12 and exactly 13 (test_sg_edges_cpu.py)
        a, b = stretch_pair(7200 + run, [(lo, run) for lo in STRETCH_AT])
        out.append(Case("stretch%d" % run, a, b, _full(LEN - 2 * run * 3)))
    # one alignment that sinks to every depth from 40 to 66 below the best value and recovers
    a, b = stretch_pair(7300, [(400 + 500 * (run - 40), run) for run in range(40, 67)])
    out.append(Case("stretch_ramp", a, b, _full(LEN - 2 * sum(range(40, 67)))))
    for run in STRETCHES:                   # the threshold met off the band's centre: seq2 starts 8 bases into seq1
        a = _random(7400 + run)
        b = np.concatenate([a[8:], _random(7450 + run, 8)])
        a[6008: 6008 + run], b[6000: 6000 + run] = 0, 1
        out.append(Case("stretch%d_shifted" % run, a, b, None))
    return out


def _prefix_cases():
    out = [Case("all_mismatch", np.zeros(LEN, np.uint8), np.ones(LEN, np.uint8), dict(score=0, length=1, end=(0, 0)))]
    for n in PREFIXES:
        p = _random(7500 + n, n)
        a = np.concatenate([p, np.zeros(LEN - n, np.uint8)])
        b = np.concatenate([p, np.ones(LEN - n, np.uint8)])
        # L matches need L rows and L columns: (L, L) is the first cell that holds L, and nothing matches behind it
        out.append(Case("prefix%d" % n, a, b, dict(score=n, length=n + 1, end=(n, n))))
        cut = n // 2                            # one base of the prefix missing in seq2: the best cell lies in an odd round
        b = np.concatenate([p[:cut], p[cut + 1:], np.ones(LEN - n + 1, np.uint8)])
        out.append(Case("prefix%d_deleted" % n, a, b, None))
    return out


def _edge_cases():
    out = []
    for s in SHIFTS:
        a = _random(7600 + s)
        out.append(Case("shift_left%d" % s, a, np.concatenate([a[s:], _random(7650 + s, s)]), None))      # seq2 = seq1[s:]
        out.append(Case("shift_right%d" % s, a, np.concatenate([_random(7680 + s, s), a[:LEN - s]]), None))
    a = _random(7700)
    b = a.copy()
    b[LEN - 1] = (a[LEN - 1] + 1) & 3
    out.append(Case("last_base_mismatch", a, b, dict(score=LEN - 1, length=LEN, end=(LEN - 1, LEN - 1))))
    b = a.copy()
    b[0] = (a[0] + 1) & 3
    out.append(Case("first_base_mismatch", a, b, _full(LEN - 2)))
    out.append(Case("identical", a, a.copy(), _full(LEN)))
    # the band rides into the corner of the padded matrix: the state the reference reads past its pads in (touched_oob)
    out.append(Case("acg_acgt", np.resize(np.array([0, 1, 2], np.uint8), LEN), np.resize(np.array([0, 1, 2, 3], np.uint8), LEN), None))
    return out


def _tie_cases():
    zeros = np.zeros(LEN, np.uint8)
    ac = np.resize(np.array([0, 1], np.uint8), LEN)
    out = [Case("all_a", zeros, zeros.copy(), _full(LEN)),
           Case("acac_caca", ac, np.resize(np.array([1, 0], np.uint8), LEN), dict(score=LEN - 2, length=LEN + 1, end=(LEN - 1, LEN)))]
    for unit in ((0, 0, 1), (0, 1, 1, 2, 3)):          # a repeat against itself one period on: every multiple of the period ties
        a = np.resize(np.array(unit, np.uint8), LEN)
        out.append(Case("period%d" % len(unit), a, np.roll(a, -len(unit)), None))
    return out


def _non_base_cases():
    out = []
    for v in NON_BASES:
        for where in ("seq1", "seq2", "both"):
            a = _random(7800 + v)
            b = _substituted(a, 7900 + v, 0.02)
            for at in NON_BASE_AT:
                if where != "seq2":
                    a[at] = v
                if where != "seq1":
                    b[at] = v                       # (the same byte in both: still a mismatch)
            out.append(Case("non_base_%02x_%s" % (v, where), a, b, None))
    a = _random(8000)
    b = a.copy()
    a[32::64] = 4                                   # calm and exact windows in turn, to the end
    out.append(Case("non_base_periodic", a, b, _full(LEN - 2 * (LEN // 64))))
    return out


def _healthy_cases():
    out = []
    for k in range(12):
        a = _random(8100 + k)
        b = _substituted(a, 8200 + k, 0.05)
        if k % 3 == 0:
            cut, sh = 1000 + 1100 * k, (3, -5, 9, -12)[k // 3]
            b[cut:] = np.roll(b, sh)[cut:]
        out.append(Case("healthy%d" % k, a, b, None))
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """The cases, dead alignments (a few rounds long) dealt out among the live ones so that they share every sweep
    wavefront of every mapping (16, 32 or 64 alignments), and a count that fills no wavefront."""
    cases = _threshold_cases() + _prefix_cases() + _edge_cases() + _tie_cases() + _non_base_cases() + _healthy_cases()
    n = len(cases)
    assert n % 16 != 0 and np.gcd(n, 37) == 1
    dealt = tuple(cases[(k * 37) % n] for k in range(n))
    for c in dealt:
        assert c.a.shape == c.b.shape == (LEN,) and c.a.dtype == c.b.dtype == np.uint8
        c.a.setflags(write=False)
        c.b.setflags(write=False)
    assert len({c.name for c in dealt}) == n
    return dealt


def index_of(name):
    return [c.name for c in batch()].index(name)


def arrays():
    """(seq1s[n, 16384], seq2s[n, 16384]) of the batch"""
    return np.stack([c.a for c in batch()]), np.stack([c.b for c in batch()])


# the alignments whose count of calm windows the GPU tests compare with the profile, one per launch
COUNTED = ("stretch45", "stretch60", "stretch70", "stretch_ramp", "shift_left24", "non_base_periodic", "all_mismatch")
CAP_CASES = ("all_mismatch", "prefix8", "identical")      # path lengths 1, 9 and 16385


def caps_for(length):
    return sorted({1, 2, length - 1, length, length + 1})


def move_words(tb, words):
    """The library's move words of a traceback (ascending positions): the steps in walking order (the last one first) as
    3 diagonal / 2 up / 1 left, 32 per 64-bit word."""
    d = np.diff(np.asarray(tb, np.int64), axis=0)[::-1]
    codes = (2 * d[:, 0] + d[:, 1]).astype(np.uint64)
    assert ((d >= 0) & (d <= 1)).all() and (codes > 0).all()
    out = np.zeros(words, np.uint64)
    padded = np.zeros(((len(codes) + 31) // 32) * 32, np.uint64)
    padded[: len(codes)] = codes
    out[: len(padded) // 32] = (padded.reshape(-1, 32) << (2 * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
    return out


def same_moves(got, want, length):
    """move words up to the last step (bits past it are unspecified)"""
    full, part = divmod(int(length) - 1, 32)
    if not np.array_equal(got[:full], want[:full]):
        return False
    mask = np.uint64((1 << (2 * part)) - 1)
    return part == 0 or (got[full] & mask) == (want[full] & mask)


def band_cells(tb, top_y):
    """the band cell of every path step: 31 - (y - top_y[y + x])"""
    tb = np.asarray(tb, np.int64)
    return 31 - (tb[:, 0] - top_y[tb[:, 0] + tb[:, 1]])


Profile = namedtuple("Profile", "windows rounds at_threshold best_round score touched_oob by_rule lowest margin score_at dropped "
                                "dropped_live reach top_y")


class SgProfile:
    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libsg_xdrop_profile.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-Wall", "-o", so,
                               os.path.join(ROOT, "tests", "native", "sg_xdrop_profile.c")])
        self.lib = ctypes.CDLL(so)
        self.max_windows = self.lib.sg_xdrop_profile_windows()
        self.max_rounds = self.lib.sg_xdrop_profile_rounds()

    def profile(self, a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        assert a.shape == b.shape == (LEN,)
        margin = np.zeros(self.max_windows, np.int32)
        score_at = np.zeros(self.max_windows, np.int32)
        dropped = np.zeros(self.max_windows, np.int32)
        live = np.zeros(self.max_windows, np.int32)
        reach = np.zeros(self.max_windows, np.uint8)
        top_y = np.zeros(self.max_rounds, np.int32)
        out = (ctypes.c_long * 8)()
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        assert self.lib.sg_xdrop_profile(P(a), P(b), P(margin), P(score_at), P(dropped), P(live), P(reach), P(top_y), out) == 0
        w, r = int(out[0]), int(out[1])
        return Profile(w, r, int(out[2]), int(out[3]), int(out[4]), int(out[5]), int(out[6]), int(out[7]), margin[:w], score_at[:w], dropped[:w],
                       live[:w], reach[:w].astype(bool), top_y[: r + 1].astype(np.int64))

    @staticmethod
    def calm(p, margin):
        """calm windows of the restatement's predicate: no cell dropped, the lowest at least `margin` above best - 70"""
        return int((p.margin >= margin).sum())


def kernel_predicate(p, margin):
    """calm windows of the predicate as sg_kernels.hip states it: the lowest cell at least `margin` above max(best - 70, 1)
    -- one higher than the restatement's threshold while the score is 0 -- and no pad or non-base in reach"""
    return int(((p.margin - (p.score_at == 0) >= margin) & ~p.reach).sum())
