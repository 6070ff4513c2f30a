"""The mixed-shape banded aligners on the GPU (libswmi_banded_ragged.so, include/swmi_banded_ragged.h).
Every comparison is against the two existing C restatements, called once per alignment with that alignment's lengths and
diagonal (banded_ragged_support.RaggedOracle), unconditionally: score, the four ends, steps, and the moves word for word up to
steps.  Every test runs all four kernels of a kind -- with a traceback and ends-only, gap_open >= gap_extend and gap_open <
gap_extend -- and every test of the global kind runs the masks 0 .. 19 (the matrix test spreads them over its matrices).  The
shapes are the smallest that hold the traps of sections 33 and 34 in a MIXED batch: lane 0's left neighbour, trips that end at
every remainder, move-word seams, bands that miss the table, empty sequences, one workgroup whose four wavefronts run very
different trip counts."""
import os
import subprocess

import numpy as np
import pytest
import torch

from banded_ragged_support import (ALL_MASKS, FORMS, GLOBAL, INT32_MAX, INT32_MIN, LOCAL, MAX_SLICE, NO_ALIGNMENT, Batch, RaggedOracle,
                                   assert_same, move_words, moves_of, path_from, permuted, related_batch, related_pairs)
from conftest import PKG, ROOT, match_matrix

pytestmark = pytest.mark.gpu

GUARD = 16                                  # guard words behind every output array
PATTERN = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return RaggedOracle(tmp_path_factory.mktemp("banded_ragged_oracle"))


@pytest.fixture(scope="module")
def br(swmi_mod):
    swmi_mod.banded_ragged.load()
    return swmi_mod.banded_ragged


def _dev_bytes(cat):
    """a side's bytes on the device; a side that is empty throughout passes a buffer the library never reads"""
    host = np.ascontiguousarray(cat) if len(cat) else np.full(16, 255, np.uint8)
    return torch.from_numpy(host).to("cuda:0")


class DeviceCall:
    """One device call on fresh tensors with GUARD words behind every output array and the moves pre-filled with PATTERN;
    result() waits and returns numpy arrays in the host entry's layout after checking the guards."""

    def __init__(self, br, kind, batch, sm, go, ge, mask=0, traceback=True, stream=0):
        n, words = batch.n, int(batch.move_offsets[-1])
        self.batch, self.traceback = batch, traceback
        self.keep = (_dev_bytes(batch.cat1), _dev_bytes(batch.cat2))
        self.scores = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.ends = torch.full((4 * n + GUARD,), -7, dtype=torch.int32, device="cuda:0")
        self.moves = torch.full((words + GUARD,), PATTERN, dtype=torch.int64, device="cuda:0") if traceback else None
        self.steps = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda:0") if traceback else None
        args = (self.keep[0], batch.off1, self.keep[1], batch.off2, sm, go, ge)
        tail = (self.scores, self.ends, self.moves, self.steps, batch.diagonals, stream)
        if kind == GLOBAL:
            br.global_device(*args, mask, *tail)
        else:
            br.local_device(*args, *tail)

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


def both_ways(br, orc, kind, batch, sm, go, ge, mask, what):
    """with a traceback and ends-only against the restatements; returns the traceback result"""
    want = orc.align(kind, batch, sm, go, ge, mask)
    got = DeviceCall(br, kind, batch, sm, go, ge, mask).result()
    assert_same(got, want, batch, what)
    eo = DeviceCall(br, kind, batch, sm, go, ge, mask, traceback=False).result()
    assert_same(eo, want, batch, (what, "ends-only"), traceback=False)         # (the same scores and end cells; starts (-1, -1))
    return got


def kinds_and_masks():
    return [(LOCAL, 0)] + [(GLOBAL, m) for m in ALL_MASKS]


def hand_built(rng):
    """test 1's batch; n = 30 is not a multiple of 4"""
    parts = [related_batch(rng, [(63, 127)], [64]),                              # section 33's lane-0 trap
             related_batch(rng, [(1, 1)], [0])]
    e = np.zeros(0, np.uint8)
    five = rng.integers(0, 4, 5, dtype=np.uint8)
    for d in (0, 64, -65, 70):                                                   # (0, 0) in the band (0, 64) and not (-65, 70)
        parts.append(Batch([e, five, e], [five, e, e], [d, d, d]))
    parts.append(related_batch(rng, [(300, 280), (280, 300)], [0, 0]))
    parts.append(related_batch(rng, [(65, 70), (66, 71), (67, 69), (68, 70)], [0, 3, -3, 1]))     # len1 + 63 and len1 + 64: every remainder mod 4
    same = [rng.integers(0, 4, L, dtype=np.uint8) for L in (32, 33, 64, 65)]     # all-match pairs: move-word seams
    parts.append(Batch(same, same, [0, 0, 0, 0]))
    a, b = related_pairs(rng, 4, 50, 60)
    parts.append(Batch(list(a), list(b), [20000, -20000, INT32_MIN, INT32_MAX]))                  # bands that miss the table
    long1, one = related_pairs(rng, 1, 16384, 1)
    parts.append(Batch([long1[0], one[0]], [one[0], long1[0]], [0, 0]))          # 65 swept rows beside a long sequence
    batch = parts[0]
    for p in parts[1:]:
        batch = batch + p
    return batch


def test_one_mixed_batch_of_hand_built_shapes_in_caller_order_and_reversed(br, orc):
    rng = np.random.default_rng(1)
    batch = hand_built(rng)
    assert batch.n == 30 and batch.n % 4 != 0
    back = batch.reversed()
    order = list(range(batch.n))[::-1]
    sm = match_matrix(2, -3)
    seams = set()
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            got = both_ways(br, orc, kind, batch, sm, go, ge, mask, (kind, mask, go, ge))
            rev = DeviceCall(br, kind, back, sm, go, ge, mask).result()
            assert_same(permuted(rev, batch, order), got, batch, ("reversed", kind, mask, go, ge))
            rev_eo = DeviceCall(br, kind, back, sm, go, ge, mask, traceback=False).result()
            assert_same(permuted(rev_eo, batch, order), got, batch, ("reversed, ends-only", kind, mask, go, ge), traceback=False)
            if kind == LOCAL or mask == 0:
                seams |= {int(got[3][k]) for k in range(20, 24)}
            if kind == LOCAL:
                assert not got[0][24:28].any() and not got[3][24:28].any()       # the band misses the table
            else:
                assert (got[0][24:28] == NO_ALIGNMENT).all()
    assert seams == {32, 33, 64, 65}


def test_workgroups_whose_four_wavefronts_run_different_trip_counts(br, orc):
    rng = np.random.default_rng(2)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 701, 64), rng.integers(1, 701, 64))]
    shapes[:4] = [(700, 690), (1, 1), (650, 700), (3, 500)]                      # caller neighbours: long, tiny, long, thin
    batch = related_batch(rng, shapes, [(0, 40, -37)[k % 3] for k in range(64)])
    longest = 0
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            got = both_ways(br, orc, kind, batch, match_matrix(2, -3), go, ge, mask, (kind, mask, go, ge))
            longest = max(longest, int(got[3].max()))
    assert longest > 3 * 64                                                      # a path crosses the 64-iteration window at least twice


def test_equal_shapes_equal_the_fixed_entries(br, swmi_mod):
    """37 alignments of (300, 270) with diagonals: the ragged call and the fixed device entries give the same fields and moves."""
    rng = np.random.default_rng(3)
    a, b = related_pairs(rng, 37, 300, 270)
    b[1::3] = rng.integers(0, 4, (len(b[1::3]), 270), dtype=np.uint8)
    d = rng.integers(-70, 70, 37).astype(np.int32)
    batch = Batch(list(a), list(b), d)
    mw = move_words(300, 270)
    dev = torch.device("cuda:0")
    ta, tb_, td = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(d).to(dev)
    sm = match_matrix(2, -3)
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            for traceback in (True, False):
                scores = torch.full((37,), -7, dtype=torch.int32, device=dev)
                ends = torch.full((37, 4), -7, dtype=torch.int32, device=dev)
                moves = torch.zeros((37, mw), dtype=torch.int64, device=dev) if traceback else None
                steps = torch.full((37,), -7, dtype=torch.int32, device=dev) if traceback else None
                if kind == GLOBAL:
                    swmi_mod.banded_global.align_device(ta, tb_, sm, go, ge, scores, ends, moves, steps, free_ends=mask, diagonals=td)
                else:
                    swmi_mod.banded.local_device(ta, tb_, sm, go, ge, scores, ends, moves, steps, diagonals=td)
                torch.cuda.synchronize()
                want = (scores.cpu().numpy(), ends.cpu().numpy(), moves.cpu().numpy().view(np.uint64).reshape(-1) if traceback else None,
                        steps.cpu().numpy().view(np.uint32) if traceback else None)
                got = DeviceCall(br, kind, batch, sm, go, ge, mask, traceback=traceback).result()
                assert_same(got, want, batch, (kind, mask, go, ge, traceback), traceback=traceback)
                assert np.array_equal(got[1], want[1])                           # every field, ends-only too
                assert (want[0] != 0).any()


def test_negative_bests_and_ties_across_lanes_in_a_mixed_batch(br, orc):
    """Two-letter and periodic sequences, three shapes in one call: several candidates hold the maximum, on different lanes;
    with a matrix that is negative everywhere the ties are among negative values."""
    rng = np.random.default_rng(4)
    s1, s2 = [], []
    for len1, len2 in ((96, 96), (150, 131), (131, 150)):
        s1 += [np.arange(len1) % 2, np.arange(len1) % 3, np.arange(len1) % 4, (np.arange(len1) // 5) % 2, rng.integers(0, 2, len1),
               np.tile([0, 0, 1], len1)[:len1]]
        s2 += [np.arange(len2) % 2, np.arange(len2) % 3, np.arange(len2) % 4, (np.arange(len2) // 5) % 2, rng.integers(0, 2, len2),
               np.tile([0, 1, 1], len2)[:len2]]
    order = rng.permutation(18)                                                  # the three shapes interleaved
    s1, s2 = [s1[k] for k in order], [s2[k] for k in order]
    negative = 0
    for sm, go, ge in ((match_matrix(1, -1), 1, 1), (match_matrix(-1, -2), 3, 1), (match_matrix(-2, -2), 1, 2), (match_matrix(1, 0), 0, 0),
                       (match_matrix(-1, -1), 127, 127)):
        for d in (None, np.tile([3, -3, 10, -10, 0, 1], 3).astype(np.int32)):
            batch = Batch(s1, s2, d)
            for mask in ALL_MASKS:
                got = both_ways(br, orc, GLOBAL, batch, sm, go, ge, mask, (list(sm), go, ge, mask))
                negative += int(((got[0] < 0) & (got[0] != NO_ALIGNMENT)).sum())
    assert negative > 100


def test_random_extreme_and_asymmetric_matrices_on_48_mixed_shapes(br, orc):
    rng = np.random.default_rng(5)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 201, 48), rng.integers(1, 201, 48))]
    shapes[0], shapes[1] = (200, 200), (200, 1)
    batch = related_batch(rng, shapes, rng.integers(-70, 70, 48))
    for k in range(1, 48, 2):
        batch.seq2s[k][:] = rng.integers(0, 4, len(batch.seq2s[k]), dtype=np.uint8)
    batch = Batch(batch.seq1s, batch.seq2s, batch.diagonals)
    mats = [rng.integers(-128, 128, 16).astype(np.int8) for _ in range(3)]
    mats += [np.full(16, 127, np.int8), np.full(16, -128, np.int8), match_matrix(127, -128), np.arange(-8, 8, dtype=np.int8),
             (np.arange(16, dtype=np.int8) * 7 % 23 - 11).astype(np.int8)]
    covered = set()
    turn = 0
    for sm in mats:
        for go, ge in ((0, 0), (127, 127), (127, 0), (0, 127), (7, 2), (2, 7)):
            both_ways(br, orc, LOCAL, batch, sm, go, ge, 0, ("local", list(sm), go, ge))
            for mask in [(turn * 5 + x) % 20 for x in range(5)]:                 # five masks a turn, every mask under twelve (matrix, gaps)
                both_ways(br, orc, GLOBAL, batch, sm, go, ge, mask, (list(sm), go, ge, mask))
                covered.add(mask)
            turn += 1
    assert covered == set(ALL_MASKS)
    # junk in bits 2 - 7 of the bases
    junk = Batch([x | 0xA4 for x in batch.seq1s], [x | 0x58 for x in batch.seq2s], batch.diagonals)
    both_ways(br, orc, LOCAL, junk, mats[0], 4, 1, 0, "junk bits")
    both_ways(br, orc, GLOBAL, junk, mats[0], 4, 1, 15, "junk bits")


def test_output_guards_and_no_move_word_outside_an_alignments_own_row(br, orc):
    """DeviceCall checks the guard words behind scores, ends, steps and moves.  Here also: in a moves buffer pre-filled with a
    pattern the row of a zero-length alignment keeps the pattern (it writes no move word), and so does the row of an alignment
    missed by its band; an empty sequence of the global kind whose border is not free has its forced steps, which the
    comparison with the oracle covers."""
    rng = np.random.default_rng(6)
    e = np.zeros(0, np.uint8)
    shapes = [(70, 90), (5, 0), (200, 180), (0, 7), (33, 33), (0, 0), (64, 64), (40, 50), (129, 127)]
    batch = related_batch(rng, [(max(x, 1), max(y, 1)) for x, y in shapes], [0, 0, 5, 0, 0, 0, -3, 30000, 1])
    s1 = [e if shapes[k][0] == 0 else batch.seq1s[k] for k in range(9)]
    s2 = [e if shapes[k][1] == 0 else batch.seq2s[k] for k in range(9)]
    batch = Batch(s1, s2, batch.diagonals)
    assert batch.shapes() == shapes
    for go, ge in FORMS:
        for kind, mask in kinds_and_masks():
            call = DeviceCall(br, kind, batch, match_matrix(2, -3), go, ge, mask)
            got = call.result()
            assert_same(got, orc.align(kind, batch, match_matrix(2, -3), go, ge, mask), batch, (kind, mask, go, ge))
            for k in range(9):
                row = got[2][int(batch.move_offsets[k]):int(batch.move_offsets[k + 1])]
                if got[3][k] == 0 and (0 in shapes[k] or k == 7):            # a closed form: no step, so no move word
                    assert (row == np.uint64(PATTERN)).all(), (kind, mask, k)
                if kind == LOCAL and 0 in shapes[k]:
                    assert got[3][k] == 0 and got[0][k] == 0
            DeviceCall(br, kind, batch, match_matrix(2, -3), go, ge, mask, traceback=False).result()     # (the guards, ends-only)


def _tiled(base, n):
    """(cat1, off1, cat2, off2, diagonals) of n alignments: base's alignments again and again, without a python list of n"""
    reps = -(-n // base.n)
    len1 = np.tile(np.diff(base.off1.astype(np.int64)), reps)[:n]
    len2 = np.tile(np.diff(base.off2.astype(np.int64)), reps)[:n]
    off1 = np.concatenate([[0], np.cumsum(len1)]).astype(np.uint64)
    off2 = np.concatenate([[0], np.cumsum(len2)]).astype(np.uint64)
    cat1, cat2 = np.tile(base.cat1, reps)[:int(off1[-1])], np.tile(base.cat2, reps)[:int(off2[-1])]
    return cat1, off1, cat2, off2, np.tile(base.diagonals, reps)[:n]


def test_the_host_entries_in_two_slices(br, orc):
    """Ends-only the count cap binds on tiny mixed shapes; with a traceback the byte budget does on (16384, 1)-shaped
    alignments, with three more of them and a handful of mixed ones behind, so that the second slice is mixed.  The batches repeat a few distinct
    alignments, and the oracle runs once per distinct alignment."""
    rng = np.random.default_rng(7)
    sm = match_matrix(2, -1)
    shapes = [(int(x), int(y)) for x, y in zip(rng.integers(1, 4, 101), rng.integers(1, 4, 101))]
    base = Batch([rng.integers(0, 4, x, dtype=np.uint8) for x, _ in shapes], [rng.integers(0, 4, y, dtype=np.uint8) for _, y in shapes],
                 rng.integers(-2, 3, 101))
    n = MAX_SLICE + 5
    cat1, off1, cat2, off2, d = _tiled(base, n)
    assert br.slices_for(LOCAL, off1, off2, traceback=False) == br.slices_for(GLOBAL, off1, off2, traceback=False) == [MAX_SLICE, 5]
    reps = -(-n // 101)
    for (go, ge), (kind, mask) in zip(FORMS + FORMS, [(LOCAL, 0), (GLOBAL, 0), (GLOBAL, 19), (LOCAL, 0)]):
        want = orc.align(kind, base, sm, go, ge, mask, traceback=False)
        if kind == GLOBAL:
            got = br.global_((cat1, off1), (cat2, off2), sm, go, ge, free_ends=mask, diagonals=d, traceback=False)
        else:
            got = br.local((cat1, off1), (cat2, off2), sm, go, ge, diagonals=d, traceback=False)
        assert got[2] is None and got[3] is None and got[4] is None
        assert np.array_equal(got[0], np.tile(want[0], reps)[:n]) and np.array_equal(got[1], np.tile(want[1], (reps, 1))[:n]), (kind, mask, go, ge)
    # with a traceback
    a, b = related_pairs(rng, 3, 16384, 1)
    tall = Batch(list(a), list(b), [0, -40, -16300])
    probe = np.arange(8193, dtype=np.uint64)
    for kind, mask in ((LOCAL, 0), (GLOBAL, 7)):                                 # BEGIN1 | BEGIN2 | END1: a start and an end in every band
        per = br.slices_for(kind, 16384 * probe, probe)[0]
        assert 4000 < per < 4200
        tail = related_batch(rng, [(700, 650), (1, 16384), (0, 9), (300, 2), (64, 64)], [0, 0, 0, -100, 0])
        count = per + 3                                                          # the second slice: three more of them, then the mixed ones
        cat1, off1, cat2, off2, d = _tiled(tall, count)
        cat1, cat2 = np.concatenate([cat1, tail.cat1]), np.concatenate([cat2, tail.cat2])
        off1 = np.concatenate([off1, off1[-1] + tail.off1[1:]])
        off2 = np.concatenate([off2, off2[-1] + tail.off2[1:]])
        d = np.concatenate([d, tail.diagonals]).astype(np.int32)
        assert br.slices_for(kind, off1, off2) == [per, 8]
        reps = -(-count // 3)
        for go, ge in FORMS:
            w_tall, w_tail = orc.align(kind, tall, sm, go, ge, mask), orc.align(kind, tail, sm, go, ge, mask)
            if kind == GLOBAL:
                sc, ends, moves, mo, steps = br.global_((cat1, off1), (cat2, off2), sm, go, ge, free_ends=mask, diagonals=d)
            else:
                sc, ends, moves, mo, steps = br.local((cat1, off1), (cat2, off2), sm, go, ge, diagonals=d)
            assert np.array_equal(sc, np.concatenate([np.tile(w_tall[0], reps)[:count], w_tail[0]])), (kind, go, ge)
            assert np.array_equal(ends, np.concatenate([np.tile(w_tall[1], (reps, 1))[:count], w_tail[1]])), (kind, go, ge)
            assert np.array_equal(steps, np.concatenate([np.tile(w_tall[3], reps)[:count], w_tail[3]])), (kind, go, ge)
            mw = move_words(16384, 1)
            rows = moves[:count * mw].reshape(count, mw)
            for x in range(3):                                                   # every copy of a distinct alignment: its moves, word for word
                full, part = divmod(int(w_tall[3][x]), 32)
                mine, theirs = rows[x::3], w_tall[2][x * mw:(x + 1) * mw]
                assert (mine[:, :full] == theirs[:full]).all(), (kind, go, ge, x)
                if part:
                    m = np.uint64((1 << (2 * part)) - 1)
                    assert ((mine[:, full] & m) == (theirs[full] & m)).all(), (kind, go, ge, x)
            got_tail = (sc[count:], ends[count:], moves[int(mo[count]):], steps[count:])
            assert_same(got_tail, w_tail, tail, (kind, go, ge, "the mixed second slice"))
            assert w_tail[3].max() > 64
    br.release_workspaces()


def test_back_to_back_device_calls_and_the_module(br, orc):
    rng = np.random.default_rng(8)
    sm = match_matrix(2, -3)
    first = related_batch(rng, [(400, 380), (20, 30), (0, 4), (129, 140), (77, 60)], [0, 5, 0, -20, 64])
    second = related_batch(rng, [(10, 600), (350, 350), (63, 127), (1, 1), (500, 90), (90, 500), (200, 210)], [30, 0, 64, 0, -300, 300, 2])
    for go, ge in FORMS:
        for kind, mask in ((LOCAL, 0), (GLOBAL, 0), (GLOBAL, 10), (GLOBAL, 19)):
            for traceback in (True, False):
                one = DeviceCall(br, kind, first, sm, go, ge, mask, traceback=traceback)          # two calls on one stream, no wait between them
                two = DeviceCall(br, kind, second, sm, go, ge, mask, traceback=traceback)
                assert_same(one.result(), orc.align(kind, first, sm, go, ge, mask), first, ("first", kind, mask), traceback=traceback)
                assert_same(two.result(), orc.align(kind, second, sm, go, ge, mask), second, ("second", kind, mask), traceback=traceback)
    # the module with lists and with (concatenated, offsets), and the paths
    for kind, mask in ((LOCAL, 0), (GLOBAL, 5)):
        want = orc.align(kind, second, sm, 5, 1, mask)
        call = (lambda s1, s2, **kw: br.global_(s1, s2, sm, 5, 1, free_ends=mask, diagonals=second.diagonals, **kw)) if kind == GLOBAL else \
            (lambda s1, s2, **kw: br.local(s1, s2, sm, 5, 1, diagonals=second.diagonals, **kw))
        for s1, s2 in ((second.seq1s, second.seq2s), ((second.cat1, second.off1), (second.cat2, second.off2))):
            sc, ends, moves, mo, steps = call(s1, s2)
            assert np.array_equal(mo, second.move_offsets) and np.array_equal(mo, br.move_offsets(second.off1, second.off2))
            assert_same((sc, ends, moves, steps), want, second, ("module", kind))
            paths = br.paths((sc, ends, moves, mo, steps))
            for k in range(second.n):
                if sc[k] == NO_ALIGNMENT:
                    assert paths[k] is None
                else:
                    assert np.array_equal(paths[k], path_from(want[2][int(mo[k]):], want[3][k], want[1][k, 0], want[1][k, 1])), k
            eo = call(s1, s2, traceback=False)
            assert eo[2] is None and eo[3] is None and eo[4] is None
            assert_same((eo[0], eo[1], None, None), want, second, ("module, ends-only", kind), traceback=False)
    far = Batch(second.seq1s[:2], second.seq2s[:2], [INT32_MAX, 0])
    res = br.global_(far.seq1s, far.seq2s, sm, 5, 1, diagonals=far.diagonals)
    assert res[0][0] == NO_ALIGNMENT and br.paths(res)[0] is None and br.paths(res)[1] is not None
    br.release_workspaces()
    res = br.local(second.seq1s, second.seq2s, sm, 5, 1, diagonals=second.diagonals)
    assert_same((res[0], res[1], res[2], res[4]), orc.align(LOCAL, second, sm, 5, 1), second, "after release")


@pytest.mark.parametrize("kind,mask", [(LOCAL, 0), (GLOBAL, 10)], ids=["local", "global"])
def test_the_cpp_overloads(br, orc, tmp_path, kind, mask):
    exe = str(tmp_path / "compat_banded_ragged")
    lib = os.path.join(PKG, "lib")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "compat_banded_ragged.cpp"), "-o", exe, "-L", lib, "-lswmi_banded_ragged", "-lswmi",
                            "-lpthread", "-Wl,-rpath," + lib], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    rng = np.random.default_rng(12)
    batch = related_batch(rng, [(210, 190), (30, 300), (1, 1), (190, 210), (64, 70), (50, 50), (9, 1)], [0, 10, 0, 64, -3, 300, 0])
    batch = Batch(batch.seq1s[:6] + [batch.seq1s[6]], batch.seq2s[:6] + [np.zeros(0, np.uint8)], batch.diagonals)
    for name, arr in (("a", batch.cat1), ("b", batch.cat2), ("o1", batch.off1), ("o2", batch.off2), ("d", batch.diagonals)):
        arr.tofile(str(tmp_path / (name + ".bin")))
    for go, ge in FORMS:
        out = subprocess.run([exe, str(tmp_path), str(batch.n), str(kind), "2", "-3", str(go), str(ge), str(mask)], stdout=subprocess.PIPE, text=True,
                             check=True, timeout=120).stdout
        want = orc.align(kind, batch, match_matrix(2, -3), go, ge, mask)
        lines = out.strip().splitlines()
        assert len(lines) == batch.n
        for k, line in enumerate(lines):
            f = [int(x) for x in line.split()]
            path = path_from(want[2][int(batch.move_offsets[k]):], want[3][k], want[1][k, 0], want[1][k, 1])
            assert f[0] == want[0][k] and f[1:5] == list(want[1][k]) and f[5] == len(path), k
            assert f[6:] == [int(x) for x in path.reshape(-1)], k
        assert moves_of(want[2], want[3][0]).size > 100
        assert want[0][5] == (NO_ALIGNMENT if kind == GLOBAL else 0)
