"""What test_gpu_pk_edges.py stands on, proved without a device: the table of pk_edges.py reaches every instantiation of
sw128_pk_kernel<MODE, VARIANT, L> through the library's own dispatch rule, on both sides of each of its inequalities; the
structured batch reaches the largest and the smallest score under every set; the oracle the GPU tests compare with agrees
with a numpy restatement of the recurrence that keeps every H matrix; and the values each cell body holds while it walks
those matrices stay finite half-precision patterns with row bytes in 0..255 -- the figures of DESIGN.md 5.1."""
import numpy as np
import pytest

import pk_edges as pe

# Largest value a 16-bit half holds, per body and rows per lane, over the table and the batch of pk_edges.py:
#   q0    (127/-127, 127): H(127,127) + 127 + 127 = 16 129 + 254
#   bias  any 127/-128 set: H(127,127) + (s - min s) = 16 129 + 255 = (H + gap) + Q at the last cell
#   vert  (127/-128, 64): H(127,127) + gap (R - 1) + s + 2 gap = 16 129 + 64 (R - 1) + 255
HELD_MAX = {"q0": {32: 16383, 16: 16383, 8: 16383}, "bias": {32: 16384, 16: 16384, 8: 16384}, "vert": {32: 18368, 16: 17344, 8: 16832}}

_REF = {}


def reference(k):
    """(H, S, scores) of the numpy restatement for the built batch under PARAM_SETS[k]; computed once, never changed"""
    if k not in _REF:
        p = pe.PARAM_SETS[k]
        a, b, _ = batch()
        H, S = pe.numpy_sw(a, b, p.sm, p.gap)
        H.setflags(write=False)
        _REF.clear()                                # one set's matrices at a time: 26 MB each
        _REF[k] = (H, S, H.max(axis=(0, 1)))
    return _REF[k]


_BATCH = []
_HELD = {}


def batch():
    if not _BATCH:
        _BATCH.append(pe.build_batch())
    return _BATCH[0]


def held(k):
    """{rows per lane: (smallest, largest) value a half holds} for PARAM_SETS[k] on the built batch; computed once per set,
    whichever test asks first (only the vertical-offset form depends on the rows per lane)"""
    if k not in _HELD:
        p = pe.PARAM_SETS[k]
        H, S, _ = reference(k)
        one = None if p.variant == "vert" else pe.held_values(H, S, p.sm, p.gap, p.variant, 32)
        _HELD[k] = {r: one or pe.held_values(H, S, p.sm, p.gap, p.variant, r) for r in (32, 16, 8)}
    return _HELD[k]


SET_IDS = [p.label for p in pe.PARAM_SETS]


def test_the_table_holds_what_it_claims():
    sets = pe.PARAM_SETS
    assert len({p.label for p in sets}) == len(sets)
    for p in sets:
        assert p.sm.dtype == np.int8 and p.sm.shape == (16,) and 0 <= p.gap <= 127
        assert pe.expected_variant(p.sm, p.gap) == p.variant, p.label
        rb = pe.row_bytes(p.sm, p.gap, p.variant)
        assert rb.min() >= 0 and rb.max() <= 255, (p.label, rb)
    lo = lambda p: int(p.sm.min())
    hi = lambda p: int(p.sm.max())
    # both sides of every inequality of the rule, at distance one where the rule allows it
    assert {lo(p) + p.gap for p in sets} >= {0, -1}
    assert {lo(p) + 2 * p.gap for p in sets if lo(p) + p.gap < 0} >= {0, -1}
    assert {hi(p) + 2 * p.gap for p in sets if lo(p) + p.gap < 0 <= lo(p) + 2 * p.gap} >= {255, 256, 257}
    for variant in pe.VARIANTS:
        mine = pe.sets_of(variant)
        asym = [p for p in mine if all(p.sm[4 * a + b] != p.sm[4 * b + a] for a in range(4) for b in range(a))]
        assert len(asym) >= 2, variant
        bytes_seen = set(np.concatenate([pe.row_bytes(p.sm, p.gap, variant) for p in asym]).tolist())
        assert 0 in bytes_seen and (255 in bytes_seen or variant == "q0" and 254 in bytes_seen), variant    # s + gap <= 127 + 127
    vert = {(int(p.sm[0]), int(p.sm[1]), p.gap) for p in pe.sets_of("vert")}
    assert (127, -128, 64) in vert
    bias = {(int(p.sm[0]), int(p.sm[1]), p.gap) for p in pe.sets_of("bias")}
    assert {(127, -128, 63), (127, -128, 65), (127, -128, 127), (127, -128, 0)} <= bias


def test_dispatch_sends_every_set_to_its_body(swmi_mod):
    """swmi_score_kernel_for_batch (no device needed) for every set, mode and forced L: the instantiation is the one the
    table claims, and each of the 27 is named by at least three sets."""
    named = {}
    try:
        for lanes in pe.LANES:
            swmi_mod.set_schedule(lanes, 0)
            for mode in pe.MODES.values():
                for p in pe.PARAM_SETS:
                    got, per_wave = swmi_mod.score_kernel_for_batch(442, p.sm, p.gap, mode)
                    assert got == pe.expected_name(mode, p.variant, lanes), (p.label, mode, lanes, got)
                    assert per_wave == 128 // lanes
                    named[got] = named.get(got, 0) + 1
    finally:
        swmi_mod.set_schedule(0, 0)
    assert len(named) == 27 and min(named.values()) >= 3, named


def test_the_batch_holds_what_it_claims():
    a, b, labels = batch()
    assert len(a) == 197 and a.shape == b.shape == (197, 128) and a.max() <= 3 and b.max() <= 3
    pairs = {(tuple(x), tuple(y)) for x, y in zip(a, b)}
    for x in range(4):
        for y in range(4):
            assert (tuple(pe.homopolymer(x)), tuple(pe.homopolymer(y))) in pairs
    assert sum(l.startswith("single match") for l in labels) == len(pe.LANE_EDGE_ROWS) * len(pe.SINGLE_COLUMNS)
    for r in (8, 16, 32):                   # the first and the last row of a lane, for every rows-per-lane
        assert {1, r, r + 1, 128} <= set(pe.LANE_EDGE_ROWS), r
    # placement: every built pair sits in each half of a register once, each time beside a different partner
    pa, pb, origin = pe.place(a, b)
    assert len(pa) % 2 == 0 and len(pa) == 2 * 197 + 48
    for k in range(len(a)):
        at = np.nonzero(origin == k)[0]
        assert sorted(at % 2) == [0, 1], k
        partners = [int(origin[i ^ 1]) for i in at]
        assert partners[0] != partners[1] and k not in partners, (k, partners)
        assert all(np.array_equal(pa[i], a[k]) and np.array_equal(pb[i], b[k]) for i in at)
    # one-vs-many: one seq2 per batch; together the batches hold all 16 homopolymer pairs and every single-match cell
    ovm = pe.ovm_batches()
    _, s1, shared = ovm[0]
    ovm_labels = pe.build_batch(shared)[2]
    assert ovm_labels == labels
    at = {l: i for i, l in enumerate(ovm_labels)}
    assert [ovm_labels[i] for i in np.nonzero((s1 == shared).all(axis=1))[0]] == ["self"]       # exactly one self-pair
    for pos in pe.RUN_POSITIONS:            # both directions of every gap run, around the one seq2
        for k in pe.RUN_LENGTHS:
            more, fewer = s1[at["run of %d deleted at %d" % (k, pos)]], s1[at["run of %d inserted at %d" % (k, pos)]]
            end = 128 - k                   # seq1 with k rows more than seq2 (vertical run), with k rows fewer (horizontal run)
            assert np.array_equal(more[:pos], shared[:pos]) and np.array_equal(more[pos + k:], shared[pos:end]), (pos, k)
            assert np.array_equal(fewer[:pos], shared[:pos]) and np.array_equal(fewer[pos:end], shared[pos + k:]), (pos, k)
    for r in pe.ROTATIONS:
        assert np.array_equal(s1[at["rotated by %d" % r]], np.roll(shared, -r)) and np.array_equal(s1[at["rotated by -%d" % r]], np.roll(shared, r))
    # ... and the gap run is what the alignment takes: with match 10, mismatch -30, gap 1 the score is that of the copy with
    # one run of k gaps or better, in either direction; the same structure holds in the pairs batch
    sm10 = pe.match_matrix(10, -30)         # more than either side of the run scores alone
    for s1x, s2x, where in ((s1, np.broadcast_to(shared, s1.shape).copy(), "one-vs-many"), (a, b, "pairs")):
        runs = [i for i, l in enumerate(labels) if l.startswith("run of")]
        H, _ = pe.numpy_sw(s1x[runs], s2x[runs], sm10, 1)
        crossed = set()
        for score, i in zip(H.max(axis=(0, 1)), runs):
            k, direction, pos = int(labels[i].split()[2]), labels[i].split()[3], int(labels[i].split()[-1])
            before, after = pos, max(0, 128 - pos - k)
            assert score >= max(10 * before, 10 * after, 10 * (before + after) - k), (where, labels[i], score)
            if 10 * min(before, after) > k:                     # crossing the run pays: the bound above is the crossing one
                crossed.add((k, pos, direction))
        for direction in ("deleted", "inserted"):               # every length and every position, in both directions
            assert {k for k, _, d in crossed if d == direction} == set(pe.RUN_LENGTHS), (where, direction)
            assert {p for _, p, d in crossed if d == direction} == set(pe.RUN_POSITIONS), (where, direction)
    seen = set()
    for label, s1, s2 in ovm:
        assert s1.shape == (197, 128) and s2.shape == (128,), label
        seen |= {(tuple(x), tuple(s2)) for x in s1}
    for x in range(4):
        for y in range(4):
            assert (tuple(pe.homopolymer(x)), tuple(pe.homopolymer(y))) in seen
    for i in pe.LANE_EDGE_ROWS:
        for j in pe.SINGLE_COLUMNS:
            assert (tuple(pe.single_row(i)), tuple(pe.single_column(j))) in seen
    junk = pe.with_junk(a)
    assert np.array_equal(junk & 3, a) and (junk >> 2).max() == 63 and len(np.unique(junk >> 2)) == 64
    assert pe.tail_sizes(4, 442) == [1, 2, 31, 33, 129, 441]


@pytest.mark.parametrize("k", range(len(pe.PARAM_SETS)), ids=SET_IDS)
def test_oracle_batch_and_range_under_every_set(oracle, k):
    """Per set, on the reference's H matrices (never on the library's results): oracle.batch agrees with the restatement;
    the batch reaches 128 d for the largest diagonal entry d > 0, and 0 where an entry is <= 0; it gives at least 20
    distinct scores; a single-match pair scores exactly `match`; every value the set's body holds is in [0, 0x7C00) for
    R = 32, 16, 8, with the largest the figure of DESIGN.md 5.1 or below it.
    A constant matrix cannot give 20 distinct scores -- every pair scores 128 s -- and is held to exactly one."""
    p = pe.PARAM_SETS[k]
    a, b, labels = batch()
    H, S, want = reference(k)
    assert np.array_equal(oracle.batch(a, b, p.sm, p.gap), want), p.label
    pa, pb, origin = pe.place(a, b)
    placed = oracle.batch(pa, pb, p.sm, p.gap)
    built = origin >= 0
    assert np.array_equal(placed[built], want[origin[built]]), p.label
    assert np.array_equal(oracle.batch(pe.with_junk(pa), pe.with_junk(pb, 98), p.sm, p.gap), placed), p.label

    sm = p.sm.astype(np.int64).reshape(4, 4)
    off = sm[~np.eye(4, dtype=bool)]
    plain = len(set(np.diag(sm))) == 1 and len(set(off)) == 1       # a match / mismatch matrix
    d = int(np.diag(sm).max())
    if d > 0:
        assert 128 * d in want, p.label
    if sm.min() <= 0:
        assert 0 in want, p.label
    if plain and d > 0 and off[0] <= 0:     # the extreme blocks: the largest score beside 0, in both orders of the halves
        assert want.max() == 128 * d
        assert [tuple(x) for x in np.unique(placed[~built].reshape(-1, 2), axis=0)] == [(0, 128 * d), (128 * d, 0)], p.label
    # Distinct scores: a matrix without a positive entry scores 0 throughout, and a constant one scores 128 s throughout
    # (H(i,j) = s min(i,j) whatever the sequences are): no batch can tell pairs apart under those
    if sm.max() > 0 and sm.min() != sm.max():
        assert len(np.unique(want)) >= 20, (p.label, len(np.unique(want)))
    else:
        assert len(np.unique(want)) == 1, p.label
    if plain and d > 0 and off[0] < 0:
        singles = [i for i, l in enumerate(labels) if l.startswith("single match")]
        assert len(singles) == 70 and np.all(want[singles] == d), p.label

    rb = pe.row_bytes(p.sm, p.gap, p.variant)
    assert 0 <= rb.min() and rb.max() <= 255, p.label
    for rows_per_lane, (lo, hi) in held(k).items():
        assert 0 <= lo and hi < pe.PK_LIMIT, (p.label, rows_per_lane, lo, hi)
        assert hi <= HELD_MAX[p.variant][rows_per_lane], (p.label, rows_per_lane, hi)
        if p.variant == "vert":             # the closed form make_config checks bounds what the sweep really holds
            assert hi < 128 * max(0, int(sm.max())) + 34 * p.gap + 256


def test_the_largest_held_values_are_the_documented_ones():
    """HELD_MAX is reached, not only respected: per body and rows per lane, the largest value over the table"""
    for variant in pe.VARIANTS:
        mine = [held(k) for k, p in enumerate(pe.PARAM_SETS) if p.variant == variant]
        top = {r: max(h[r][1] for h in mine) for r in (32, 16, 8)}
        assert top == HELD_MAX[variant], (variant, top)


def test_one_vs_many_batches_against_the_restatement(oracle):
    """the oracle on a shared seq2 (broadcast, as the GPU test does) against the restatement, under each body's extreme set"""
    extreme = [q for q in pe.PARAM_SETS if q.label.startswith(("q0 127/-127 gap 127", "vert 127/-128 gap 64", "bias 127/-128 gap 0"))]
    assert [q.variant for q in extreme] == ["q0", "vert", "bias"]
    for label, s1, s2 in pe.ovm_batches()[:2]:
        b = np.broadcast_to(s2, s1.shape).copy()
        for p in extreme:
            H, _ = pe.numpy_sw(s1, b, p.sm, p.gap)
            assert np.array_equal(oracle.batch(s1, b, p.sm, p.gap), H.max(axis=(0, 1))), (label, p.label)
