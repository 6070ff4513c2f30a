"""wide_edges.py without a device: the inputs mean what they claim.  Every relabelled hand case gives, through the C restatements
tests/native/wide_affine_oracle.c and wide_profile_oracle.c, the hand-pinned score, ends and codes and exactly the 4-letter
restatement's result on the unrelabelled case (whose edge predicates test_local_full_affine_edges_cpu.py confirms; the
counterparts that only this file builds have theirs confirmed here); the census alignments give their closed forms and reach
every profile byte they claim; and the traps bite: the restatement called with a transposed matrix, with letters masked to four
bits or with seq2 one column off changes a field in every family, while another filler changes none.  Every comparison is exact
integer equality."""
import numpy as np
import pytest

import affine_edges as ae
import local_full_affine_edges as lfe
import wide_edges as we
from global_full_affine_support import GlobalFullAffineOracle
from local_full_affine_support import LocalFullAffineOracle
from wide_profile_support import ProfileOracle, from_sequence
from wide_support import GLOBAL, LOCAL, WideOracle, assert_same

ALL_FAMILIES = dict(we.families(), **we.long_families())


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("wide_edges_oracles")
    return {"wide": WideOracle(tmp), "profile": ProfileOracle(tmp), LOCAL: LocalFullAffineOracle(tmp), GLOBAL: GlobalFullAffineOracle(tmp)}


_FOUR = {}


def _four_letter_result(oracles, case):
    """The 4-letter restatement's result on the unrelabelled case, in the ragged layout; computed once per case."""
    if id(case) not in _FOUR:
        A, B = np.stack(case.a), np.stack(case.b)
        if case.kind == LOCAL:
            r = oracles[LOCAL].align(A, B, case.sm4, case.gap_open, case.gap_extend)
        else:
            r = oracles[GLOBAL].align(A, B, case.sm4, case.gap_open, case.gap_extend, case.mask)
        _FOUR[id(case)] = we.fixed_as_ragged(case.a, case.b, r)
    return _FOUR[id(case)]


def _align(oracles, call, fault=None, relabelling=None, traceback=True):
    kind, mask, a, b, sm, go, ge, _ = call
    if fault is not None:
        a, b, sm = we.with_fault(fault, a, b, sm, relabelling)
    return oracles["wide"].align(kind, a, b, sm, go, ge, mask, traceback=traceback)


def test_the_wide_constants_and_the_replaced_cases():
    assert (we.MAX_WAVES, we.MAX_LEN1, we.MAX_LEN2, we.LONG_MAX_LEN) == (4, 16384, 4096, 65536)
    assert we.MAX_WAVES * we.WAVE_COLS == we.MAX_LEN2 and we.TIE_C0 == 960
    # the five hand cases of the 4-letter file that do not fit 4096 columns, and their counterparts
    assert we.replaced_hands() == ["carried_F/r=2100/x=2300", "last_column/15361/0,0", "last_column/15361/0,3", "last_column/15361/2,1",
                                   "long_left/last_wave"]
    names = {c.name for cases in we.local_families().values() for c in cases}
    assert {"carried_F/r=1400/x=1300", "last_column/3073/0,0", "last_column/3073/0,3", "last_column/3073/2,1", "long_left/last_wave",
            "columns_1024_1025/0,0", "columns_2048_2049/0,4", "columns_3072_3073/0,0"} <= names
    kept = {h.name for make in lfe.hand_groups().values() for h in make()} - set(we.replaced_hands())
    assert kept <= names and len(kept) == 36
    # the maps: injective, rows != cols in two of them, letters >= 16 in two, both fillers
    for rows, cols, filler in we.RELABELLINGS:
        assert len(set(rows)) == len(set(cols)) == 4 and filler in (127, -128)
    assert [r != c for r, c, _ in we.RELABELLINGS] == [False, True, True] and [max(r) >= 16 for r, _, _ in we.RELABELLINGS] == [False, True, True]
    # the long library's cases lie across its stripe edge
    assert all(len(c.b[0]) > we.MAX_LEN2 for cases in we.long_families().values() for c in cases)


@pytest.mark.parametrize("index", range(len(we.RELABELLINGS)))
@pytest.mark.parametrize("family", sorted(ALL_FAMILIES))
def test_relabelled_cases_keep_every_pinned_field(oracles, family, index):
    relabelling = we.RELABELLINGS[index]
    cases = ALL_FAMILIES[family]
    for call in we.calls_of(cases, relabelling):
        got = _align(oracles, call)
        ends_only = _align(oracles, call, traceback=False)
        for case, first in call[7]:
            mine = we.result_slice(got, first, len(case.a))
            assert_same(mine, _four_letter_result(oracles, case), (case, relabelling))
            if case.pinned is not None:
                we.assert_pinned(got, first, case.pinned, (case, relabelling))
                we.assert_pinned(ends_only, first, case.pinned, (case, relabelling, "ends-only"), traceback=False)
        sm = call[4].reshape(32, 32)
        assert int((sm == relabelling[2]).sum()) >= 1024 - 16 and np.concatenate(call[2] + call[3]).max() >= 32       # filler and junk bits
    assert sum(len(c[7]) for c in we.calls_of(cases, relabelling)) == len(cases)


def _facts(case):
    a, b = case.a[0], case.b[0]
    score, end, walk, flags = ae.numpy_affine(a, b, case.sm4, case.gap_open, case.gap_extend, local=True)
    facts = ae.sg_walk_facts(ae.Case(case.name, a[None], b[None], case.sm4, case.gap_open, case.gap_extend, {}), score, walk, flags)
    facts.update(ae.path_tie_facts(walk, flags, True))
    return facts, walk


def test_the_wide_counterparts_reach_the_edges_they_stand_for():
    """Only the cases that this file's callers build with other arguments than local_full_affine_edges.py's own: the predicates
    are affine_edges.py's, evaluated on the numpy tables as test_local_full_affine_edges_cpu.py evaluates them."""
    cases = {c.name: c for cases in we.local_families().values() for c in cases}
    for name, edge in (("carried_F/r=1400/x=1300", 2 * we.WAVE_COLS), ("long_left/last_wave", (we.MAX_WAVES - 1) * we.WAVE_COLS)):
        facts, walk = _facts(cases[name])
        for claim in cases[name].claims:
            assert facts[claim], (name, claim)
        left = walk.j[:-1][walk.codes == we.LEFT]
        assert left.min() <= edge < left.max(), (name, edge)               # the one left run spans the wave edge
    # with the three existing left runs the F runs cross every wave edge of the four wavefronts
    crossed = set()
    for c in cases.values():
        if c.pinned and c.pinned[0][2] is not None and we.LEFT in c.pinned[0][2]:
            codes = np.asarray(c.pinned[0][2])
            j = c.pinned[0][1][1] - np.concatenate([[0], np.cumsum(codes != we.UP)[:-1]])          # the column each move is made from
            left = j[codes == we.LEFT]
            crossed |= {e for e in (1024, 2048, 3072) if left.min() <= e < left.max()}
    assert crossed == {1024, 2048, 3072}
    # the last-column and hand-over counterparts: the end cell in the last valid column, one valid column in wave 3
    for name in ("last_column/3073/0,0", "columns_2048_2049/0,0", "columns_3072_3073/0,4"):
        c = cases[name]
        assert c.gap_open == 0 and c.pinned[0][1][1] in (len(c.b[0]), 2048, 3072)
    # the long library's shifted ties keep the ties their claims count (the 4-letter CPU test shows it for c0 = 960 only)
    for case in we.long_families()["long_path_ties"]:
        tally = dict.fromkeys(case.claims, 0)
        for a, b in zip(case.a, case.b):
            _, _, walk, flags = ae.numpy_affine(a, b, case.sm4, case.gap_open, case.gap_extend, local=True)
            facts = ae.path_tie_facts(walk, flags, True)
            for c in tally:
                tally[c] += bool(facts[c])
            assert len(walk.codes) == 0 or walk.j.max() > we.MAX_LEN2 - 64
        small = {c.name + "/shifted": c for c in ae.local_path_tie_cases()}[case.name]
        for c, least in small.claims.items():
            assert tally[c] >= least, (case, c, tally[c])


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_census_alignments_give_their_closed_forms(oracles, kind):
    calls = we.census_calls(kind) + [c for c in we.extreme_census_calls() if c.kind == kind]
    assert len(calls) == 32 + (1 if kind == LOCAL else 2)
    for cen in calls:
        for tb in (True, False):
            got = oracles["wide"].align(cen.kind, cen.a, cen.b, cen.sm, *we.CENSUS_GAPS, cen.mask, traceback=tb)
            we.assert_pinned(got, 0, cen.pinned, cen.name, traceback=tb)


def test_census_coverage():
    cells, pairs, values = we.census_coverage()
    columns = we.census_columns()
    assert len(columns) == len(set(columns)) == 192 and min(columns) == 1 and max(columns) == we.MAX_LEN2
    assert {(c - 1) // 16 % 64 for c in columns} == {0, 31, 63} and {(c - 1) // 1024 for c in columns} == {0, 1, 2, 3}
    assert {(c, p) for c in columns for p in range(32)} <= cells                    # every letter row at every census column
    assert pairs == {(p, q) for p in range(32) for q in range(32)}                  # every byte of the 32 x 32 matrix decides once
    assert {127, -128} <= values and max(v for v in values if v < 127) >= 64 and len([v for v in values if 64 <= v < 127]) >= 10
    for kind in (LOCAL, GLOBAL):
        probes = [p for cen in we.census_calls(kind) for p in cen.probes]
        assert {(c, p) for c, p, _, _, _ in probes} == {(c, p) for c in columns for p in range(32)}
        assert any(c == len2 for c, _, _, _, len2 in probes) and any(c < len2 for c, _, _, _, len2 in probes)
        assert {r for _, _, _, r, _ in probes} == (set(we.CENSUS_ROWS) if kind == LOCAL else {1})
        assert len({cen.sm.tobytes() for cen in we.census_calls(kind)}) == 32            # all 32 shifts, one call each
    rows_by_letter = {(r, p) for cen in we.census_calls(LOCAL) for _, p, _, r, _ in cen.probes}
    assert len(rows_by_letter) == 32 * len(we.CENSUS_ROWS)


@pytest.mark.parametrize("len2", we.PROFILE_LEN2S)
def test_profile_census_gives_its_closed_forms(oracles, len2):
    rewarded = we.profile_census_columns(len2)
    assert 1 in rewarded and len2 in rewarded and len(set(rewarded.values())) == len(rewarded) and we.PROFILE_BACKGROUND not in rewarded.values()
    assert len(rewarded) == min(31, len({c for c in we.census_columns() if c <= len2} | {1, len2}))
    for kind in (LOCAL, GLOBAL):
        profile, seqs, pinned, mask = we.profile_census(len2, kind)
        assert profile.shape == (len2, 32) and len(seqs) == 32 * (len(we.CENSUS_ROWS) if kind == LOCAL else 1)
        assert int((profile != -3).sum()) == len(rewarded)
        for tb in (True, False):
            got = oracles["profile"].align(kind, seqs, profile, *we.CENSUS_GAPS, mask, traceback=tb)
            we.assert_pinned(got, 0, pinned, (len2, kind), traceback=tb)


@pytest.mark.parametrize("index", range(len(we.RELABELLINGS)))
def test_relabelled_cases_hold_as_from_sequence_profiles(oracles, index):
    """One profile per query (a case's relabelled seq2): the profile restatement gives the pinned fields and the wide one's."""
    relabelling = we.RELABELLINGS[index]
    for family, cases in sorted(we.families().items()):
        for call in we.calls_of(cases, relabelling):
            kind, mask, a, b, sm, go, ge, where = call
            want = _align(oracles, call)
            for k in range(len(a)):
                got = oracles["profile"].align(kind, [a[k]], from_sequence(b[k], sm), go, ge, mask)
                assert_same(got, we.result_slice(want, k, 1), (family, k, relabelling))
            for case, first in where:
                if case.pinned is not None:
                    we.assert_pinned(want, first, case.pinned, (case, relabelling))


# ---- the traps bite ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fault", we.FAULTS)
def test_one_deliberate_fault_at_a_time(oracles, fault):
    """Faults 1 - 3 change at least one field in every family under every relabelling with rows != cols or letters >= 16, and in
    the census; another filler changes nothing under any relabelling."""
    for relabelling in we.RELABELLINGS:
        rows, cols, _ = relabelling
        trapped = rows != cols or max(rows + cols) >= 16
        if fault != "filler_changed" and not trapped:
            continue
        for family, cases in sorted(ALL_FAMILIES.items()):
            changed = False
            for call in we.calls_of(cases, relabelling):
                changed |= we.differs(_align(oracles, call, fault, relabelling), _align(oracles, call))
            assert changed == (fault != "filler_changed"), (fault, family, relabelling)
    if fault == "filler_changed":
        return
    for kind in (LOCAL, GLOBAL):
        changed = 0
        calls = we.census_calls(kind) + [c for c in we.extreme_census_calls() if c.kind == kind]
        for cen in calls:
            a, b, sm = we.with_fault(fault, cen.a, cen.b, cen.sm)
            want = oracles["wide"].align(cen.kind, cen.a, cen.b, cen.sm, *we.CENSUS_GAPS, cen.mask)
            changed += we.differs(oracles["wide"].align(cen.kind, a, b, sm, *we.CENSUS_GAPS, cen.mask), want)
        # a transposed M_s is M_-s: the shifts 0 and 16 are their own transposes, every other call changes
        assert changed >= len(calls) - 2, (fault, kind, changed)

