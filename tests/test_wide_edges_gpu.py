"""The three wide-alphabet libraries (swmi.wide, swmi.wide_long, swmi.wide_profile) on the GPU, on the hand-built inputs of
wide_edges.py: 4-letter hand cases relabelled over 32 letters with a trap filler, and the profile census.  Every comparison is
exact integer equality, with a traceback and ends-only, against the hand-pinned fields or closed forms AND against the C
restatement (tests/native/wide_affine_oracle.c, wide_profile_oracle.c).  test_wide_edges_cpu.py shows without a device that the
inputs reach the edges they claim and that a transposed lookup, a dropped letter bit or a column off by one changes a field in
every family.

swmi.wide: every family of the local and the global kind under its own mask, several cases in one ragged call between random
neighbours over all 32 letters (wave counts 1 - 4 side by side); the census, one call per shift.  swmi.wide_profile: the census
as position-specific profiles, and every family through from_sequence, which must also equal swmi.wide on the replicated query.
swmi.wide_long at stripe widths 0, 1 and 4: ties, the last column and the hand-over across column 4096.  And the full shape
16384 x 4096 (four wavefronts, 137 KiB of LDS) once, on closed forms and on a related pair."""
import numpy as np
import pytest

import wide_edges as we
from wide_profile_support import ProfileOracle
from wide_support import GLOBAL, LOCAL, WideOracle, assert_same, inputs, moves_of, scoring_matrix

pytestmark = pytest.mark.gpu

FAMILIES = we.families()
RELABELLINGS = range(len(we.RELABELLINGS))
WIDTHS = [0, 1, 4]


@pytest.fixture(scope="module")
def woracle(tmp_path_factory):
    return WideOracle(tmp_path_factory.mktemp("wide_edges_gpu_oracle"))


@pytest.fixture(scope="module")
def poracle(tmp_path_factory):
    return ProfileOracle(tmp_path_factory.mktemp("wide_edges_gpu_profile_oracle"))


@pytest.fixture(scope="module")
def wide(swmi_mod):
    swmi_mod.wide.load()
    return swmi_mod.wide


@pytest.fixture(scope="module")
def wp(swmi_mod):
    swmi_mod.wide_profile.load()
    return swmi_mod.wide_profile


@pytest.fixture(scope="module")
def wl(swmi_mod):
    swmi_mod.wide_long.load()
    return swmi_mod.wide_long


@pytest.fixture(scope="module")
def neighbours():
    """Random alignments over all 32 letters at one to four wavefronts, put between the hand cases of a call; never changed."""
    return inputs([(70, 100), (33, 1500), (70, 2500), (40, 4000), (129, 1025), (5, 4096)], seed=91)


def _run(lib, kind, a, b, sm, go, ge, mask, traceback):
    if kind == LOCAL:
        return lib.local(a, b, sm, go, ge, traceback=traceback)
    return lib.global_(a, b, sm, go, ge, mask, traceback=traceback)


def _check_call(lib, woracle, call, what, cache=None):
    """One ragged call on the GPU, with a traceback and ends-only: the restatement's result, and the pinned fields."""
    kind, mask, a, b, sm, go, ge, where = call
    for tb in (True, False):
        key = (what, tb)
        if cache is None or key not in cache:
            want = woracle.align(kind, a, b, sm, go, ge, mask, traceback=tb)
            if cache is not None:
                cache[key] = want
        else:
            want = cache[key]
        got = _run(lib, kind, a, b, sm, go, ge, mask, tb)
        assert_same(got, want, (what, tb), traceback=tb)
        for case, first in where:
            if case.pinned is not None:
                we.assert_pinned(got, first, case.pinned, (what, case, tb), traceback=tb)


# ---- swmi.wide ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", RELABELLINGS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_relabelled_families(wide, woracle, neighbours, family, index):
    calls = we.calls_of(FAMILIES[family], we.RELABELLINGS[index], neighbours)
    for x, call in enumerate(calls):
        assert len({-(-len(y) // we.WAVE_COLS) for y in call[3]}) == we.MAX_WAVES          # wave counts 1 - 4 side by side
        _check_call(wide, woracle, call, (family, index, x))


@pytest.mark.parametrize("kind", [LOCAL, GLOBAL])
def test_census(wide, woracle, kind):
    """One call per shift: every (column of lanes 0, 31, 63 of the four waves, letter row) and every (p, q) decides one result."""
    for cen in we.census_calls(kind) + [c for c in we.extreme_census_calls() if c.kind == kind]:
        for tb in (True, False):
            got = _run(wide, cen.kind, cen.a, cen.b, cen.sm, *we.CENSUS_GAPS, cen.mask, tb)
            we.assert_pinned(got, 0, cen.pinned, (cen.name, tb), traceback=tb)
            assert_same(got, woracle.align(cen.kind, cen.a, cen.b, cen.sm, *we.CENSUS_GAPS, cen.mask, traceback=tb), (cen.name, tb), traceback=tb)


# ---- swmi.wide_profile ----------------------------------------------------------------------------------------------------------

def _run_profile(wp, kind, seqs, profile, go, ge, mask, traceback):
    if kind == LOCAL:
        return wp.local(seqs, profile, go, ge, traceback=traceback)
    return wp.global_(seqs, profile, go, ge, mask, traceback=traceback)


@pytest.mark.parametrize("len2", we.PROFILE_LEN2S)
def test_profile_census(wp, poracle, len2):
    """The census written straight into a position-specific profile (no from_sequence): one call per len2 and kind."""
    for kind in (LOCAL, GLOBAL):
        profile, seqs, pinned, mask = we.profile_census(len2, kind)
        for tb in (True, False):
            got = _run_profile(wp, kind, seqs, profile, *we.CENSUS_GAPS, mask, tb)
            we.assert_pinned(got, 0, pinned, (len2, kind, tb), traceback=tb)
            assert_same(got, poracle.align(kind, seqs, profile, *we.CENSUS_GAPS, mask, traceback=tb), (len2, kind, tb), traceback=tb)


@pytest.mark.parametrize("index", RELABELLINGS)
def test_families_as_from_sequence_profiles(wp, wide, index):
    """Every relabelled case against the profile of its own relabelled seq2, one profile per call: the pinned fields, and
    swmi.wide's result on the same pair, field by field and move by move."""
    for family, cases in sorted(FAMILIES.items()):
        for x, (kind, mask, a, b, sm, go, ge, where) in enumerate(we.calls_of(cases, we.RELABELLINGS[index])):
            for tb in (True, False):
                want = _run(wide, kind, a, b, sm, go, ge, mask, tb)
                for case, first in where:
                    for k in range(first, first + len(case.a)):
                        got = _run_profile(wp, kind, [a[k]], wp.from_sequence(b[k], sm), go, ge, mask, tb)
                        assert_same(got, we.result_slice(want, k, 1), (family, index, x, k, tb), traceback=tb)
                        if case.pinned is not None:
                            we.assert_pinned(got, 0, case.pinned[k - first:k - first + 1], (family, index, case, tb), traceback=tb)


# ---- swmi.wide_long -------------------------------------------------------------------------------------------------------------

_LONG_WANT = {}


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("index", RELABELLINGS)
def test_long_families_across_column_4096(wl, woracle, index, width):
    """Stripes of 1024 columns (width 1), of 4096 (width 4) and the library's own rule (0): the shifted path ties over columns
    4033 .. 4160, the end cell in column 4097 with a stripe of padding beside it, the hand-over from column 4096 to 4097."""
    wl.set_stripe_waves(width)
    try:
        for family, cases in sorted(we.long_families().items()):
            for x, call in enumerate(we.calls_of(cases, we.RELABELLINGS[index])):
                _check_call(wl, woracle, call, (family, index, x), cache=_LONG_WANT)
    finally:
        wl.set_stripe_waves(0)


# ---- the full shape ---------------------------------------------------------------------------------------------------------------

def test_the_full_shape_16384_by_4096(wide, woracle):
    """One alignment of 16384 x 4096 per case: four wavefronts, the whole profile, the walk's staging block where wave 0's profile
    lay.  Closed forms under match 127 / mismatch -127 (relabelled by a permutation of all 32 letters) and under all -128, gaps
    (127, 127) -- the largest and the most negative score the shapes allow -- and a related pair whose path crosses all four
    waves and many staging blocks."""
    rng = np.random.default_rng(31000)
    len1, len2 = we.MAX_LEN1, we.MAX_LEN2
    perm = rng.permutation(32).astype(np.uint8)
    assert not np.array_equal(perm, np.arange(32))
    x = rng.integers(0, 32, len1, dtype=np.uint8)
    y = perm[x[:len2]]
    sm = np.full((32, 32), -127, np.int8)
    sm[np.arange(32), perm] = 127
    sm = sm.reshape(-1)
    junk = lambda s: (s | (rng.integers(0, 8, len(s), dtype=np.uint8) << 5)).astype(np.uint8)  # noqa: E731
    a, b = [junk(x)], [junk(y)]
    # local: seq2 is the head of seq1 and nothing else holds 4096 matches in a row
    for tb in (True, False):
        got = wide.local(a, b, sm, 127, 127, traceback=tb)
        we.assert_pinned(got, 0, [(127 * len2, (len2, len2, 0, 0), [we.DIAG] * len2)], ("full local", tb), traceback=tb)
        assert_same(got, woracle.align(LOCAL, a, b, sm, 127, 127, traceback=tb), ("full local", tb), traceback=tb)
    # global under mask 0: every column matched, 12288 rows of gap at 127 each; where the gaps lie is the restatement's to say
    want = woracle.align(GLOBAL, a, b, sm, 127, 127, 0)
    got = wide.global_(a, b, sm, 127, 127, 0)
    assert int(got[0][0]) == 127 * len2 - 127 * (len1 - len2) and tuple(got[1][0]) == (len1, len2, 0, 0) and int(got[4][0]) == len1
    assert moves_of(got, 0).count(we.DIAG) == len2 and moves_of(got, 0).count(we.UP) == len1 - len2
    assert_same(got, want, "full global")
    assert_same(wide.global_(a, b, sm, 127, 127, 0, traceback=False), woracle.align(GLOBAL, a, b, sm, 127, 127, 0, traceback=False), "full global ends-only",
                traceback=False)
    # nothing matches, all -128: each of the 4096 diagonals replaces two gap moves (254) by 128
    low = np.full(1024, -128, np.int8)
    want = woracle.align(GLOBAL, a, b, low, 127, 127, 0)
    got = wide.global_(a, b, low, 127, 127, 0)
    assert int(got[0][0]) == -128 * len2 - 127 * (len1 - len2) == -2084864 and tuple(got[1][0]) == (len1, len2, 0, 0) and int(got[4][0]) == len1
    assert_same(got, want, "full all -128")
    ends_only = wide.global_(a, b, low, 127, 127, 0, traceback=False)
    assert int(ends_only[0][0]) == -2084864 and tuple(ends_only[1][0]) == (len1, len2, -1, -1)
    # a related pair: seq2 a noisy copy of 4096 letters out of seq1's middle with two indels, under a scoring matrix
    sm = scoring_matrix(23)
    piece = x[6000:6000 + len2 + 30].copy()
    noise = rng.random(len(piece)) < 0.08
    piece[noise] = rng.integers(0, 32, int(noise.sum()), dtype=np.uint8)
    z = np.concatenate([piece[:1500], piece[1530:3000], rng.integers(0, 32, 9, dtype=np.uint8), piece[3000:]])[:len2]
    b = [junk(z)]
    for kind, mask in ((LOCAL, 0), (GLOBAL, 0)):
        want = woracle.align(kind, a, b, sm, 6, 1, mask)
        assert_same(_run(wide, kind, a, b, sm, 6, 1, mask, True), want, ("full related", kind))
        codes = moves_of(want, 0)
        assert {we.DIAG, we.UP, we.LEFT} <= set(codes) and int(want[4][0]) > 3000
        if kind == LOCAL:                                        # the path crosses all four waves and more than 20 staging blocks of 128 rows
            assert int(want[1][0, 3]) < 1024 and int(want[1][0, 1]) > 3072 and int(want[1][0, 0]) - int(want[1][0, 2]) > 20 * 128
    wide.release_workspaces()
