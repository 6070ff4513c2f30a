"""The flag form of the packed scorer without a GPU: the host rule (csrc/pk_form.h through swmi_pk_cell_form) on both sides of
each of its conditions, and the numpy model of the cell on 16-bit patterns (pk_flag_form.flag_model) against the recurrence
restated in pk_edges.numpy_sw -- scores, every H, and the range argument: enabled diagonal terms and max3 results stay in
[0, 0x7C00), disabled ones are finite negative half-precision patterns, no add carries out of its half."""
import numpy as np
import pytest

import pk_edges as pe
import pk_flag_form as pf


@pytest.mark.parametrize("k", range(len(pf.RULE_SETS)), ids=[p.label for p in pf.RULE_SETS])
def test_rule_gives_the_claimed_form(swmi_mod, k):
    p = pf.RULE_SETS[k]
    assert pf.expected_form(p.sm, p.gap) == p.form                     # the restatement against the hand-made claim
    assert pf.flag_rule(p.sm, p.gap) == p.scale
    form, unit, scaled_gap = swmi_mod.pk_form.cell_form(p.sm, p.gap)    # the library's rule
    assert pf.FORMS[form] == p.form
    assert (unit, scaled_gap) == (p.scale or (0, 0))
    # the kernel and its reported name are the existing rule's: the flag form lives inside the vertical-offset instantiations
    swmi_mod.set_schedule(0, 0)
    name, _ = swmi_mod.score_kernel_for_batch(1 << 20, p.sm, p.gap)
    assert name == pe.expected_name(0, pe.expected_variant(p.sm, p.gap), 4)


def test_rule_agrees_with_its_restatement_on_a_sweep(swmi_mod):
    """match / mismatch matrices over a grid, and random two-valued asymmetric matrices: the C rule is the Python rule"""
    rng = np.random.default_rng(3)
    flagged = 0
    for gap in (1, 2, 3, 5, 15, 17, 30, 50, 64, 100, 127):
        for m in (-20, -1, 0, 1, 2, 7, 10, 16, 36, 50, 70, 127):
            for low in (-2 * gap - 1, -2 * gap, -2 * gap + 1, -gap):
                if -128 <= low <= 127:
                    cases = [pf.match_matrix(m, low)]
                    cells = [(int(a), int(b)) for a, b in zip(*np.nonzero(rng.random((4, 4)) < 0.4))]
                    cases.append(pf.matrix_of(cells, m, low))
                    for sm in cases:
                        form, unit, scaled_gap = swmi_mod.pk_form.cell_form(sm, gap)
                        assert pf.FORMS[form] == pf.expected_form(sm, gap), (sm, gap)
                        assert (unit, scaled_gap) == (pf.flag_rule(sm, gap) or (0, 0))
                        flagged += form == 3
    assert flagged > 20
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.pk_form.cell_form(pf.match_matrix(10, -30), -1)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.pk_form.cell_form(pf.match_matrix(10, -30), 128)


_BATCHES = {}


def _batch(which):
    if which not in _BATCHES:
        a, b, labels = pf.build_batch() if which == "flag" else pe.build_batch()
        _BATCHES[which] = (a, b, labels)
    return _BATCHES[which]


# the model runs wherever the mathematics holds, which is wider than the host rule: the strict set (10, -40, 15) is not sent to
# the flag form (its kernel is the bias one) but its scores -s <= -2 gap never deciding a cell- come out of the model all the same
MODEL_SETS = [(p.label, p.sm, p.gap) + p.scale for p in pf.RULE_SETS if p.form == "flag"] + [
    ("strict 10/-40 gap 15 (model only)", pf.match_matrix(10, -40), 15, 25, 153),
    ("asymmetric strict 10/-128 gap 15 (model only)", pf.matrix_of(pf.ASYMMETRIC, 10, -128), 15, 25, 153)]


@pytest.mark.parametrize("which", ["flag", "edges"])
@pytest.mark.parametrize("k", range(len(MODEL_SETS)), ids=[s[0] for s in MODEL_SETS])
def test_model_is_the_recurrence(k, which):
    label, sm, gap, unit, scaled_gap = MODEL_SETS[k]
    a, b, labels = _batch(which)
    H, _ = pe.numpy_sw(a, b, sm, gap)
    want = H.max(axis=(0, 1))
    got, Hm, seen = pf.flag_model(a, b, sm, gap, unit, scaled_gap)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (label, labels[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
    assert np.array_equal(Hm * unit, H * 255)                   # every held H is the true one, rescaled: no disabled term ever won
    # the range argument
    assert seen["carries"] == 0
    assert 0 <= seen["min_enabled"] and seen["max_enabled"] < pf.PK_LIMIT and seen["max_x"] < pf.PK_LIMIT
    m = unit - gap
    assert seen["max_x"] <= 255 * (128 * max(m, 0) + gap) // unit + 255      # the host rule's bound holds what the cell holds
    if seen["max_negative_magnitude"]:
        assert 0x00FF <= seen["min_negative_magnitude"] and seen["max_negative_magnitude"] < pf.PK_LIMIT
    if which == "flag" and m > 0:
        assert want.max() == 128 * m and want.min() == 0         # the batch reaches the top of the range and the all-zero case
