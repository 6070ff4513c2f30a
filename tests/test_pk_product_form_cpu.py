"""The product form of the packed scorer without a GPU: the host rule (csrc/pk_form.h through swmi_pk_product_form) on both
sides of each of its conditions, the committed constants against their window -- exhaustively, every (row base, column base)
and every H up to the verified bound -- the generated include against its generator, and the numpy model of the cell on 16-bit
patterns (pk_product_form.product_model) against the recurrence and against the flag form's model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pk_edges as pe
import pk_flag_form as pf
import pk_product_form as pp
from conftest import PKG


def _consts(swmi_mod):
    ok, a, b, bound = swmi_mod.pk_form.product_form(pp.RULE_SETS[0].sm, pp.RULE_SETS[0].gap)
    assert ok
    return a, b, bound


def test_constants_are_what_their_generator_prints():
    csrc = os.path.join(PKG, "csrc")
    out = subprocess.run([sys.executable, os.path.join(csrc, "gen_pk_product_consts.py")], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out == open(os.path.join(csrc, "pk_product_consts_gen.inc")).read(), "run: python3 gen_pk_product_consts.py > pk_product_consts_gen.inc (in csrc/)"


@pytest.mark.parametrize("k", range(len(pp.RULE_SETS)), ids=[p.label for p in pp.RULE_SETS])
def test_rule_gives_the_claimed_form(swmi_mod, k):
    p = pp.RULE_SETS[k]
    a, b, bound = _consts(swmi_mod)
    assert bound >= 13056                                               # the headline's largest rescaled H
    assert pf.expected_form(p.sm, p.gap) == p.form
    assert pp.product_rule(p.sm, p.gap, bound) == p.product             # the restatement against the hand-made claim
    ok, ra, rb, rbound = swmi_mod.pk_form.product_form(p.sm, p.gap)     # the library's rule
    assert ok == p.product
    assert (ra, rb, rbound) == ((a, b, bound) if p.product else ((0,) * 4, (0,) * 4, 0))
    # the form swmi_pk_cell_form reports, its scale and the kernel's name are the flag form's: the product form lives inside it
    form, unit, scaled_gap = swmi_mod.pk_form.cell_form(p.sm, p.gap)
    assert pf.FORMS[form] == p.form
    assert (unit, scaled_gap) == (pf.flag_rule(p.sm, p.gap) or (0, 0))
    swmi_mod.set_schedule(0, 0)
    assert swmi_mod.score_kernel_for_batch(1 << 20, p.sm, p.gap)[0] == pe.expected_name(0, pe.expected_variant(p.sm, p.gap), 4)


def test_rule_agrees_with_its_restatement_on_a_sweep(swmi_mod):
    """match / mismatch matrices over a grid, each also with one diagonal entry disabled and with one more entry enabled"""
    _, _, bound = _consts(swmi_mod)
    eligible = refused_by_bound = 0
    for gap in (1, 2, 3, 5, 15, 17, 30, 50, 64, 100, 127):
        for m in (-20, -1, 0, 1, 2, 7, 10, 16, 36, 50, 70, 127):
            for low in (-2 * gap - 1, -2 * gap, -2 * gap + 1, -gap):
                if -128 <= low <= 127:
                    plain = pf.match_matrix(m, low)
                    for sm in (plain, pf.matrix_of(pf.DIAGONAL[1:], m, low), pf.matrix_of(pf.DIAGONAL + [(2, 1)], m, low)):
                        want = pp.product_rule(sm, gap, bound)
                        assert swmi_mod.pk_form.product_form(sm, gap)[0] == want, (sm, gap)
                        eligible += want
                        refused_by_bound += bool(sm is plain and pf.flag_rule(sm, gap) and low <= -2 * gap and not want)
    assert eligible > 10 and refused_by_bound > 3
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.pk_form.product_form(pf.match_matrix(10, -30), -1)
    with pytest.raises(swmi_mod.SwmiError):
        swmi_mod.pk_form.product_form(pf.match_matrix(10, -30), 128)


def test_constants_hold_their_window_for_every_h(swmi_mod):
    a, b, bound = _consts(swmi_mod)
    d = np.arange(bound + 1, dtype=np.int64)
    lowest, highest = 0xFFFF, 0
    for r in range(4):
        for c in range(4):
            assert 0 <= a[r] < 65536 and 0 <= b[c] < 65536
            t = (a[r] * b[c] + d) & 0xFFFF
            if r == c:
                assert np.array_equal(t, d + pp.K)
                assert t.max() < pp.PK_LIMIT
            else:
                assert a[r] * b[c] % 65536 + bound <= 0xFFFF             # no sum wraps back to a non-negative pattern
                assert ((t & 0x8000) != 0).all()
                mag = t & 0x7FFF
                assert mag.min() >= 0x00FF and mag.max() < pp.PK_LIMIT    # the domain swmi_pk_selftest_max3_negative covers
                lowest, highest = min(lowest, int(mag.min())), max(highest, int(mag.max()))
    assert 0x00FF <= lowest and highest < pp.PK_LIMIT


_BATCHES = {}


def _batch(which):
    if which not in _BATCHES:
        _BATCHES[which] = pf.build_batch() if which == "flag" else pe.build_batch()
    return _BATCHES[which]


MODEL_SETS = [p for p in pp.RULE_SETS if p.product]


@pytest.mark.parametrize("which", ["flag", "edges"])
@pytest.mark.parametrize("k", range(len(MODEL_SETS)), ids=[p.label for p in MODEL_SETS])
def test_model_is_the_recurrence_and_the_flag_model(swmi_mod, k, which):
    p = MODEL_SETS[k]
    row_mul, col_mul, bound = _consts(swmi_mod)
    unit, scaled_gap = pf.flag_rule(p.sm, p.gap)
    a, b, labels = _batch(which)
    H, _ = pe.numpy_sw(a, b, p.sm, p.gap)
    want = H.max(axis=(0, 1))
    got, Hm, seen = pp.product_model(a, b, p.gap, unit, scaled_gap, row_mul, col_mul)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (p.label, labels[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
    assert np.array_equal(Hm * unit, H * 255)                   # every held H is the true one, rescaled: no disabled term ever won
    flag_scores, flag_H, _ = pf.flag_model(a, b, p.sm, p.gap, unit, scaled_gap)
    assert np.array_equal(got, flag_scores) and np.array_equal(Hm, flag_H)
    # the range argument
    m = unit - p.gap
    assert seen["wraps"] == 0
    assert seen["max_h"] <= 255 * 128 * max(m, 0) // unit <= bound         # the host rule's bound holds what the cell holds
    assert 0 <= seen["min_enabled"] and seen["max_enabled"] < pp.PK_LIMIT and seen["max_x"] < pp.PK_LIMIT
    assert 0x00FF <= seen["min_negative_magnitude"] and seen["max_negative_magnitude"] < pp.PK_LIMIT
    if which == "flag" and m > 0:
        # the extremes are reached, not only respected: 128 matches in a row give the largest H and the largest enabled term;
        # a mismatch beside them adds the largest H but one row to an off-diagonal product, and one on an all-zero state adds 0
        assert want.max() == 128 * m and want.min() == 0
        assert seen["max_h"] == 255 * 128 * m // unit and seen["max_enabled"] == 255 * 127 * m // unit + 255
        off = [row_mul[r] * col_mul[c] % 65536 for r in range(4) for c in range(4) if r != c]
        assert seen["min_negative_magnitude"] == min(off) - 0x8000
        assert seen["max_negative_magnitude"] >= max(off) - 0x8000
