"""The product form of the packed scorer on the GPU: the exhaustive self-test of its premise (v_pk_mad_i16 with the committed
constants, and the max3 behind it); the two eligible sets on the structured batch of pk_flag_form.py plus the pk_edges pairs, at
every forced lane count, through the pairs, packed and one-vs-many entries, on batches of 1, 31, 32, 33, 81 pairs (the
wavefront boundary at L = 4, and the ragged tail that recomputes the last pair) and on the whole batch -- every score equal
to oracle/sw_oracle.c and to the flag form's own cell, forced through SWMI_PK_NO_PRODUCT; and the ineligible neighbours, which
keep their cells and their scores."""
import os

import numpy as np
import pytest

import pk_edges as pe
import pk_flag_form as pf
import pk_product_form as pp

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 81)
_CACHE = {}


def _inputs(oracle):
    if "in" not in _CACHE:
        fa, fb, fl = pf.build_batch()
        ea, eb, el = pe.build_batch()
        a, b = np.concatenate([fa, ea]), np.concatenate([fb, eb])
        shared = np.random.default_rng(11).integers(0, 4, 128).astype(np.uint8)
        _CACHE["in"] = dict(a=a, b=b, labels=fl + el, pka=oracle.pack(a), pkb=oracle.pack(b), shared=shared)
    return _CACHE["in"]


def _want(oracle, p, ovm):
    """oracle scores under set p: the pairs batch, or every seq1 against the shared sequence; computed once, read-only"""
    key = (p.label, ovm)
    if key not in _CACHE:
        x = _inputs(oracle)
        b = np.broadcast_to(x["shared"], x["a"].shape).copy() if ovm else x["b"]
        want = oracle.batch(x["a"], b, p.sm, p.gap)
        want.setflags(write=False)
        _CACHE[key] = want
    return _CACHE[key]


def _score_all(gpu, x, p, lanes, sizes=None):
    """{(entry, batch size): scores} of set p at the forced lane count, through all three entries; "names": the kernels reported"""
    out = {}
    gpu.set_schedule(lanes, 0)
    try:
        out["names"] = [gpu.score_kernel_for_batch(len(x["a"]), p.sm, p.gap, m)[0] for m in pe.MODES.values()]
        for t in sizes or SIZES + (len(x["a"]),):
            out["pairs", t] = gpu.score_batch(x["a"][:t], x["b"][:t], p.sm, p.gap)
            out["packed2bit", t] = gpu.score_batch_packed(x["pka"][:t], x["pkb"][:t], p.sm, p.gap)
            out["one_vs_many", t] = gpu.score_one_vs_many(x["a"][:t], x["shared"], p.sm, p.gap)
    finally:
        gpu.set_schedule(0, 0)
    return out


def _forced_flag_form(gpu, x, p):
    """the same scores with the product form switched off (the library reads SWMI_PK_NO_PRODUCT when it initialises)"""
    key = ("flag cell", p.label)
    if key not in _CACHE:
        os.environ["SWMI_PK_NO_PRODUCT"] = "1"
        try:
            gpu.shutdown()
            gpu.init(0)
            _CACHE[key] = {lanes: _score_all(gpu, x, p, lanes) for lanes in pe.LANES}
        finally:
            del os.environ["SWMI_PK_NO_PRODUCT"]
            gpu.shutdown()
            gpu.init(0)
    return _CACHE[key]


def test_the_multiply_add_gives_both_addends(gpu):
    a, b, bound = gpu.pk_form.product_form(pp.GPU_ELIGIBLE[0].sm, pp.GPU_ELIGIBLE[0].gap)[1:]
    checked, bad = gpu.pk_form.selftest_product_mad()
    assert checked == 2 * 16 * (bound + 1)          # the multiply-add and the max3 behind it, per (r, c) and H (both halves at once)
    assert bad == 0


@pytest.mark.parametrize("lanes", pe.LANES)
@pytest.mark.parametrize("k", range(len(pp.GPU_ELIGIBLE)), ids=[p.label.split(":")[0] for p in pp.GPU_ELIGIBLE])
def test_scores_match_the_oracle_and_the_flag_cell(gpu, oracle, k, lanes):
    p, x = pp.GPU_ELIGIBLE[k], _inputs(oracle)
    assert gpu.pk_form.product_form(p.sm, p.gap)[0]
    flag = _forced_flag_form(gpu, x, p)[lanes]
    got = _score_all(gpu, x, p, lanes)
    # the kernel and its reported name stay the vertical-offset instantiation's, with the product form and without
    assert got.pop("names") == flag["names"] == [pe.expected_name(m, "vert", lanes) for m in pe.MODES.values()]
    for (entry, t), scores in got.items():
        want = _want(oracle, p, entry == "one_vs_many")[:t]
        bad = np.nonzero(scores != want)[0]
        assert not len(bad), (p.label, entry, lanes, t, "%d wrong, first: pair %d (%s) got %d want %d" % (
            len(bad), bad[0], x["labels"][bad[0]], scores[bad[0]], want[bad[0]]))
        assert np.array_equal(scores, flag[entry, t]), (p.label, entry, lanes, t, "differs from the flag form's cell")


@pytest.mark.parametrize("k", range(len(pp.GPU_NEIGHBOURS)), ids=[p.form + " " + p.label.split(":")[0] for p in pp.GPU_NEIGHBOURS])
def test_ineligible_neighbours_keep_their_cells(gpu, oracle, k):
    p, x = pp.GPU_NEIGHBOURS[k], _inputs(oracle)
    assert not gpu.pk_form.product_form(p.sm, p.gap)[0]
    assert pf.FORMS[gpu.pk_form.cell_form(p.sm, p.gap)[0]] == p.form
    for lanes in pe.LANES:
        got = _score_all(gpu, x, p, lanes, sizes=(33, len(x["a"])))
        assert got.pop("names") == [pe.expected_name(m, pe.expected_variant(p.sm, p.gap), lanes) for m in pe.MODES.values()]
        for (entry, t), scores in got.items():
            assert np.array_equal(scores, _want(oracle, p, entry == "one_vs_many")[:t]), (p.label, entry, lanes, t)
