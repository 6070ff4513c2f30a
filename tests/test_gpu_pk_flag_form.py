"""The flag form of the packed scorer on the GPU: eligible parameter sets, the strict set and the ineligible neighbour, at every
forced lane count, in all three modes, on batches of 1, 2A - 1, 2A, 2A + 1 alignments (A = alignments per wavefront: the ragged
tail) and on the whole structured batch of pk_flag_form.py -- every score equal to oracle/sw_oracle.c, the reported kernel name
the existing rule's; and the exhaustive self-test of the premise (a finite negative half loses v_pk_maximum3_f16)."""
import numpy as np
import pytest

import pk_edges as pe
import pk_flag_form as pf

pytestmark = pytest.mark.gpu

_CACHE = {}


def _inputs(oracle):
    if "in" not in _CACHE:
        a, b, labels = pf.build_batch()
        shared = [("homopolymer 1", pe.homopolymer(1)), ("random", np.random.default_rng(11).integers(0, 4, 128).astype(np.uint8)),
                  ("seq1 of pair 40", a[40].copy())]
        _CACHE["in"] = dict(a=a, b=b, labels=labels, pka=oracle.pack(a), pkb=oracle.pack(b), shared=shared)
    return _CACHE["in"]


def _want(oracle, k, shared=None):
    """oracle scores under GPU_SETS[k]: the pairs batch, or every seq1 against shared sequence `shared`; computed once"""
    if (k, shared) not in _CACHE:
        p, x = pf.GPU_SETS[k], _inputs(oracle)
        b = x["b"] if shared is None else np.broadcast_to(x["shared"][shared][1], x["a"].shape).copy()
        want = oracle.batch(x["a"], b, p.sm, p.gap)
        want.setflags(write=False)
        _CACHE[(k, shared)] = want
    return _CACHE[(k, shared)]


@pytest.mark.parametrize("lanes", pe.LANES)
@pytest.mark.parametrize("k", range(len(pf.GPU_SETS)), ids=[p.form + " " + p.label.split(":")[0] for p in pf.GPU_SETS])
def test_scores_and_kernel_name(gpu, oracle, k, lanes):
    p, x = pf.GPU_SETS[k], _inputs(oracle)
    n = len(x["a"])
    per_wave = 128 // lanes
    sizes = [1, 2 * per_wave - 1, 2 * per_wave, 2 * per_wave + 1, n]
    assert n >= sizes[3]
    assert pf.FORMS[gpu.pk_form.cell_form(p.sm, p.gap)[0]] == p.form
    gpu.set_schedule(lanes, 0)
    try:
        for mode, m in pe.MODES.items():
            name, got_per_wave = gpu.score_kernel_for_batch(n, p.sm, p.gap, m)
            assert name == pe.expected_name(m, pe.expected_variant(p.sm, p.gap), lanes) and got_per_wave == per_wave
            for t in sizes:
                if mode == "pairs":
                    runs = [("", gpu.score_batch(x["a"][:t], x["b"][:t], p.sm, p.gap), _want(oracle, k)[:t])]
                elif mode == "packed2bit":
                    runs = [("", gpu.score_batch_packed(x["pka"][:t], x["pkb"][:t], p.sm, p.gap), _want(oracle, k)[:t])]
                else:
                    runs = [(label, gpu.score_one_vs_many(x["a"][:t], s2, p.sm, p.gap), _want(oracle, k, w)[:t])
                            for w, (label, s2) in enumerate(x["shared"])]
                for label, got, want in runs:
                    bad = np.nonzero(got != want)[0]
                    assert not len(bad), (p.label, mode, lanes, t, label, "%d wrong, first: pair %d (%s) got %d want %d" % (
                        len(bad), bad[0], x["labels"][bad[0]], got[bad[0]], want[bad[0]]))
    finally:
        gpu.set_schedule(0, 0)


def test_default_schedule_large_batch(gpu, oracle):
    """what the default schedule runs for a batch that fills the chip (L = 4 by choice, not by force), on 100 000 generated pairs
    with every fourth one made similar"""
    n = 100000
    a, b = gpu.generate_pairs_host(n, 4242, 0)
    b[::4] = np.where(np.random.default_rng(5).random((len(b[::4]), 128)) < 0.9, a[::4], b[::4])
    for p in (pf.GPU_SETS[0], pf.GPU_SETS[2]):
        assert gpu.score_kernel_for_batch(n, p.sm, p.gap)[0] == "sw128_pk_kernel<0,2>"
        got, want = gpu.score_batch(a, b, p.sm, p.gap), oracle.batch(a, b, p.sm, p.gap)
        assert np.array_equal(got, want), (p.label, int((got != want).sum()))


def test_a_negative_half_loses_the_packed_max3(gpu):
    checked, bad = gpu.pk_form.selftest_max3_negative()
    assert checked == 9 * 0x7C00 ** 2
    assert bad == 0
