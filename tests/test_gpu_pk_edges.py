"""The packed scorer sw128_pk_kernel<MODE, VARIANT, L> at the edges of its three cell bodies' domains: every parameter set
of pk_edges.py (row bytes 0 and 255, both sides of each inequality of the dispatch rule, asymmetric matrices) on the
structured batch built there (16 256 beside 0 in one register, single matching cells in every lane-edge row, gap runs across
the lanes' hand-over), placed so that every pair sits in either half of a register, with ragged tails and junk bits.  Each of
the 27 instantiations is forced by lane count and required BY NAME before its scores are compared, bit-exact, with
oracle/sw_oracle.c -- which test_pk_edges_cpu.py pins to a numpy restatement, with the proof that table and batch reach the
edges.  The same table and batch then go through every other schedule of test_gpu_parity.py (int32, 16-bit-max, LDS-lookup
kernels at every lane count)."""
import numpy as np
import pytest

import pk_edges as pe
from test_gpu_parity import SCHEDULES

pytestmark = pytest.mark.gpu

_CACHE = {}


def _inputs(oracle):
    """the placed pairs batch (with its 2-bit packing and junk-bit copy) and the placed one-vs-many batches; built once"""
    if "in" not in _CACHE:
        a, b, _ = pe.build_batch()
        pa, pb, _ = pe.place(a, b)
        ovm = []
        for label, s1, s2 in pe.ovm_batches():
            p1 = pe.place(s1, np.broadcast_to(s2, s1.shape))[0]
            ovm.append((label, p1, s2))
        _CACHE["in"] = dict(a=pa, b=pb, ja=pe.with_junk(pa), jb=pe.with_junk(pb, 98), pka=oracle.pack(pa), pkb=oracle.pack(pb), ovm=ovm,
                            jovm=(pe.with_junk(ovm[0][1]), pe.with_junk(ovm[0][2], 98)))
    return _CACHE["in"]


def _want(oracle, k, which=None):
    """oracle scores of the placed batch under PARAM_SETS[k]: the pairs batch, or one-vs-many batch `which` (seq2 broadcast);
    computed once and left unchanged"""
    key = (k, which)
    if key not in _CACHE:
        p, x = pe.PARAM_SETS[k], _inputs(oracle)
        if which is None:
            want = oracle.batch(x["a"], x["b"], p.sm, p.gap)
        else:
            _, s1, s2 = x["ovm"][which]
            want = oracle.batch(s1, np.broadcast_to(s2, s1.shape).copy(), p.sm, p.gap)
        want.setflags(write=False)
        _CACHE[key] = want
    return _CACHE[key]


def _same(got, want, *what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), what + ("%d wrong, first: pair %d got %d want %d" % (len(bad), bad[0], got[bad[0]], want[bad[0]]),)


@pytest.mark.parametrize("lanes", pe.LANES)
@pytest.mark.parametrize("variant", pe.VARIANTS)
@pytest.mark.parametrize("mode", list(pe.MODES))
def test_packed_kernel_at_its_domain_edges(gpu, oracle, mode, variant, lanes):
    x = _inputs(oracle)
    n = len(x["a"])
    m = pe.MODES[mode]
    ran = 0
    gpu.set_schedule(lanes, 0)
    try:
        for k, p in enumerate(pe.PARAM_SETS):
            if p.variant != variant:
                continue
            name, per_wave = gpu.score_kernel_for_batch(n, p.sm, p.gap, m)
            assert name == pe.expected_name(m, variant, lanes), (p.label, name)
            assert per_wave == 128 // lanes
            if mode == "one_vs_many":
                for w, (label, s1, s2) in enumerate(x["ovm"]):
                    _same(gpu.score_one_vs_many(s1, s2, p.sm, p.gap), _want(oracle, k, w), p.label, mode, lanes, label)
                _, s1, s2 = x["ovm"][0]
                want = _want(oracle, k, 0)
                _same(gpu.score_one_vs_many(x["jovm"][0], x["jovm"][1], p.sm, p.gap), want, p.label, mode, lanes, "junk bits 2..7")
                for t in pe.tail_sizes(lanes, n):
                    _same(gpu.score_one_vs_many(s1[:t], s2, p.sm, p.gap), want[:t], p.label, mode, lanes, "first %d" % t)
            else:
                want = _want(oracle, k)
                if mode == "pairs":
                    score = lambda t: gpu.score_batch(x["a"][:t], x["b"][:t], p.sm, p.gap)
                    _same(gpu.score_batch(x["ja"], x["jb"], p.sm, p.gap), want, p.label, mode, lanes, "junk bits 2..7")
                else:
                    score = lambda t: gpu.score_batch_packed(x["pka"][:t], x["pkb"][:t], p.sm, p.gap)
                _same(score(n), want, p.label, mode, lanes, "all %d" % n)
                for t in pe.tail_sizes(lanes, n):
                    _same(score(t), want[:t], p.label, mode, lanes, "first %d" % t)
            ran += 1
    finally:
        gpu.set_schedule(0, 0)
    assert ran >= 8, "the table holds too few sets for the %s cell" % variant


@pytest.mark.parametrize("lanes,flags", SCHEDULES)
def test_every_other_schedule_at_the_same_edges(gpu, oracle, lanes, flags):
    """pairs mode, the whole table: the int32 kernels (folded, general and 16-bit-max cells), the LDS-lookup kernel and, where
    the schedule leaves it in place, the packed kernel again"""
    x = _inputs(oracle)
    n = len(x["a"])
    gpu.set_schedule(lanes, flags)
    try:
        for k, p in enumerate(pe.PARAM_SETS):
            want = _want(oracle, k)
            _same(gpu.score_batch(x["a"], x["b"], p.sm, p.gap), want, p.label, lanes, flags, "all %d" % n)
            _same(gpu.score_batch(x["ja"][:n - 1], x["jb"][:n - 1], p.sm, p.gap), want[:n - 1], p.label, lanes, flags, "junk bits, first %d" % (n - 1))
    finally:
        gpu.set_schedule(0, 0)
