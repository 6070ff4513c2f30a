"""The table aligners (swmi_local_align*, swmi_semiglobal_full*) on the GPU at the edges of their mappings: shape grids
derived from the kernels' constants, long interior gap runs, staircases and corner exits of the walk's staging blocks,
best cells at wave edges, ties that only the reduction order decides, the pad column with gap 0, the extremes of H, and
bytes 0..255.  Every field bit-exact against the C restatements; table_edges.py builds the inputs and
test_table_edges_cpu.py checks, without a device, that each reaches the edge it claims."""
import numpy as np
import pytest
import torch

import table_edges as te
from local_support import LocalOracle
from sgfull_support import SgFullOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgFullOracle(tmp_path_factory.mktemp("sgfull_oracle"))


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return LocalOracle(tmp_path_factory.mktemp("local_oracle"))


def _sg_both_modes(gpu, a, b, sm, gap, want, what):
    te.assert_same(gpu.semiglobal_full(a, b, sm, gap), want, what, "sgfull")
    sc, ends, _, _ = gpu.semiglobal_full(a, b, sm, gap, traceback=False)
    te.assert_same((sc, ends, None, None), want, (what, "ends-only"), "sgfull", traceback=False)


def _local_both_modes(gpu, a, b, sm, gap, want, what):
    te.assert_same(gpu.local_align(a, b, sm, gap), want, what, "local")
    sc, ends, _, _ = gpu.local_align(a, b, sm, gap, traceback=False)
    te.assert_same((sc, ends[:, :2], None, None), (want[0], want[1][:, :2], None, None), (what, "ends-only"), "local", traceback=False)
    assert (ends[:, 2:] == -1).all(), what


@pytest.mark.parametrize("len1,len2,n", te.sg_shape_grid())
def test_sgfull_shape_grid(gpu, sgoracle, len1, len2, n):
    for name, sm, gap in te.SG_PARAMS:
        a, b = te.sg_mixed_pairs(n, len1, len2, len1 * 7919 + len2 + gap)
        _sg_both_modes(gpu, a, b, sm, gap, sgoracle.align(a, b, sm, gap), ("%dx%d n=%d W=%d" % (len1, len2, n, te.sg_waves(len2)), name))


@pytest.mark.parametrize("len1,n", te.local_shape_grid())
def test_local_shape_grid(gpu, loracle, len1, n):
    for name, sm, gap in te.LOCAL_PARAMS:
        a, b = te.local_mixed_pairs(n, len1, len1 * 131 + n + gap)
        _local_both_modes(gpu, a, b, sm, gap, loracle.align(a, b, sm, gap), ("len1=%d n=%d" % (len1, n), name))


@pytest.mark.parametrize("group", ["gap_runs", "staircases", "corners", "wave_edge_ends", "ties", "pad"])
def test_sgfull_constructed_edges(gpu, sgoracle, group):
    cases = {"gap_runs": te.sg_gap_run_cases, "staircases": te.sg_staircase_cases, "corners": te.sg_corner_cases,
             "wave_edge_ends": te.sg_wave_edge_end_cases, "ties": te.sg_tie_cases, "pad": te.sg_pad_cases}[group]()
    for case in cases:
        _sg_both_modes(gpu, case.a, case.b, case.sm, case.gap, sgoracle.align(case.a, case.b, case.sm, case.gap), repr(case))


@pytest.mark.parametrize("group", ["insertions", "ties"])
def test_local_constructed_edges(gpu, loracle, group):
    cases = te.local_insertion_cases() if group == "insertions" else te.local_tie_cases()
    for case in cases:
        _local_both_modes(gpu, case.a, case.b, case.sm, case.gap, loracle.align(case.a, case.b, case.sm, case.gap), repr(case))


def test_sgfull_extremes_at_16384(gpu, sgoracle):
    """all +127 with gap 0 (the highest H), all -128 with gap 127 (the lowest), +127 / -128 with gap 127; an identical, a
    shifted and a random pair each"""
    for case in te.sg_extreme_cases():
        want = sgoracle.align(case.a, case.b, case.sm, case.gap)
        _sg_both_modes(gpu, case.a, case.b, case.sm, case.gap, want, repr(case))
        if case.name == "extreme/all+127/0":
            assert (want[0] == 127 * 16384).all() and (want[1] == 16384).all()
        if case.name == "extreme/all-128/127":
            assert (want[0] == 0).all() and (want[1] == 0).all() and (want[3] == 1).all()


def test_local_extremes_at_16384(gpu, loracle):
    for case in te.local_extreme_cases():
        want = loracle.align(case.a, case.b, case.sm, case.gap)
        _local_both_modes(gpu, case.a, case.b, case.sm, case.gap, want, repr(case))
        if case.name == "local_extreme/all+127/0":
            assert (want[0] == 16256).all() and (want[1][:, :2] == 128).all()
        if case.name == "local_extreme/all-128/127":
            assert (want[0] == 0).all() and (want[1] == 0).all() and (want[3] == 0).all()


def test_bytes_0_to_255_through_both_host_entries(gpu, sgoracle, loracle):
    """bases are taken modulo 4: any byte gives what its low two bits give, on the GPU and in the restatements"""
    rng = np.random.default_rng(255)
    a = rng.integers(0, 256, (24, 1500), dtype=np.uint8)
    b = rng.integers(0, 256, (24, 1100), dtype=np.uint8)
    b[::2, :1000] = (a[::2, :1000] & 3) | (rng.integers(0, 64, (12, 1000), dtype=np.uint8) << 2)   # same bases, other bytes
    for name, sm, gap in te.SG_PARAMS:
        want = sgoracle.align(a & 3, b & 3, sm, gap)
        got = gpu.semiglobal_full(a, b, sm, gap)
        te.assert_same(got, want, ("bytes", name), "sgfull")
        te.assert_same(got, gpu.semiglobal_full(a & 3, b & 3, sm, gap), ("bytes vs & 3", name), "sgfull")
    la = rng.integers(0, 256, (40, 700), dtype=np.uint8)
    lb = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    la[::2, 300:428] = (lb[::2] & 3) | 0xF0
    for name, sm, gap in te.LOCAL_PARAMS:
        want = loracle.align(la & 3, lb & 3, sm, gap)
        got = gpu.local_align(la, lb, sm, gap)
        te.assert_same(got, want, ("bytes", name), "local")
        te.assert_same(got, gpu.local_align(la & 3, lb & 3, sm, gap), ("bytes vs & 3", name), "local")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def test_device_entries_on_one_stream(gpu, sgoracle, loracle):
    """swmi_semiglobal_full_device and swmi_local_align_device on torch buffers and one stream, for the gap runs, the corner
    exits, the ties and the pad cases"""
    stream = torch.cuda.Stream(device="cuda:0")
    for case in te.sg_gap_run_cases()[:2] + te.sg_corner_cases() + te.sg_tie_cases()[:3] + te.sg_pad_cases()[2:4]:
        n, (len1, len2) = len(case.a), case.shape
        mw = gpu.semiglobal_full_move_words(len1, len2)
        a, b = _dev(case.a), _dev(case.b)
        sc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ends = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
        mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda:0")
        ln = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()                        # the buffers were filled on the default stream
        gpu.semiglobal_full_device(a.data_ptr(), len1, b.data_ptr(), len2, n, case.sm, case.gap, sc.data_ptr(), ends.data_ptr(),
                                   mv.data_ptr(), ln.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got = (sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32))
        te.assert_same(got, sgoracle.align(case.a, case.b, case.sm, case.gap), ("device", repr(case)), "sgfull")
    for case in te.local_insertion_cases()[:2] + te.local_tie_cases()[:2]:
        n, len1 = case.a.shape
        mw = gpu.local_move_words(len1)
        a, b = _dev(case.a), _dev(case.b)
        sc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ends = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda:0")
        st = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        gpu.local_align_device(a.data_ptr(), len1, b.data_ptr(), n, case.sm, case.gap, sc.data_ptr(), ends.data_ptr(), mv.data_ptr(),
                               st.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got = (sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32))
        te.assert_same(got, loracle.align(case.a, case.b, case.sm, case.gap), ("device", repr(case)), "local")
