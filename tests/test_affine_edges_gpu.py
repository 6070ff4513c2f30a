"""The affine table aligners (swmi_local_align_affine*, swmi_semiglobal_full_affine*) on the GPU at the edges of their
mappings: shape grids derived from the affine kernels' constants over the three gap families, single gap runs that extend
across wave and lane boundaries and leave staging blocks inside the gap, exits on the opening move and through the corner,
ties that only the tag order or the reduction order decides, the pad column with open = 0, the extremes of H, E and F, and
bytes 0..255.  Every field bit-exact against the C restatements, with a traceback and ends-only; affine_edges.py builds the
inputs and test_affine_edges_cpu.py checks, without a device, that each reaches the edge it claims."""
import numpy as np
import pytest
import torch

import affine_edges as ae
import table_edges as te
from local_affine_support import AffineOracle
from sgfull_affine_support import SgAffineOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgoracle(tmp_path_factory):
    return SgAffineOracle(tmp_path_factory.mktemp("sgfull_affine_oracle"))


@pytest.fixture(scope="module")
def loracle(tmp_path_factory):
    return AffineOracle(tmp_path_factory.mktemp("local_affine_oracle"))


def _sg_both_modes(gpu, a, b, sm, go, ge, want, what):
    te.assert_same(gpu.semiglobal_full_affine(a, b, sm, go, ge), want, what, "sgfull")
    sc, ends, _, _ = gpu.semiglobal_full_affine(a, b, sm, go, ge, traceback=False)
    te.assert_same((sc, ends, None, None), want, (what, "ends-only"), "sgfull", traceback=False)


def _local_both_modes(gpu, a, b, sm, go, ge, want, what):
    te.assert_same(gpu.local_align_affine(a, b, sm, go, ge), want, what, "local")
    sc, ends, _, _ = gpu.local_align_affine(a, b, sm, go, ge, traceback=False)
    te.assert_same((sc, ends[:, :2], None, None), (want[0], want[1][:, :2], None, None), (what, "ends-only"), "local", traceback=False)
    assert (ends[:, 2:] == -1).all(), what


def _sg_case(gpu, oracle, case):
    want = oracle.align(case.a, case.b, case.sm, case.gap_open, case.gap_extend)
    _sg_both_modes(gpu, case.a, case.b, case.sm, case.gap_open, case.gap_extend, want, repr(case))
    if case.linear_gap is not None:                     # open = extend: the linear entry computes the same thing
        te.assert_same(gpu.semiglobal_full(case.a, case.b, case.sm, case.linear_gap), want, ("linear entry", repr(case)), "sgfull")
    return want


def _local_case(gpu, oracle, case):
    want = oracle.align(case.a, case.b, case.sm, case.gap_open, case.gap_extend)
    _local_both_modes(gpu, case.a, case.b, case.sm, case.gap_open, case.gap_extend, want, repr(case))
    if case.linear_gap is not None:
        te.assert_same(gpu.local_align(case.a, case.b, case.sm, case.linear_gap), want, ("linear entry", repr(case)), "local")
    return want


@pytest.mark.parametrize("index,shape", list(enumerate(ae.sg_shape_grid())), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sgfull_affine_shape_grid(gpu, sgoracle, index, shape):
    len1, len2, n = shape
    for name, sm, go, ge in ae.grid_params(index):
        a, b = te.sg_mixed_pairs(n, len1, len2, len1 * 7919 + len2 + 16 * go + ge)
        _sg_both_modes(gpu, a, b, sm, go, ge, sgoracle.align(a, b, sm, go, ge), ("%dx%d n=%d W=%d" % (len1, len2, n, te.sg_waves(len2)), name))
    if len1 * len2 >= 1 << 27:
        gpu.semiglobal_full_affine_release_workspaces()


@pytest.mark.parametrize("index,shape", list(enumerate(ae.local_shape_grid())), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_local_affine_shape_grid(gpu, loracle, index, shape):
    len1, n = shape
    for name, sm, go, ge in ae.grid_params(index):
        a, b = te.local_mixed_pairs(n, len1, len1 * 131 + n + 16 * go + ge)
        _local_both_modes(gpu, a, b, sm, go, ge, loracle.align(a, b, sm, go, ge), ("len1=%d n=%d" % (len1, n), name))


@pytest.mark.parametrize("group", list(ae.SG_GROUPS))
def test_sgfull_affine_constructed_edges(gpu, sgoracle, group):
    """runs: left runs inside F across j = 1024 k, up runs inside E, blocks left inside the gap; extend0: one F along a row
    of 16 waves; staircases, corners, open_exits: every way out of a block, in every state; best_ties, pad: the reductions
    (also against the linear entry); path_ties: the tag order"""
    for case in ae.SG_GROUPS[group]():
        _sg_case(gpu, sgoracle, case)
    gpu.semiglobal_full_affine_release_workspaces()


@pytest.mark.parametrize("group", list(ae.LOCAL_GROUPS))
def test_local_affine_constructed_edges(gpu, loracle, group):
    for case in ae.LOCAL_GROUPS[group]():
        _local_case(gpu, loracle, case)


def test_local_affine_constructed_edges_through_the_ragged_entry(gpu, loracle):
    """every constructed local case once more through swmi_local_align_affine_ragged, the cases of one parameter set (of
    different len1) together in one call: the RAGGED instantiation shares the cell and the walk"""
    by_params = {}
    for make in ae.LOCAL_GROUPS.values():
        for case in make():
            by_params.setdefault((case.sm.tobytes(), case.gaps), []).append(case)
    assert any(len({c.shape[0] for c in cases}) > 1 for cases in by_params.values())
    for cases in by_params.values():
        c0 = cases[0]
        seq1s = [row for c in cases for row in c.a]
        seq2s = np.concatenate([c.b for c in cases])
        for traceback in (True, False):
            sc, ends, moves, mo, steps = gpu.local_align_affine_ragged(seq1s, seq2s, c0.sm, c0.gap_open, c0.gap_extend, traceback=traceback)
            at = 0
            for c in cases:
                n = len(c.a)
                want = loracle.align(c.a, c.b, c.sm, c.gap_open, c.gap_extend)
                what = ("ragged", repr(c), traceback)
                if traceback:
                    mv = np.zeros_like(want[2])
                    for k in range(n):
                        row = moves[int(mo[at + k]):int(mo[at + k + 1])][:mv.shape[1]]
                        mv[k, :len(row)] = row
                    te.assert_same((sc[at:at + n], ends[at:at + n], mv, steps[at:at + n]), want, what, "local")
                else:
                    te.assert_same((sc[at:at + n], ends[at:at + n, :2], None, None), (want[0], want[1][:, :2], None, None), what, "local",
                                   traceback=False)
                    assert (ends[at:at + n, 2:] == -1).all(), what
                at += n


def test_sgfull_affine_extremes_at_16384(gpu, sgoracle):
    """all +127 with (0, 0) (the highest H), all -128 with (127, 127), (127, 0), (0, 127) (the lowest H, E and F), +127 /
    -128 with (127, 0) and (0, 127); an identical, a shifted and a random pair each"""
    for case in ae.sg_extreme_cases():
        want = _sg_case(gpu, sgoracle, case)
        if case.name == "extreme/all+127/0,0":
            assert (want[0] == 127 * 16384).all() and (want[1] == 16384).all()
        if case.name.startswith("extreme/all-128"):
            assert (want[0] == 0).all() and (want[1] == 0).all() and (want[3] == 1).all()
    gpu.semiglobal_full_affine_release_workspaces()
    gpu.semiglobal_full_release_workspaces()


def test_local_affine_extremes_at_16384(gpu, loracle):
    for case in ae.local_extreme_cases():
        want = _local_case(gpu, loracle, case)
        if case.name == "local_extreme/all+127/0,0":
            assert (want[0] == 16256).all() and (want[1][:, :2] == 128).all()
        if case.name.startswith("local_extreme/all-128"):
            assert (want[0] == 0).all() and (want[1] == 0).all() and (want[3] == 0).all()


def test_bytes_0_to_255_through_both_affine_host_entries(gpu, sgoracle, loracle):
    """bases are taken modulo 4: any byte gives what its low two bits give, on the GPU and in the restatements"""
    rng = np.random.default_rng(2550)
    a = rng.integers(0, 256, (24, 1500), dtype=np.uint8)
    b = rng.integers(0, 256, (24, 1100), dtype=np.uint8)
    b[::2, :1000] = (a[::2, :1000] & 3) | (rng.integers(0, 64, (12, 1000), dtype=np.uint8) << 2)   # same bases, other bytes
    la = rng.integers(0, 256, (40, 700), dtype=np.uint8)
    lb = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    la[::2, 300:428] = (lb[::2] & 3) | 0xF0
    for name, sm, go, ge in ae.grid_params(0) + ae.grid_params(1)[2:]:
        want = sgoracle.align(a & 3, b & 3, sm, go, ge)
        got = gpu.semiglobal_full_affine(a, b, sm, go, ge)
        te.assert_same(got, want, ("bytes", name), "sgfull")
        te.assert_same(got, gpu.semiglobal_full_affine(a & 3, b & 3, sm, go, ge), ("bytes vs & 3", name), "sgfull")
        want = loracle.align(la & 3, lb & 3, sm, go, ge)
        got = gpu.local_align_affine(la, lb, sm, go, ge)
        te.assert_same(got, want, ("bytes", name), "local")
        te.assert_same(got, gpu.local_align_affine(la & 3, lb & 3, sm, go, ge), ("bytes vs & 3", name), "local")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def test_affine_device_entries_on_one_stream(gpu, sgoracle, loracle):
    """swmi_semiglobal_full_affine_device and swmi_local_align_affine_device on torch buffers and one non-default stream, for
    the long runs, the corner and opening-move exits, the ties and the pad cases"""
    stream = torch.cuda.Stream(device="cuda:0")
    sg_cases = (ae.sg_run_cases()[:5] + ae.sg_run_cases()[6:8] + ae.sg_corner_cases()[::3] + ae.sg_open_exit_cases() + ae.sg_best_tie_cases()[:2]
                + ae.sg_path_tie_cases() + ae.sg_pad_cases()[4:8])
    for case in sg_cases:
        n, (len1, len2) = len(case.a), case.shape
        mw = gpu.semiglobal_full_move_words(len1, len2)
        a, b = _dev(case.a), _dev(case.b)
        sc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ends = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
        mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda:0")
        ln = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()                        # the buffers were filled on the default stream
        gpu.semiglobal_full_affine_device(a.data_ptr(), len1, b.data_ptr(), len2, n, case.sm, case.gap_open, case.gap_extend,
                                          sc.data_ptr(), ends.data_ptr(), mv.data_ptr(), ln.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got = (sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), ln.cpu().numpy().view(np.uint32))
        te.assert_same(got, sgoracle.align(case.a, case.b, case.sm, case.gap_open, case.gap_extend), ("device", repr(case)), "sgfull")
    for case in ae.local_run_cases()[3:7] + ae.local_best_tie_cases()[:2] + ae.local_path_tie_cases():
        n, len1 = case.a.shape
        mw = gpu.local_move_words(len1)
        a, b = _dev(case.a), _dev(case.b)
        sc = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        ends = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        mv = torch.zeros((n, mw), dtype=torch.int64, device="cuda:0")
        st = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        gpu.local_align_affine_device(a.data_ptr(), len1, b.data_ptr(), n, case.sm, case.gap_open, case.gap_extend, sc.data_ptr(),
                                      ends.data_ptr(), mv.data_ptr(), st.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        got = (sc.cpu().numpy(), ends.cpu().numpy(), mv.cpu().numpy().view(np.uint64), st.cpu().numpy().view(np.uint32))
        te.assert_same(got, loracle.align(case.a, case.b, case.sm, case.gap_open, case.gap_extend), ("device", repr(case)), "local")
