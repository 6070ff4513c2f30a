"""The long local aligner (swmi_local_long*) on the GPU, every field bit-exact against the C restatement
tests/native/local_full_oracle.c, compiled unchanged (it takes any lengths).  The kernel sweeps len2 in stripes of 16384
columns (16 wavefronts of 1024) and folds each stripe's best cell into the first one in row-major order; the shapes sit at the
stripe's and the wavefront's edges, the planted pairs' paths cross them, and the hand-built pairs put equal cells into
different stripes.  Moves are compared up to `steps`; words past it are unspecified."""
import pytest

import local_long_support as S
from conftest import match_matrix

pytestmark = pytest.mark.gpu

FAM = S.Family(affine=False)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return FAM.oracle(tmp_path_factory.mktemp("local_long_oracle"))


# ---- 1. stripe edges on len2 ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1", S.LEN1S)
@pytest.mark.parametrize("len2", S.LEN2S)
def test_stripe_edges(gpu, oracle, len2, len1):
    S.check_stripe_edges(FAM, gpu, oracle, len2, len1)


# ---- 2., 3. long seq1 in one stripe; both long -----------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(16385, 17), (65536, 1025), (40000, 1024)])
def test_long_seq1_one_stripe(gpu, oracle, len1, len2):
    S.check_long_seq1(FAM, gpu, oracle, len1, len2)


def test_both_long(gpu, oracle):
    S.check_both_long(FAM, gpu, oracle, match_matrix(5, -4), (3,))


# ---- 4. hand-built ---------------------------------------------------------------------------------------------------------

def test_tie_between_stripes_goes_to_the_lower_row_in_the_later_stripe(gpu, oracle):
    S.check_tie_lower_row_in_the_later_stripe(FAM, gpu, oracle)


@pytest.mark.parametrize("gap", [2, 0])
def test_tie_on_one_row_goes_to_the_earlier_column(gpu, oracle, gap):
    S.check_tie_on_one_row(FAM, gpu, oracle, gap)


@pytest.mark.parametrize("first", [16384, 16385])
def test_start_exactly_at_the_boundary(gpu, oracle, first):
    S.check_start_at_the_boundary(FAM, gpu, oracle, first)


def test_left_run_across_the_boundary(gpu, oracle):
    S.check_left_run_across_the_boundary(FAM, gpu, oracle)


def test_up_run_in_stripe_1(gpu, oracle):
    S.check_up_run_in_stripe_1(FAM, gpu, oracle)


def test_all_mismatch(gpu, oracle):
    S.check_all_mismatch(FAM, gpu, oracle)


@pytest.mark.parametrize("len2", [16385, 17409])
def test_last_stripe_of_one_column(gpu, oracle, len2):
    S.check_last_stripe_of_one_column(FAM, gpu, oracle, len2)


def test_walk_whose_staging_blocks_straddle_the_boundary(gpu, oracle):
    S.check_walk_straddles_the_boundary(FAM, gpu, oracle)


def test_bytes_0_to_255(gpu, oracle):
    S.check_bytes_0_to_255(FAM, gpu, oracle)


# ---- 5. 65536 x 65536: the top of the key range ----------------------------------------------------------------------------

@pytest.mark.parametrize("match,gap", [(1, 1), (127, 127)])
def test_full_size_identical_sequences(gpu, match, gap):
    S.check_full_size_identical(FAM, gpu, match, (gap,))


# ---- 6. ties to the fixed-length entry -------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(300, 16384), (16384, 300), (1000, 5000)])
def test_equals_the_fixed_entry_where_both_reach(gpu, len1, len2):
    S.check_equals_fixed(FAM, gpu, len1, len2)


# ---- 8., 9., 10. the host entry with the expander, the device entry, the C++ overloads -------------------------------------

def test_host_entry_and_expand_moves(gpu, oracle):
    S.check_host_entry_and_expand(FAM, gpu, oracle, match_matrix(5, -4), (3,))


def test_device_entry_on_resident_buffers(gpu, oracle):
    S.check_device_entry(FAM, gpu, oracle, match_matrix(1, -1), (1,))


def test_cpp_overloads(gpu, oracle, tmp_path):
    S.check_cpp_overloads(FAM, gpu, oracle, tmp_path)
