"""The long semi-global aligner (swmi_semiglobal_long*) on the GPU, every field bit-exact against the C restatement
tests/native/sgfull_oracle.c, compiled unchanged (it takes any lengths), with a traceback and ends-only.  The kernel sweeps len2
in stripes of 16384 columns (16 wavefronts of 1024) and folds each stripe's best cell into the first one in row-major order.  A
semi-global path pays for its leading gap, so the pairs are built to reach the later stripes (semiglobal_long_support.py), and
each check asserts on the restatement's result that they do.  Moves are compared up to `lengths - 1`; words past that are
unspecified."""
import pytest

import semiglobal_long_support as S

pytestmark = pytest.mark.gpu

FAM = S.Family(affine=False)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return FAM.oracle(tmp_path_factory.mktemp("semiglobal_long_oracle"))


# ---- 1. stripe edges on len2, paths that reach the later stripes ------------------------------------------------------------

@pytest.mark.parametrize("len1", S.LEN1S)
@pytest.mark.parametrize("len2", S.LEN2S)
def test_stripe_edges(gpu, oracle, len2, len1):
    S.check_stripe_edges(FAM, gpu, oracle, len2, len1)


# ---- 2., 3. a positive gap across the first boundary; both lengths beyond 32768 ---------------------------------------------

@pytest.mark.parametrize("which", range(len(S.insertion_sets(FAM))))
def test_positive_gap_across_the_first_boundary(gpu, oracle, which):
    S.check_positive_gap_across_the_boundary(FAM, gpu, oracle, which)


def test_both_beyond_32768_with_a_positive_gap(gpu, oracle):
    S.check_both_beyond_32768(FAM, gpu, oracle)


# ---- 4. long seq1, one stripe ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(16385, 17), (65536, 1025), (40000, 1024)])
def test_long_seq1_one_stripe(gpu, oracle, len1, len2):
    S.check_long_seq1(FAM, gpu, oracle, len1, len2)


# ---- 5. hand-built -----------------------------------------------------------------------------------------------------------

def test_tie_between_stripes_goes_to_the_smaller_row_in_the_later_stripe(gpu, oracle):
    S.check_tie_between_stripes(FAM, gpu, oracle)


def test_tie_on_one_row_goes_to_the_earlier_column(gpu, oracle):
    S.check_tie_on_one_row(FAM, gpu, oracle)


@pytest.mark.parametrize("column", [16384, 16385])
def test_best_cell_exactly_on_the_boundary(gpu, oracle, column):
    S.check_best_cell_on_column(FAM, gpu, oracle, column)


def test_forced_walk_along_row_0_across_two_boundaries(gpu, oracle):
    S.check_forced_walk_along_row_0(FAM, gpu, oracle)


def test_all_mismatch(gpu, oracle):
    S.check_all_mismatch(FAM, gpu, oracle)


@pytest.mark.parametrize("len2", [16385, 32769])
def test_last_stripe_of_one_column(gpu, oracle, len2):
    S.check_best_cell_on_column(FAM, gpu, oracle, len2, len2=len2)


def test_walk_whose_staging_blocks_straddle_the_boundary(gpu, oracle):
    S.check_walk_straddles_the_boundary(FAM, gpu, oracle)


def test_bytes_0_to_255(gpu, oracle):
    S.check_bytes_0_to_255(FAM, gpu, oracle)


# ---- 6. 65536 x 65536 in closed form: the edge of the domain, and the unit costs ---------------------------------------------

@pytest.mark.parametrize("match,gap", [(64, 64), (1, 1)])
def test_full_size_closed_forms(gpu, match, gap):
    S.check_full_size(FAM, gpu, match, gap)


# ---- 7. ties to other entries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(300, 16384), (16384, 300), (1000, 5000)])
def test_equals_the_fixed_entry_where_both_reach(gpu, len1, len2):
    S.check_equals_fixed(FAM, gpu, len1, len2)


@pytest.mark.parametrize("name", ["insertion", "both_long"])
def test_global_long_on_the_prefixes_gives_the_same_score(gpu, oracle, name):
    sm, gaps = S.insertion_sets(FAM)[0] if name == "insertion" else S.both_long_set(FAM)
    S.check_global_witness(FAM, gpu, oracle, name, sm, gaps)


# ---- 8. the host entry with the expander, the device entry, the C++ overloads -------------------------------------------------

def test_host_entry_and_expand_moves(gpu, oracle):
    S.check_host_entry_and_expand(FAM, gpu, oracle)


def test_device_entry_on_resident_buffers(gpu, oracle):
    S.check_device_entry(FAM, gpu, oracle)


def test_cpp_overloads(gpu, oracle, tmp_path):
    S.check_cpp_overloads(FAM, gpu, oracle, tmp_path)
