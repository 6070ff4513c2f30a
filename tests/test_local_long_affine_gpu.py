"""The long local aligner with affine gaps (swmi_local_long_affine*) on the GPU, every field bit-exact against the C restatement
tests/native/local_full_affine_oracle.c, compiled unchanged (it takes any lengths).  The kernel sweeps len2 in stripes of 16384
columns (16 wavefronts of 1024) and folds each stripe's best cell into the first one in row-major order; the shapes sit at the
stripe's and the wavefront's edges, the planted pairs' paths cross them, and the hand-built pairs put equal cells into
different stripes (those at open == extend, the linear recurrence); gaps open at, beside and across the boundary, where F
rides in the carry.  Moves are compared up to `steps`; words past it are unspecified."""
import numpy as np
import pytest

import local_long_support as S
from conftest import match_matrix

pytestmark = pytest.mark.gpu

FAM = S.Family(affine=True)
DIAG, LEFT = S.DIAG, S.LEFT


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    return FAM.oracle(tmp_path_factory.mktemp("local_long_affine_oracle"))


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
    S.check_both_long(FAM, gpu, oracle, match_matrix(5, -4), (6, 2))


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


# ---- 4b. affine only: gaps at the boundary ---------------------------------------------------------------------------------

def _with_insert(first, half, k, seed):
    """seq1 = 2 * half bases over {0, 1}; seq2 over {2, 3} holds its first half ending at column first - 1, k foreign bases
    from column `first` on, then its second half."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, 2 * half, dtype=np.uint8)
    b = np.concatenate([rng.integers(2, 4, first - 1 - half, dtype=np.uint8), s[:half], rng.integers(2, 4, k, dtype=np.uint8), s[half:],
                        rng.integers(2, 4, 64, dtype=np.uint8)])
    return s, b


@pytest.mark.parametrize("first", [16384, 16385])
@pytest.mark.parametrize("go,ge", [(7, 2), (2, 7)])
def test_gap_that_opens_at_the_boundary(gpu, oracle, first, go, ge):
    """A 3-base insert in seq2 whose first column is 16384 -- the gap opens in stripe 0 and extends into stripe 1, F carried --
    or 16385 -- it opens in stripe 1 from the carried H.  The values are the restatement's; the path is 40 diagonals, 3 left
    moves, 40 diagonals, and the score 80 * 5 less open + 2 min(open, extend): where open < extend every left step opens anew."""
    s, b = _with_insert(first, 40, 3, first)
    score, ends, codes = FAM.one(gpu, oracle, s, b, match_matrix(5, -4), (go, ge), ("gap at", first, go, ge))
    assert score == 400 - go - 2 * min(go, ge) and ends == [80, first + 42, 0, first - 41]
    assert codes == [DIAG] * 40 + [LEFT] * 3 + [DIAG] * 40


@pytest.mark.parametrize("go,ge", [(9, 2), (9, 0)])
def test_long_gap_across_the_boundary(gpu, oracle, go, ge):
    """A 200-base insert over columns 16285 .. 16484, open > extend and extend = 0: 200 diagonals, one left run of 200 across
    column 16384, 200 diagonals; the values are the restatement's."""
    s, b = _with_insert(16285, 200, 200, 77)
    score, ends, codes = FAM.one(gpu, oracle, s, b, match_matrix(5, -4), (go, ge), ("long gap", go, ge))
    assert score == 2000 - go - 199 * ge and ends == [400, 16684, 0, 16084]
    assert codes == [DIAG] * 200 + [LEFT] * 200 + [DIAG] * 200


# ---- 5. 65536 x 65536: the top of the key range ----------------------------------------------------------------------------

@pytest.mark.parametrize("match,go,ge", [(1, 3, 1), (127, 127, 127)])
def test_full_size_identical_sequences(gpu, match, go, ge):
    S.check_full_size_identical(FAM, gpu, match, (go, ge))


# ---- 6. ties to the fixed-length entry -------------------------------------------------------------------------------------

@pytest.mark.parametrize("len1,len2", [(300, 16384), (16384, 300), (1000, 5000)])
def test_equals_the_fixed_entry_where_both_reach(gpu, len1, len2):
    S.check_equals_fixed(FAM, gpu, len1, len2)


# ---- 7. open == extend is the linear entry ---------------------------------------------------------------------------------

def test_open_equal_to_extend_is_the_linear_entry(gpu):
    """(129, 17409): with gap_open == gap_extend == g every field equals swmi_local_long's with gap g."""
    a, b = S.local_batch(129, 17409, 55)
    for sm, (g,) in S.Family(affine=False).params:
        S.assert_same(gpu.local_long.local_long_affine(a, b, sm, g, g), gpu.local_long.local_long(a, b, sm, g), ("open == extend", g))


# ---- 8., 9., 10. the host entry with the expander, the device entry, the C++ overloads -------------------------------------

def test_host_entry_and_expand_moves(gpu, oracle):
    S.check_host_entry_and_expand(FAM, gpu, oracle, match_matrix(5, -4), (6, 2))


def test_device_entry_on_resident_buffers(gpu, oracle):
    S.check_device_entry(FAM, gpu, oracle, match_matrix(1, -1), (3, 1))


def test_cpp_overloads(gpu, oracle, tmp_path):
    S.check_cpp_overloads(FAM, gpu, oracle, tmp_path)
