// local_long_affine_kernels.hip -- gfx950 kernel of the local aligner with AFFINE gaps for two sequences of up to 65536 bases,
// with end cell, start cell and traceback (swmi_local_long_affine*).
//
// Semantics: local_full_affine_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 18 and 25); the variant is
// that file's (local_full_affine_variant.h).  Mapping: local_long_kernels.hip's column stripes, with the affine body's (H, F)
// pairs in the carry (len1 int2 per alignment): F runs along the row, so a gap that opens left of a stripe's edge extends
// across it through the carry as it does through the ring between two waves; E runs down a column and stays with the lane.
// Wave 0's border in stripe 0 stays the constant key of H = 0 with F = -inf, and row 0's diag_in that key.
//
// Carry ordering and BARRIER INVARIANT: local_long_kernels.hip's argument, word for word.  Row i's (H, F) is read by wave 0 in
// chunk (i - 1) / 32 of a stripe and overwritten by wave 15 in chunk 45 + (i + 62) / 32 of the same stripe; the next stripe
// reads it behind the closing s_waitcnt vmcnt(0), the workgroup barrier and the agent-scope acquire fence.  Every wave
// executes total_chunks + 1 barriers in every stripe but the last and total_chunks in the last, total_chunks made of len1 and
// blockDim alone; the local variant's row maximum and the fold of the stripe's best cell lie on no path that holds a barrier.
// A wave with my_chunks = 0 folds (H 0, row 0, column 0).  The carry is written with vector stores (one 8-byte store per row)
// and read with per-lane vector loads, never through a scalar load.
//
// Best cell under stripes: local_long_kernels.hip's fold of the stripe's per-lane best into r with a 64-bit maximum; the pack
// (H desc, row asc, column asc) makes it the first cell in row-major order over all stripes.
//
// Key range.  0 <= H <= 127 * 65536 = 8 323 072 < 2^23.  Every computed E and F is rebuilt from H's open term in its own
// cell (E(i, j) >= H(i - 1, j) - open, F(i, j) >= H(i, j - 1) - open, with H >= 0), so it is at least -127, and at most H's
// bound.  Apart from the sentinel every key lies in (-2^14, 2^29 + 2^6), and every candidate (a key plus at most 128 << 6)
// below 2^30 in magnitude.  kMinusInf = -2^30 is
// strictly below every reachable key, so it still loses every max it should lose (E(1, j) and F(i, 1) always open, also
// F into a later stripe's lane 0, which is the carry's reachable F of column 16384 s); it is extended at most once before an
// open candidate replaces it: -2^30 - 127 * 64 > -2^31, no wrap.  That is local_full_affine_kernels.hip's argument with 2^23
// for 2^21: unchanged.  NO DOMAIN RULE is needed: every int8 matrix and gaps in [0, 127] are accepted at every shape up to
// 65536 x 65536.
//
// Columns past len2 occur in the last stripe only.  local_full_affine_kernels.hip's induction in row-major order holds over all
// stripes: a padded cell above 0 is at most some valid cell earlier in row-major order (every gap cost is >= 0, a padded
// diagonal costs 128), on the same or an earlier row, in this or an earlier stripe, and that cell wins the pack's comparison.
// Padded columns feed only padded columns, never the carry, and the walk never enters one.
#include "local_full_affine_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void local_long_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int len1, int len2, SmCols cols, int gap_open, int gap_extend,
    int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, uint32_t move_words, uint32_t n_trips, int2 *carry_hf)
{
    using V = LocalAffine;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED
#include "tile_sweep_affine_body.inc"
}

}  // namespace

size_t local_long_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_local_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                    int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, size_t move_words, int32_t *d_carry,
                                    hipStream_t stream)
{
    return tile::launch_striped<local_long_affine_kernel<true>, local_long_affine_kernel<false>>(
        d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_steps, move_words, reinterpret_cast<int2 *>(d_carry),
        stream, gap_open, gap_extend);
}

}  // namespace swmi
