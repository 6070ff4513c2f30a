// global_long_affine_kernels.hip -- gfx950 kernel of the global and free-end-gap aligner with AFFINE gaps for two sequences of up
// to 65536 bases, with end cell, start cell and traceback (swmi_global_long_affine*).
//
// Semantics: global_full_affine_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 21 and 23); the variant is
// that file's (global_full_affine_variant.h).  Mapping: global_long_kernels.hip's column stripes, with the affine body's
// (H, F) pairs in the carry (len1 int2 per alignment): F runs along the row, so a gap that opens left of a stripe's edge
// extends across it through the carry as it does through the ring between two waves.
//
// Key range.  The host accepts a call iff P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gap_open, gap_extend) (swmi.h).
// Every cell of a gap costs at most P and every diagonal at most P in magnitude, so H, and E and F where they are reachable,
// lie within 2^23 of 0 in every valid cell, with every mask (a free border only moves border values toward 0).  A padded
// column (j > len2, scored -128 whatever P is; at most 1023 of them, in the last stripe) has H >= F >= H(i, j - 1) - open, so
// it loses at most 127 per column: value > -2^23 - 2^17.  A lane computes no row past its border (rows outside 1 .. len1
// are skipped; the border's closed form for up to 95 such rows stays below (65536 + 95) * 127 < 2^23).  So |value << 6| <
// 2^29 + 2^23 for every reachable value: strictly above kMinusInf = -2^30, which therefore still loses every max it should
// lose (E(1, j) and F(i, 1) always open).  E and F are rebuilt from H's open term in every cell, so -inf never decays by more
// than one extend along a column or a row before a reachable value replaces it: -2^30 - 127 * 64 > -2^31, no wrap.  The
// reduction's bias is kEndBias = 2^24 > 2^23; H + 2^24 < 2^25 fits end_pack's 30 bits.
#include "global_full_affine_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void global_long_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int len1, int len2, SmCols cols, int gap_open, int gap_extend,
    unsigned free_ends, int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, uint32_t move_words, uint32_t n_trips, int2 *carry_hf)
{
    using V = GlobalAffine;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED and tile::kEndBias
    constexpr int kEndBias = 1 << 24;
#include "tile_sweep_affine_body.inc"
}

}  // namespace

size_t global_long_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_global_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_steps, size_t move_words,
                                     int32_t *d_carry, hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch_striped<global_long_affine_kernel<true>, global_long_affine_kernel<false>>(
        d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_steps, move_words, reinterpret_cast<int2 *>(d_carry),
        stream, gap_open, gap_extend, free_ends);
}

}  // namespace swmi
