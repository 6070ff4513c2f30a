// global_long_kernels.hip -- gfx950 kernel of the global and free-end-gap aligner for two sequences of up to 65536 bases, with
// end cell, start cell and traceback (swmi_global_long*).
//
// Semantics: global_full_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 20 and 23): the same recurrence,
// mask, end-cell rule, tie order and walk; the variant is that file's (global_full_variant.h).
//
// Mapping (tile_sweep.h, and the stripe loop of tile_sweep_body.inc): one workgroup per alignment as there, of at most 16
// wavefronts; len2 > 16384 columns are swept as STRIPES of 16384, one after another over all of seq1.  Stripe s covers columns
// 16384 s + 1 .. min(16384 (s + 1), len2); inside a stripe the lane-to-lane hand-over, the LDS ring, the chunks and the delay
// are untouched.  Wave 0's lane 0 takes its left column from the per-alignment `carry` (len1 ints in device memory), which
// lane 63 of the previous stripe's wave 15 wrote; the body gives the ordering argument and the barrier invariant.  Codes
// keep code_index's layout with G >> 6 the GLOBAL wave 0 .. 63, so the walk's staging block may straddle a stripe boundary
// and reads the right words there.
//
// Key range.  The host accepts a call iff P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gap) (swmi.h).  A path to a valid
// cell (i, j) makes at most i + j <= len1 + len2 moves, each worth at most P in magnitude (a diagonal covers two of i + j), and a
// free border only moves border values toward 0, so |H| <= 2^23 in every valid cell.  A padded column (j > len2, scored -128
// whatever P is) lies at most 1023 columns right of column len2, in the last stripe only; its H is at most the largest H
// of the cells it derives from (every score and gap only lowers it) and at least H(i, j - 1) - gap, so H >= -2^23 - 1023 * 127 >
// -2^23 - 2^17.  A lane computes no row past its border: rows outside 1 .. len1 are skipped, and the left border's closed
// form, evaluated for up to 95 such rows, is at most (65536 + 95) * 127 < 2^23 in magnitude.  So every key H << 6 has
// |H << 6| < 2^29 + 2^23, every candidate (a key plus a score or a gap, << 6) stays below 2^30 in magnitude, and nothing wraps.
// The reduction's bias must exceed the largest |H| of a valid cell: kEndBias = 2^24 here, and H + 2^24 < 2^25 fits the 30 bits
// that end_pack leaves above its 17-bit row and column fields (which hold 65536).
//
// Indices at 65536 x 65536: trips(len1) = 16400, code_words = 64 * 16400 * 256 = 268 697 600 per alignment (size_t sums, times
// the alignment index); the carry index k * len1 is a size_t; a walk is at most 131072 steps.
#include "global_full_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void global_long_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                      int len1, int len2, SmCols cols, int gap, unsigned free_ends,
                                                                      int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                                                                      uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves,
                                                                      uint32_t *__restrict__ counts, uint32_t move_words, uint32_t n_trips,
                                                                      int *carry)
{
    using V = GlobalLinear;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED and tile::kEndBias
    constexpr int kEndBias = 1 << 24;
    const V::Gaps gaps{gap, free_ends};
#include "tile_sweep_body.inc"
}

}  // namespace

size_t global_long_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_global_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              unsigned free_ends, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                              uint32_t *d_steps, size_t move_words, int32_t *d_carry, hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch_striped<global_long_kernel<true>, global_long_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends,
                                                                                     d_codes, d_moves, d_steps, move_words, d_carry,
                                                                                     stream, gap, free_ends);
}

}  // namespace swmi
