// global_full_kernels.hip -- gfx950 kernel of the global and free-end-gap aligner for two sequences of any length, with
// end cell, start cell and traceback (swmi_global_full*).
//
// Semantics (include/swmi.h): with free_ends a mask of kFreeBegin1 / kFreeBegin2 / kFreeEnd1 / kFreeEnd2,
//     H(0,0) = 0, H(i,0) = kFreeBegin1 ? 0 : -i gap, H(0,j) = kFreeBegin2 ? 0 : -j gap,
//     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)      (no zero floor)
// for i = 1..len1, j = 1..len2.  The end cell is (len1, len2), with kFreeEnd1 also any (i, len2), i = 0..len1, with kFreeEnd2
// also any (len1, j), j = 0..len2: the largest H, among equal ones the first in row-major order.  The walk goes back from
// it, diagonal before up before left; on row 0 (column 0) it ends if kFreeBegin2 (kFreeBegin1) is set and else goes on to
// (0, 0) by forced moves.  Mask 0 is Needleman-Wunsch.
//
// Mapping, ring timing, code layout, staged walk and the end rule (best cell, biased reduction, the walk's end): tile_sweep.h.
// This file holds the recurrence and the borders.
//
// The cell as KEYS is sgfull_kernels.hip's: key = H << 6 | 3 << 4 | (15 - jj), the candidates one add each from the
// neighbours' keys with tags 3 / 2 / 1 = diagonal / up / left, one v_max3_i32 and one v_and_or_b32 per cell.
// |H| <= 128 * 32768 = 2^22 and the bound is never met, so H << 6 fits.  A free border is a border of gap 0: its keys are
// those of H = 0, and the variant keeps one gap per border.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128.  What they compute flows only
// right and down, into other such columns, so no valid cell depends on one; the end rule reads the last column from the
// lane and register that hold column len2 and masks columns past len2 out of the last row, so it never picks one; the walk
// only moves up and left from a valid cell, so it never enters one.
//
// Codes: 2 bits per cell, one dword per lane and row, column jj at bits 2 jj: the move itself (3 / 2 / 1).  A staging block
// of the walk is 128 rows x 64 lanes (1024 columns).
#include "global_full_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds and code word were written against (tile_sweep.h owns it; a change there must revisit them)
namespace written_for {
constexpr int kCols = 16;
constexpr int kMaxWaves = 16;
constexpr int kUnroll = 4;
constexpr int kChunk = 32;
constexpr int kDelay = 3;
constexpr int kRing = 256;
constexpr int kStageRows = 128;
static_assert(kCols == tile::kCols && kMaxWaves == tile::kMaxWaves && kUnroll == tile::kUnroll && kChunk == tile::kChunk &&
              kDelay == tile::kDelay && kRing == tile::kRing && kStageRows == tile::kStageRows);
}  // namespace written_for

// free_ends is an argument, not a template parameter: it is uniform, stays in SGPRs, and one pair of kernels serves all 16 masks.
// RAGGED: one TileWork per workgroup (work[blockIdx.x]) names the alignment, and the launch's own shape (fixed_*, move_words)
// is unused; else `work` is NULL and unread (tile_sweep.h).  The mask and the gap stay the launch's: one call has one of each.
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void global_full_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                      int fixed_len1, int fixed_len2, SmCols cols, int gap,
                                                                      unsigned free_ends, int32_t *__restrict__ scores,
                                                                      int32_t *__restrict__ ends, uint32_t *__restrict__ codes,
                                                                      unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts,
                                                                      uint32_t move_words, uint32_t fixed_trips,
                                                                      const TileWork *__restrict__ work)
{
    using V = GlobalLinear;
    const V::Gaps gaps{gap, free_ends};
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_body.inc"
}

}  // namespace

size_t global_full_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_global_full(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              unsigned free_ends, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                              uint32_t *d_steps, size_t move_words, hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch<global_full_kernel<true>, global_full_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes,
                                                                             d_moves, d_steps, move_words, stream, gap, free_ends);
}

int global_full_ragged_waves(int len1, int len2) { return len1 > 0 && len2 > 0 ? tile::waves(len2) : 1; }

hipError_t launch_global_full_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                     const int8_t *sm, int gap, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch_ragged<global_full_kernel<true, true>, global_full_kernel<false, true>>(
        d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores, d_ends, d_codes, d_moves, d_steps, stream, gap, free_ends);
}

}  // namespace swmi
