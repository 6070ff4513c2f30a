// local_long_kernels.hip -- gfx950 kernel of the local aligner for two sequences of up to 65536 bases, with end cell, start
// cell and traceback (swmi_local_long*).
//
// Semantics: local_full_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 17 and 25): the same recurrence, zero
// floor, best-cell rule (the first cell in row-major order holding max H) and walk (it stops on the first cell holding 0);
// the variant is that file's (local_full_variant.h).
//
// Mapping (tile_sweep.h, and the stripe loop of tile_sweep_body.inc): global_long_kernels.hip's.  One workgroup per alignment,
// of at most 16 wavefronts; len2 > 16384 columns are swept as STRIPES of 16384, one after another over all of seq1.  Stripe s
// covers columns 16384 s + 1 .. min(16384 (s + 1), len2); inside a stripe the lane-to-lane hand-over, the LDS ring, the chunks
// and the delay are untouched.  Codes keep code_index's layout with G >> 6 the GLOBAL wave 0 .. 63, so the walk's staging block
// may straddle a stripe boundary and reads the right words there.
//
// The carry (len1 ints per alignment in device memory) holds the stored key of column 16384 (s + 1) of every row, which lane
// 63 of stripe s's wave 15 writes and lane 0 of stripe s + 1's wave 0 takes as its left column, as it would from the ring.
// Row 0's diag_in and wave 0's border in stripe 0 stay the variant's constant key of H = 0.  Ordering, as for the global
// kernels: row i is read by wave 0 in chunk (i - 1) / 32 of a stripe and overwritten by wave 15 in chunk 45 + (i + 62) / 32 of
// the SAME stripe, 45 barriers after its value was consumed; it is read again only in the next stripe, behind the closing
// s_waitcnt vmcnt(0) (the writer's stores have reached L2), the workgroup barrier (every wave has passed that drain and its
// last ring read) and the agent-scope acquire fence (the next stripe's loads miss this CU's L1, which may hold the rows as
// the previous stripe left them).  The carry is written with vector stores and read with per-lane vector loads (carry_row,
// tile_sweep.h), never through a scalar load.  None of this depends on what an entry holds, so the local variant adds nothing.
//
// BARRIER INVARIANT: every wave of the workgroup executes total_chunks + 1 barriers in every stripe but the last and
// total_chunks in the last, with total_chunks = ceil((len1 + 63) / 32) + 3 (W - 1) made of len1 and blockDim alone.  The local
// variant's work -- the row maximum, the fold of the stripe's best cell -- lies inside a chunk's work or between the sweep and
// the closing barrier, on no path that holds a barrier, and `more_stripes` is uniform.  A wave with no column in the last
// stripe (my_chunks = 0) skips the chunks' work, not their barriers, and folds the candidate (H 0, row 0, column 0), which
// every other candidate ties or beats and which is the answer when no cell is above 0.  With len2 <= 16384 (a long seq1
// alone) there is one stripe, W = waves(len2) and the carry is never touched (it may be NULL).
//
// Best cell under stripes.  Each lane keeps `best` and `best_row` per stripe (first row with the strictly largest H among its
// 16 columns of that stripe, the key's low bits naming the first such column) and after the stripe folds
//     H << 34 | (0x1FFFF - row) << 17 | (0x1FFFF - col),      col = the lane's GLOBAL jbase + jj + 1
// into r with a 64-bit maximum.  The pack orders H descending, then row ascending, then column ascending; the maximum over all
// lanes and all stripes is therefore the first cell in row-major order holding max H, whichever stripe it lies in.  It is not
// "the earlier stripe wins": a later stripe's cell in a lower row beats an equal cell of stripe 0.
//
// Key range.  0 <= H <= 127 * 65536 = 8 323 072 < 2^23, so a stored key H << 6 | tag << 4 | low is positive and below
// 2^29 + 2^6; every candidate is a key plus (score or -gap) << 6 and a tag difference, |.| <= 128 * 64 + 48, so every candidate
// lies below 2^30 in magnitude and nothing wraps.  H < 2^23 fits the pack's 30 bits above bit 34, and its 17-bit fields hold
// 65536.  NO DOMAIN RULE is needed: the floor bounds H from below whatever the matrix and the gap, so every int8 matrix and
// gap is accepted at every shape up to 65536 x 65536.
//
// Columns past len2 are computed with every score -128; they occur in the LAST stripe only (every earlier stripe is full),
// in the last lanes of the wave that holds column len2 (later waves skip the stripe).  local_full_kernels.hip's induction
// over the cells in row-major order carries over with "cell" read over all stripes: a padded cell holds 0, or its diagonal
// candidate (a cell of the row above minus 128), or its up candidate (a padded cell of the row above minus gap >= 0), or its
// left candidate (the row's last valid cell or a padded cell left of it, minus gap >= 0); so a padded cell above 0 is at most
// some valid cell EARLIER in row-major order -- on the same row left of it or on an earlier row, in the last stripe or in an
// earlier one.  That valid cell has H at least as large, and a smaller row or the same row and a smaller column, so it wins
// the pack's comparison against the padded cell whichever stripe folded it: the reduction never picks a padded cell.  What
// padded columns compute flows only right and down into other padded columns -- never into the carry, which only full stripes
// write -- and the walk only moves up and left from a valid cell.
//
// Indices at 65536 x 65536: trips(len1) = 16400, code_words = 64 * 16400 * 256 = 268 697 600 per alignment (size_t sums, times
// the alignment index); the carry index k * len1 is a size_t; a walk is at most 131072 steps.
#include "local_full_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void local_long_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                     int len1, int len2, SmCols cols, int gap,
                                                                     int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                                                                     uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves,
                                                                     uint32_t *__restrict__ counts, uint32_t move_words, uint32_t n_trips,
                                                                     int *carry)
{
    using V = LocalLinear;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED
    const V::Gaps gaps{gap};
#include "tile_sweep_body.inc"
}

}  // namespace

size_t local_long_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_local_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                             int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                             size_t move_words, int32_t *d_carry, hipStream_t stream)
{
    return tile::launch_striped<local_long_kernel<true>, local_long_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends,
                                                                                   d_codes, d_moves, d_steps, move_words, d_carry, stream,
                                                                                   gap);
}

}  // namespace swmi
