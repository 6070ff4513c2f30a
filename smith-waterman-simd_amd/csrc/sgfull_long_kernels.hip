// sgfull_long_kernels.hip -- gfx950 kernel of the exact semi-global aligner for two sequences of up to 65536 bases, with best
// cell and traceback (swmi_semiglobal_long*).
//
// Semantics: sgfull_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 13 and 26): the same recurrence and charged
// borders, no zero floor, the same best cell (the first cell in row-major order over i = 0..len1, j = 0..len2 strictly above
// every earlier one, from 0 at (0, 0)), and the same walk back to (0, 0), forced on row 0 and column 0; the variant is that
// file's (sgfull_variant.h).
//
// Mapping (tile_sweep.h, and the stripe loop of tile_sweep_body.inc): global_long_kernels.hip's.  One workgroup per alignment,
// of at most 16 wavefronts; len2 > 16384 columns are swept as STRIPES of 16384, one after another over all of seq1.  Stripe s
// covers columns 16384 s + 1 .. min(16384 (s + 1), len2); inside a stripe the lane-to-lane hand-over, the LDS ring, the chunks
// and the delay are untouched.  A stripe sets up row 0 (H(0, j) = -j gap, from the lane's GLOBAL column j) and
// diag_in = H(0, 16 G) anew.  Codes keep code_index's layout with G >> 6 the GLOBAL wave 0 .. 63, so the walk's staging block
// may straddle a stripe boundary and reads the right words there.
//
// The carry (len1 ints per alignment in device memory) holds the stored key of column 16384 (s + 1) of every row, which lane
// 63 of stripe s's wave 15 writes and lane 0 of stripe s + 1's wave 0 takes as its left column, as it would from the ring;
// wave 0's left column in stripe 0 is the variant's H(i, 0) = -i gap.  CARRY ORDERING: row i is read by wave 0 in chunk
// (i - 1) / 32 of a stripe and overwritten by wave 15 in chunk 45 + (i + 62) / 32 of the SAME stripe, 45 barriers after its
// value was consumed; it is read again only in the next stripe, behind the closing s_waitcnt vmcnt(0) (the writer's stores
// have reached L2), the workgroup barrier (every wave has passed that drain and its last ring read) and the agent-scope
// acquire fence (the next stripe's loads miss this CU's L1, which may hold the rows as the previous stripe left them).  The
// carry is written with vector stores and read with per-lane vector loads (carry_row, tile_sweep.h), never through a scalar
// load.  Which chunk reads and which writes a row follows from the row, the lane and the wave alone: a semi-global entry may
// be negative where a local one is not, and that changes no step of this argument.
//
// BARRIER INVARIANT: every wave of the workgroup executes total_chunks + 1 barriers in every stripe but the last and
// total_chunks in the last, with total_chunks = ceil((len1 + 63) / 32) + 3 (W - 1) made of len1 and blockDim alone.  What this
// variant has the body do beyond the cells -- the row maximum and its strict comparison inside a chunk's work, the fold of the
// stripe's best cell between the sweep and the closing barrier (six shuffles and one LDS word that only lane 0 of the wave
// touches) -- lies on no path that holds a barrier; the variant itself (sgfull_variant.h) holds none.  `more_stripes` is made
// of len2 and the stripe index, both uniform, so every wave takes the closing drain, barrier and fence or none does.  A wave
// with no column in the last stripe (my_chunks = 0) skips the chunks' work, not their barriers.  With len2 <= 16384 (a long
// seq1 alone) there is one stripe, W = waves(len2) and the carry is never touched (it may be NULL).
//
// Best cell under stripes.  In every stripe a lane's `best` restarts at the stored key of H = 0 and best_row at 0, and a row's
// maximum replaces them only when its H is strictly greater (compared against best | 63): so only a cell strictly above 0 is
// ever taken, and a lane ends the stripe with the first row holding the strictly largest positive H among its 16 columns of
// that stripe (the key's low bits naming the first such column), or with (H 0, row 0) and then column 0.  After the stripe it
// folds
//     H << 34 | (0x1FFFF - row) << 17 | (0x1FFFF - col),      col = the lane's GLOBAL jbase + jj + 1
// into the wave's running best with a 64-bit maximum.  The pack orders H descending, then row ascending, then column ascending,
// so the maximum over all lanes and all stripes is the first cell in row-major order holding the largest H above 0, whichever
// stripe it lies in -- which is the reference's "strictly above every earlier one" -- and (0, 0, 0) when no cell is above 0,
// which every lane of every stripe then folds.  It is not "the earlier stripe wins": a later stripe's cell in a lower row
// beats an equal cell of stripe 0.  A wave that skipped the last stripe folds (0, 0, 0) as well, which every other candidate
// ties or beats.  Cells at or below 0 never enter the pack, so its unsigned H field never sees a negative value.
//
// Key range.  The host accepts a call iff P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gap) (swmi.h): H is not floored,
// so global_long_kernels.hip's rule applies here and local_long_kernels.hip's "no domain rule" does not.  (a) A path from (0, 0)
// to a valid cell (i, j) makes at most i + j <= len1 + len2 moves of at most P each in magnitude (a diagonal covers two of
// i + j), the borders included, so |H| <= 2^23 in every valid cell.  (b) A padded column (j > len2, scored -128 whatever P is)
// lies at most 1023 columns right of column len2, in the last stripe only; its H is at most the largest H it derives from and
// at least H(i, j - 1) - gap, so H > -2^23 - 1023 * 127 > -2^23 - 2^17; row 0's closed form there is -(len2 + 1023) gap, within
// the same bound.  (c) A lane computes no row outside 1 .. len1, and the left border's closed form, evaluated for up to 95 such
// rows, is at most (65536 + 95) * 127 < 2^23 in magnitude.  So every key H << 6 has |H << 6| < 2^29 + 2^23, every candidate (a
// key plus a score or a gap, << 6) stays below 2^30 in magnitude, and nothing wraps.  The best cell's H is at least 0 and at
// most P min(len1, len2) <= 2^22 < 2^23: the local fold's pack (uint32_t)h << 34 applies as it stands, H fits the 30 bits above
// bit 34, and the 17-bit row and column fields hold 65536.
//
// Columns past len2 are computed with every score -128; they occur in the LAST stripe only (every earlier stripe is full),
// in the last lanes of the wave that holds column len2 (later waves skip the stripe).  sgfull_kernels.hip's induction over the
// cells in row-major order carries over with "cell" read over ALL stripes: a padded cell of row 0 holds -j gap <= 0 = H(0, 0);
// any other holds its diagonal candidate (a cell of the row above minus 128), or its up candidate (a padded cell of the row
// above minus gap >= 0), or its left candidate (the row's last valid cell or a padded cell left of it, minus gap >= 0); so a
// padded cell is at most some valid cell EARLIER in row-major order -- on the same row left of it or on an earlier row, in the
// last stripe or in an earlier one.  That valid cell has H at least as large, and a smaller row or the same row and a smaller
// column, so it wins the pack's comparison against the padded cell whichever stripe folded it: the reduction never picks a
// padded cell.  What padded columns compute flows only right and down into other padded columns -- never into the carry, which
// only full stripes write -- and the walk only moves up and left from a valid cell.
//
// Indices at 65536 x 65536: trips(len1) = 16400, code_words = 64 * 16400 * 256 = 268 697 600 per alignment (size_t sums, times
// the alignment index); the carry index k * len1 is a size_t; a walk is at most 131072 moves, `lengths` at most 131073.
#include "sgfull_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void sg_long_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                  int len1, int len2, SmCols cols, int gap, int32_t *__restrict__ scores,
                                                                  int32_t *__restrict__ ends, uint32_t *__restrict__ codes,
                                                                  unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts,
                                                                  uint32_t move_words, uint32_t n_trips, int *carry)
{
    using V = SgLinear;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED
    const V::Gaps gaps{gap};
#include "tile_sweep_body.inc"
}

}  // namespace

size_t sgfull_long_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_sgfull_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                              size_t move_words, int32_t *d_carry, hipStream_t stream)
{
    return tile::launch_striped<sg_long_kernel<true>, sg_long_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends,
                                                                             d_codes, d_moves, d_lengths, move_words, d_carry, stream,
                                                                             gap);
}

}  // namespace swmi
