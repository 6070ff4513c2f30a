// sgfull_long_affine_kernels.hip -- gfx950 kernel of the exact semi-global aligner with AFFINE gaps for two sequences of up to
// 65536 bases, with best cell and traceback (swmi_semiglobal_long_affine*).
//
// Semantics: sgfull_affine_kernels.hip's, cell for cell (include/swmi.h, DESIGN.md sections 16 and 26): Gotoh's recurrences
// with charged borders (H(0, j) = -(open + (j - 1) extend), E(0, j) = F(i, 0) = -inf), no zero floor, sgfull_kernels.hip's best
// cell, and the walk back to (0, 0) in state H / E / F, opening wins a tie, forced on row 0 and column 0; the variant is that
// file's (sgfull_affine_variant.h).  Mapping: sgfull_long_kernels.hip's column stripes, with the affine body's (H, F) pairs in
// the carry (len1 int2 per alignment): F runs along the row, so a gap that opens left of a stripe's edge extends across it
// through the carry as it does through the ring between two waves; E runs down a column and stays with the lane, and starts
// at -inf on row 0 of every stripe.  A stripe sets up row 0's keys from the lane's GLOBAL column and diag_in = H(0, 16 G);
// wave 0's left column in stripe 0 is H(i, 0) with F = -inf.
//
// CARRY ORDERING: row i's (H, F) is read by wave 0 in chunk (i - 1) / 32 of a stripe and overwritten by wave 15 in chunk
// 45 + (i + 62) / 32 of the SAME stripe, 45 barriers after its value was consumed; the next stripe reads it behind the closing
// s_waitcnt vmcnt(0) (the writer's stores have reached L2), the workgroup barrier (every wave has passed that drain and its
// last ring read) and the agent-scope acquire fence (the next stripe's loads miss this CU's L1).  One 8-byte vector store per
// row writes it, a per-lane vector load (carry_row, tile_sweep.h) reads it, never a scalar load.  Which chunk reads and which
// writes a row follows from the row, the lane and the wave alone; that an entry may be negative here, or F still -inf, changes
// no step of it.
//
// BARRIER INVARIANT: every wave executes total_chunks + 1 barriers in every stripe but the last and total_chunks in the last,
// total_chunks = ceil((len1 + 63) / 32) + 3 (W - 1) made of len1 and blockDim alone.  The variant is five constants and three
// one-line functions without a barrier; what the body does for it beyond the cells -- the row maximum and its strict comparison
// inside a chunk's work, the fold of the stripe's best cell between the sweep and the closing barrier -- lies on no path that
// holds a barrier.  `more_stripes` is made of len2 and the stripe index, both uniform.  A wave with my_chunks = 0 skips the
// chunks' work, not their barriers.  With len2 <= 16384 there is one stripe and the carry is never touched (it may be NULL).
//
// Best cell under stripes: sgfull_long_kernels.hip's.  `best` restarts at the stored key of H = 0 (kTagH) in every stripe, only
// a row maximum strictly above it replaces it, so only a cell strictly above 0 is ever taken; the stripe's candidate
// H << 34 | (0x1FFFF - row) << 17 | (0x1FFFF - col) with the GLOBAL column is folded with a 64-bit maximum, which orders H
// descending, row ascending, column ascending: the first cell in row-major order over all stripes holding the largest H above
// 0, or (0, 0, 0), which is also what a wave that skipped the last stripe folds.
//
// Key range.  The host accepts a call iff P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gap_open, gap_extend) (swmi.h).
// (a) Every cell of a gap costs at most P and every diagonal at most P in magnitude, the borders included, so H, and E and F
// where they are reachable, lie within 2^23 of 0 in every valid cell.  (b) A padded column (j > len2, scored -128 whatever P
// is; at most 1023 of them, in the last stripe) has H >= F >= H(i, j - 1) - open, so it loses at most 127 per column: value >
// -2^23 - 2^17; row 0's closed form there stays within the same bound.  (c) A lane computes no row outside 1 .. len1; the
// border's closed form for up to 95 such rows stays below (65536 + 95) * 127 < 2^23.  So |value << 6| < 2^29 + 2^23 for every
// reachable value: strictly above kMinusInf = -2^30, which therefore still loses every max it should lose (E(1, j) and F(i, 1)
// always open; F into a later stripe's lane 0 is the carry's reachable F of column 16384 s).  E and F are rebuilt from H's
// open term in every cell, so -inf never decays by more than one extend before a reachable value replaces it:
// -2^30 - 127 * 64 > -2^31, no wrap.  The best cell's H is in [0, 2^22], so the pack's (uint32_t)h << 34 applies as it stands.
//
// Columns past len2 occur in the LAST stripe only.  sgfull_affine_kernels.hip's induction holds with "cell" read over ALL
// stripes: with M(p) the largest H of the valid cells before p in row-major order (>= H(0, 0) = 0), every padded cell p has
// H(p) <= M(p) -- its diagonal term is a cell before p minus 128; F(i, j) is the largest of H(i, k) - open - (j - 1 - k) extend
// over k < j, each H(i, k) a cell of the same row before p, valid (in this or an earlier stripe, through the carry) or padded;
// E(i, j) is the largest of H(k, j) - open - (i - 1 - k) extend over k < i, each a padded cell of an earlier row or
// H(0, j) <= 0; every gap cost is >= 0.  A valid cell that attains M(p) precedes p in row-major order and so wins the pack's
// comparison whichever stripe folded it: the reduction never picks a padded cell.  Padded columns feed only padded columns,
// never the carry (only full stripes write it), and the walk never enters one.
#include "sgfull_affine_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's bounds were written against (tile_sweep.h owns it; a change there must revisit them)
static_assert(tile::kCols == 16 && tile::kMaxWaves == 16 && tile::kStripeCols == 16384 && tile::kChunk == 32 && tile::kDelay == 3);

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void sg_long_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int len1, int len2, SmCols cols, int gap_open, int gap_extend,
    int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, uint32_t move_words, uint32_t n_trips, int2 *carry_hf)
{
    using V = SgAffine;
    constexpr bool STRIPED = true;                 // what the body reads instead of tile::STRIPED
#include "tile_sweep_affine_body.inc"
}

}  // namespace

size_t sgfull_long_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_sgfull_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                     unsigned long long *d_moves, uint32_t *d_lengths, size_t move_words, int32_t *d_carry,
                                     hipStream_t stream)
{
    return tile::launch_striped<sg_long_affine_kernel<true>, sg_long_affine_kernel<false>>(
        d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_lengths, move_words, reinterpret_cast<int2 *>(d_carry),
        stream, gap_open, gap_extend);
}

}  // namespace swmi
