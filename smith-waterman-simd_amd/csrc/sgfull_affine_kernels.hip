// sgfull_affine_kernels.hip -- gfx950 kernel of the exact semi-global aligner with AFFINE gaps and traceback
// (swmi_semiglobal_full_affine*).
//
// Semantics (include/swmi.h): Gotoh's recurrences with the border of swmi_semiglobal_full, a gap of
// length k costing open + (k-1) extend:
//     H(0,0) = 0,  H(0,j) = -(open + (j-1) extend),  H(i,0) = -(open + (i-1) extend),  E(0,j) = F(i,0) = -inf
//     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap (an up move)
//     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap (a left move)
//     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))          (no zero floor)
// The best cell is that of sgfull_kernels.hip; the walk goes back from it in state H (diagonal, E, F) and through E / F runs
// (opening wins a tie), forced along row 0 and column 0.
//
// Mapping, ring timing, best-cell rule, code layout and ragged launches (swmi_semiglobal_full_affine_ragged*, DESIGN.md
// section 27): tile_sweep.h, which also holds the constants, the helpers and the launchers.  The sweep and the walk (the
// (H, F) hand-over, the code word, the walk's states) are tile_sweep_affine_body.inc, shared with local_full_affine_kernels.hip; what depends on the recurrence is the variant's
// (sgfull_affine_variant.h, shared with sgfull_long_affine_kernels.hip), and this file tells it.
//
// The cell as KEYS: key = value << 6 | tag << 4 | low, |value| < 2^23 (below).  A stored H key has tag 3 and low = 15 - jj
// (jj = the column within the lane); E and F are kept as keys of tag 2 and 1 with a traceback (one v_and_or_b32 after their
// max).  Every candidate is one add away from a neighbour's key:
//     diag      = key(i-1,j-1) + s << 6        tag 3              E's open = key(i-1,j) - open << 6    tag 3
//     E(i,j)    as kept                        tag 2              E's ext  = E(i-1,j) - extend << 6   tag 2
//     F(i,j)    as kept                        tag 1              F's open = key(i,j-1) - open << 6    tag 3
//                                                                 F's ext  = F(i,j-1) - extend << 6   tag 1
// so one v_max3_i32 picks H's largest candidate and, among equal values, diagonal before E before F, and the tag of the
// winner is H's field (3 / 2 / 1); each of E's and F's maxes prefers opening on equal values, and bit 4 (E) or bit 5 (F) of
// its winner is the open bit.  The low 4 bits never carry into the tag and never decide between two candidates (their tags
// differ).  Ends-only only H's values and the best key's column matter, so E and F are not masked.  Every reachable H, E
// and F lies in [-127 (len1 + len2), 127 min(len1, len2)] (include/swmi.h); a padded column below reaches at most 1023
// columns further at -127 per column, so |value| < 2^23 and value << 6 fits with room for -inf = -2^30 and one extend.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128.  What they compute flows only
// right and down: F along the row, E down the column, H diagonally -- into other such columns, never into a valid one.
// Let M(p) be the largest H of the valid cells before p in row-major order (>= H(0,0) = 0).  By induction in row-major
// order every padded cell p = (i, j) has H(p) <= M(p): its diagonal term is H(i-1,j-1) - 128, a valid cell before p minus
// 128 or a padded cell q before p with H(q) <= M(q) <= M(p), minus 128; F(i,j) is the largest of H(i,k) - open - (j-1-k)
// extend over k < j, each H(i,k) a valid cell of the same row (before p) or a padded one before p; E(i,j) is the largest of
// H(k,j) - open - (i-1-k) extend over k < i, each H(k,j) a padded cell of an earlier row or H(0,j) <= 0 = H(0,0).  Every
// gap cost is >= 0, so H(p) <= M(p): a padded cell never holds a value that an earlier valid cell lacks, and the best-cell
// rule (strictly greater; row, then column ascending) never picks one.
//
// Codes: H's field of the low dword is the winner's tag (3 / 2 / 1 = diagonal / E / F), as sgfull_kernels.hip's codes.
//
// Walk: no code stops it; it reaches row 0 or column 0 in state H, and from there it is forced to (0, 0).
#include "sgfull_affine_variant.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's proofs, bounds and code word were written against (tile_sweep.h owns it; a change there must
// revisit them)
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

// RAGGED: one TileWork per workgroup (work[blockIdx.x]) names the alignment, and the launch's own shape (fixed_*, move_words)
// is unused; else `work` is NULL and unread (tile_sweep.h).  The gaps stay the launch's: one call has one pair.  A slot with a
// zero length is sgfull_kernels.hip's: score 0 at (0, 0), no move, a path of one position.
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void sg_full_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int fixed_len1, int fixed_len2, SmCols cols, int gap_open,
    int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, uint32_t move_words, uint32_t fixed_trips,
    const TileWork *__restrict__ work)
{
    using V = SgAffine;
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_affine_body.inc"
}

}  // namespace

// qwords of codes per alignment: 4 bits per cell of every lane's 16 columns, for every step of the padded sweep
size_t sgfull_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_sgfull_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                unsigned long long *d_moves, uint32_t *d_lengths, size_t move_words, hipStream_t stream)
{
    return tile::launch<sg_full_affine_kernel<true>, sg_full_affine_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_lengths,
        move_words, stream, gap_open, gap_extend);
}

hipError_t launch_sgfull_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                       const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends,
                                       unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                                       hipStream_t stream)
{
    return tile::launch_ragged<sg_full_affine_kernel<true, true>, sg_full_affine_kernel<false, true>>(
        d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores, d_ends, d_codes, d_moves, d_lengths, stream, gap_open, gap_extend);
}

}  // namespace swmi
