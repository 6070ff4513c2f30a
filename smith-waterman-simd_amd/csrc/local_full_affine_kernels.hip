// local_full_affine_kernels.hip -- gfx950 kernel of the local aligner for two sequences of any length with AFFINE gaps, end
// cell, start cell and traceback (swmi_local_full_affine*).
//
// Semantics (include/swmi.h): swmi_local_full's borders and zero floor with Gotoh's gaps, a gap of
// length k costing open + (k-1) extend:
//     H(i,0) = H(0,j) = 0,  E(0,j) = F(i,0) = -inf
//     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap (an up move)
//     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap (a left move)
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j)),   i = 1..len1, j = 1..len2
// The end cell is the first cell in row-major order holding max H ((0,0) when that is 0).  The walk goes back from it in
// state H: it stops at the first cell holding 0 (the test comes first), else takes a diagonal, else enters E, else F; inside
// E / F it takes up / left steps and returns to H where the gap opened (opening wins a tie).
//
// Mapping, ring timing, best-cell rule and code layout: tile_sweep.h, which also holds the constants, the helpers and the
// launcher.  The sweep and the walk (the (H, F) hand-over, the code word, the walk's states) are
// tile_sweep_affine_body.inc, shared with sgfull_affine_kernels.hip; what depends on the recurrence is LocalAffine,
// local_full_affine_variant.h (shared with local_long_affine_kernels.hip); this comment tells it.
//
// The cell as KEYS: key = value << 6 | tag << 4 | low.  A stored H key has tag 2 and low = 15 - jj (jj = the column within
// the lane); with a traceback E is kept masked to tag 1 and F to tag 0 (one v_and_or_b32 after their max).  Every candidate
// is one add away from a neighbour's key:
//     floor     = 0 << 6 | 3 << 4              tag 3: the constant 48, an inline operand
//     diag      = key(i-1,j-1) + s << 6        tag 2              E's open = key(i-1,j) - open << 6    tag 2
//     E(i,j)    as kept                        tag 1              E's ext  = E(i-1,j) - extend << 6   tag 1
//     F(i,j)    as kept                        tag 0              F's open = key(i,j-1) - open << 6    tag 2
//                                                                 F's ext  = F(i,j-1) - extend << 6   tag 0
// so one v_max3_i32 and one v_max_i32 pick H's largest candidate and, among equal values, the floor before diagonal before
// E before F: at value 0 every other candidate is at most 0 << 6 | 2 << 4 | 15 = 47 < 48, so the floor wins every tie at 0,
// and a candidate below 0 is a negative key.  The winner's tag is the cell's CODE: 3 = stop, 2 = diagonal, 1 = E, 0 = F.
// Each of E's and F's maxes prefers opening on equal values (tag 2 above tag 1 and tag 0), and bit 5 of its winner is the
// open bit.  The low 4 bits never carry into the tag and never decide between two candidates (their tags differ).
// Ends-only only H's values and the best key's column matter, so E and F are not masked.  H lies in [0, 2^21)
// (127 * 16384 < 2^21), and wherever E or F derives from an H it is at least -open >= -127 and at most H, so apart from the
// sentinel every key lies in (-2^14, 2^27); -inf = -2^30 is only ever extended once before an open candidate replaces it
// (E(1,j) and F(i,1) always open), so -2^30 - (127 << 6) is the lowest key: no overflow, and far below every real key.
//
// Borders: row 0 and column 0 hold the stored key of H = 0, a constant; E on row 0 and F into wave 0's lane 0 are -inf, so
// E(1,j) and F(i,1) always open.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128; with the floor they hold values
// >= 0.  Induction over the cells in row-major order: a padded cell p = (i, j) holds 0, or its diagonal candidate (a cell of
// the row above, valid or padded, minus 128), or E(i,j) = the largest of H(k,j) - open - (i-1-k) extend over k < i (each
// H(k,j) a padded cell of an earlier row, or H(0,j) = 0), or F(i,j) = the largest of H(i,k) - open - (j-1-k) extend over
// k < j (each H(i,k) a valid cell of the same row or a padded cell left of p, all before p).  Every gap cost is >= 0, so each
// source is a valid cell earlier in row-major order or a padded cell earlier in it, which by induction is at most some
// valid cell earlier still.  So a padded cell above 0 is at most some valid cell EARLIER in row-major order -- also at
// open = 0, where "at most" may be "equal" -- and a padded cell holding 0 never beats the initial best of 0.  The best-cell
// rule (strictly greater; then row, then column ascending) never picks a padded cell.  What padded columns compute flows
// only right and down, into other padded columns, and the walk only moves up and left from a valid cell, so it never
// enters one.
//
// Codes: H's field of the low dword is the winner's tag (3 = stop, 2 / 1 / 0 = diagonal / E / F).
//
// Walk: it ends on a stop code read in state H (inside E or F the cell's H code is not consulted), on row 0 or on column 0
// (border cells hold 0 and have no code), where it arrives in state H.
#include "local_full_affine_variant.h"

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
// is unused; else `work` is NULL and unread (tile_sweep.h).
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void local_full_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int fixed_len1, int fixed_len2, SmCols cols, int gap_open,
    int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, uint32_t move_words, uint32_t fixed_trips,
    const TileWork *__restrict__ work)
{
    using V = LocalAffine;
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_affine_body.inc"
}

}  // namespace

// qwords of codes per alignment: 4 bits per cell of every lane's 16 columns, for every step of the padded sweep
size_t local_full_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_local_full_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                    int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, size_t move_words, hipStream_t stream)
{
    return tile::launch<local_full_affine_kernel<true>, local_full_affine_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_steps,
        move_words, stream, gap_open, gap_extend);
}

hipError_t launch_local_full_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                           int waves, const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores,
                                           int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                           uint32_t *d_steps, hipStream_t stream)
{
    return tile::launch_ragged<local_full_affine_kernel<true, true>, local_full_affine_kernel<false, true>>(
        d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores, d_ends, d_codes, d_moves, d_steps, stream, gap_open, gap_extend);
}

}  // namespace swmi
