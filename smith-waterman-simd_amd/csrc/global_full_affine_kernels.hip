// global_full_affine_kernels.hip -- gfx950 kernel of the global and free-end-gap aligner with AFFINE gaps for two sequences of
// any length, with end cell, start cell and traceback (swmi_global_full_affine*).
//
// Semantics (include/swmi.h): Gotoh's recurrences with the borders and the end cell of
// global_full_kernels.hip, a gap of length k costing open + (k-1) extend.  With free_ends a mask of kFreeBegin1 / kFreeBegin2 /
// kFreeEnd1 / kFreeEnd2,
//     H(0,0) = 0,  H(i,0) = kFreeBegin1 ? 0 : -(open + (i-1) extend),  H(0,j) = kFreeBegin2 ? 0 : -(open + (j-1) extend)
//     E(0,j) = F(i,0) = -inf
//     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap (an up move)
//     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap (a left move)
//     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))          (no zero floor)
// The end cell is (len1, len2), with kFreeEnd1 also any (i, len2), i = 0..len1, with kFreeEnd2 also any (len1, j), j = 0..len2:
// the largest H, among equal ones the first in row-major order.  The walk goes back from it in state H (diagonal, E, F) and
// through E / F runs (opening wins a tie); on row 0 (column 0) it ends if kFreeBegin2 (kFreeBegin1) is set and else goes on to
// (0, 0) by forced moves.  Mask 0 with open == extend is Needleman-Wunsch; mask 0 is Gotoh's global alignment.
//
// Mapping, ring timing, code layout and the end rule (best cell, biased reduction, the walk's end): tile_sweep.h.  The sweep
// and the walk (the (H, F) hand-over, the code word, the walk's states) are tile_sweep_affine_body.inc, shared with
// sgfull_affine_kernels.hip and local_full_affine_kernels.hip; this file holds what depends on the recurrence.
//
// The cell as KEYS is sgfull_affine_kernels.hip's: key = value << 6 | tag << 4 | low, a stored H key with tag 3 and
// low = 15 - jj, E and F kept as keys of tag 2 and 1 with a traceback; one v_max3_i32 picks H's winner (diagonal before E
// before F), each of E's and F's maxes prefers opening, and bit 4 (E) or bit 5 (F) of its winner is the open bit.  A free
// border is a border of open = extend = 0: its keys are those of H = 0, and the body keeps one (open, extend) per border.
//
// Key range: every reachable H, E and F of a valid cell lies in [-127 (len1 + len2), 127 min(len1, len2)]: a path to the
// cell holds at most min(i, j) diagonals at 127 each, and at most i + j <= 32768 moves at -127 each (a gap's every cell costs
// at most 127, a diagonal's at least -127 and covers two of i + j).  A free border only raises border values toward 0, so the
// lower bound holds with every mask.  A padded column (below) reaches at most 1023 columns further and loses at most 127 per
// column (its H is at least its F, one gap cell below its left neighbour).  So |value| < 2^23: value << 6 fits in 30 bits with room for -inf = -2^30 and one extend below it (E and F are
// rebuilt from H's open term every cell, so -inf never accumulates more than one extend), and kEndBias = 2^22 exceeds
// 127 * 32768, the largest |H| of a valid cell.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128.  What they compute flows only
// right and down, into other such columns, so no valid cell depends on one; the end rule reads the last column from the
// lane and register that hold column len2 and masks columns past len2 out of the last row, so it never picks one; the walk
// only moves up and left from a valid cell, so it never enters one.  No claim about the VALUES of padded cells is needed or
// made: with a free row 0 a padded cell may hold 0 = H(0, len2), which the induction of sgfull_affine_kernels.hip would not
// allow, and which harms nothing here.
//
// Codes: H's field of the low dword is the winner's tag (3 / 2 / 1 = diagonal / E / F); the high dword holds the open bits.
// A staging block of the walk is 128 rows x 32 lanes (512 columns) of qwords.
//
// Walk: no code stops it; E(1,j) and F(i,1) always open, so it reaches row 0 or column 0 in state H, and there the end rule's
// tail takes over.  An end cell on a border never enters the staged loop.
#include "global_full_affine_variant.h"

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
// is unused; else `work` is NULL and unread (tile_sweep.h).  The mask and the gaps stay the launch's: one call has one of each.
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void global_full_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int fixed_len1, int fixed_len2, SmCols cols, int gap_open,
    int gap_extend, unsigned free_ends, int32_t *__restrict__ scores, int32_t *__restrict__ ends,
    unsigned long long *__restrict__ codes, unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts,
    uint32_t move_words, uint32_t fixed_trips, const TileWork *__restrict__ work)
{
    using V = GlobalAffine;
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_affine_body.inc"
}

}  // namespace

// qwords of codes per alignment: 4 bits per cell of every lane's 16 columns, for every step of the padded sweep
size_t global_full_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_global_full_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_steps, size_t move_words,
                                     hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch<global_full_affine_kernel<true>, global_full_affine_kernel<false>>(
        d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_steps, move_words, stream, gap_open, gap_extend,
        free_ends);
}

hipError_t launch_global_full_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                            int waves, const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends,
                                            int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                            unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if (free_ends > 15u) return hipErrorInvalidValue;
    return tile::launch_ragged<global_full_affine_kernel<true, true>, global_full_affine_kernel<false, true>>(
        d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores, d_ends, d_codes, d_moves, d_steps, stream, gap_open, gap_extend, free_ends);
}

}  // namespace swmi
