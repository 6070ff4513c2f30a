// local_full_kernels.hip -- gfx950 kernel of the local aligner for two sequences of any length, with end cell, start cell
// and traceback (swmi_local_full*).
//
// Semantics: swmi_local_align's (the reference's SmithWaterman_111_long, source.cpp:1526-1576) with a seq2 of len2 bases
// instead of 128, any int8 matrix and gap:
//     H(i,0) = H(0,j) = 0
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),   i = 1..len1, j = 1..len2
// The end cell is the first cell in row-major order holding max H ((0,0) when that is 0); the walk from it stops at the
// first cell holding 0 (the test comes first), else takes a diagonal, else an up, else a left step.  DESIGN.md section 17.
//
// Mapping, ring timing, best-cell reduction, code layout and staged walk: tile_sweep.h.  The recurrence is LocalLinear,
// local_full_variant.h (shared with local_long_kernels.hip); this comment tells it.
//
// The cell as KEYS: key = H << 6 | tag << 4 | (15 - jj) (jj = the column within the lane).  H >= 0 and
// H <= 127 * 16384 < 2^21, so every stored key is positive and below 2^27.  A stored key has tag 2; the four candidates are
//     floor = 0 << 6 | 3 << 4                          (tag 3: the constant 48, an inline operand)
//     diag  = key(i-1,j-1) + s << 6                     (tag stays 2)
//     up    = key(i-1,j)   - gap << 6 - 1 << 4          (tag 1)
//     left  = key(i,j-1)   - gap << 6 - 2 << 4          (tag 0)
// so one v_max3_i32 and one v_max_i32 pick the largest value and, among equal values, the floor before diagonal before up
// before left: at value 0 the other candidates are at most 0 << 6 | 2 << 4 | 15 = 47 < 48, so the floor wins every tie at
// 0, and a candidate below 0 is a negative key.  The winner's tag is the cell's CODE: 3 = stop, 2 / 1 / 0 = diagonal / up /
// left (the move is code + 1).  The walker has no H to test: a stored stop code is what ends the walk.  One v_and_or_b32
// turns the winner back into a stored key.  The low 4 bits never carry into the tag and never decide between two
// candidates (their tags differ).
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128; with the floor they hold values
// >= 0.  Induction over the cells in row-major order: a padded cell holds 0, or its diagonal candidate (a cell of the row
// above, valid or padded, minus 128), or its up candidate (a padded cell of the row above minus gap >= 0), or its left
// candidate (the row's last valid cell or a padded cell left of it, minus gap >= 0).  Each of those is a valid cell earlier
// in row-major order or a padded cell earlier in it, which by induction is at most some valid cell earlier still.  So a
// padded cell above 0 is at most some valid cell EARLIER in row-major order -- also at gap 0, where "at most" may be
// "equal" -- and a padded cell holding 0 never beats the initial best of 0.  Valid columns are all smaller than padded
// ones, so the best-cell rule (strictly greater; then row, then column ascending) never picks a padded cell.  What padded
// columns compute flows only right and down, into other padded columns, and the walk only moves up and left from a valid
// cell, so it never enters one.
//
// Codes: 2 bits per cell, one dword per lane and row, column jj at bits 2 jj.  A staging block of the walk is 128 rows x
// 64 lanes (1024 columns); the walk inside it ends on a stop code, on row 0 or on column 0.
#include "local_full_variant.h"

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
__global__ __launch_bounds__(64 * kMaxWaves) void local_full_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                     int fixed_len1, int fixed_len2, SmCols cols, int gap,
                                                                     int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                                                                     uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves,
                                                                     uint32_t *__restrict__ counts, uint32_t move_words,
                                                                     uint32_t fixed_trips, const TileWork *__restrict__ work)
{
    using V = LocalLinear;
    const V::Gaps gaps{gap};
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_body.inc"
}

}  // namespace

size_t local_full_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_local_full(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                             int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                             size_t move_words, hipStream_t stream)
{
    return tile::launch<local_full_kernel<true>, local_full_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes,
                                                                           d_moves, d_steps, move_words, stream, gap);
}

int local_full_ragged_waves(int len1, int len2) { return len1 > 0 && len2 > 0 ? tile::waves(len2) : 1; }

hipError_t launch_local_full_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                    const int8_t *sm, int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    return tile::launch_ragged<local_full_kernel<true, true>, local_full_kernel<false, true>>(d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores,
                                                                                             d_ends, d_codes, d_moves, d_steps, stream, gap);
}

}  // namespace swmi
