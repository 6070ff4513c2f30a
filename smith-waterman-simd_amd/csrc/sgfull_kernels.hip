// sgfull_kernels.hip -- gfx950 kernel of the exact semi-global aligner with traceback (swmi_semiglobal_full*).
//
// Semantics: the reference's SemiGlobal_111 (source.cpp:1776-1834) generalised to any int8 matrix, gap and lengths:
//     H(0,0) = 0, H(0,j) = -j gap, H(i,0) = -i gap,
//     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)      (no zero floor)
// for i = 1..len1, j = 1..len2.  The best cell is the first cell in row-major order strictly above every earlier one,
// from 0 at (0,0); the walk goes back from it to (0,0), diagonal before up before left.  DESIGN.md section 13.
//
// Mapping, ring timing, best-cell reduction, code layout, staged walk and ragged launches (swmi_semiglobal_full_ragged*,
// DESIGN.md section 27): tile_sweep.h.  The recurrence is the variant's (sgfull_variant.h, shared with
// sgfull_long_kernels.hip); this file tells it.
//
// The cell as KEYS: key = H << 6 | tag << 4 | (15 - jj) (jj = the column within the lane).  A stored key has tag 3; the
// candidates come from the neighbours' keys by one add each:
//     diag = key(i-1,j-1) + s << 6            (tag stays 3)
//     up   = key(i-1,j)   - gap << 6 - 1 << 4  (tag 2)
//     left = key(i,j-1)   - gap << 6 - 2 << 4  (tag 1)
// so ONE v_max3_i32 picks the largest value and, among equal values, diagonal before up before left; the winner's tag is
// the cell's move code (3 / 2 / 1 = diagonal / up / left: the moves encoding itself), and one v_and_or_b32 turns the
// winner back into a stored key.  The low 4 bits never carry into the tag and never decide between two candidates (their
// tags differ).  |H| <= 128 * 32768 < 2^22, so H << 6 fits.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128.  What they compute flows only
// right and down, into other such columns, and by induction each of their cells is at most some valid cell that comes
// earlier in row-major order (its diagonal term is a valid cell of the row above minus 128, its up and left terms are such
// cells minus gap >= 0).  So they never hold a value that the first valid cell holding it would not already have taken,
// and the best-cell rule (strictly greater; row, then column ascending) never picks one.
//
// Codes: 2 bits per cell, one dword per lane and row, column jj at bits 2 jj: the move itself (3 / 2 / 1).  A staging block
// of the walk is 128 rows x 64 lanes (1024 columns): at 16384 x 16384 a path needs at most 256 blocks.
#include "sgfull_variant.h"

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
// is unused; else `work` is NULL and unread (tile_sweep.h).  The gap stays the launch's: one call has one.  A slot with a
// zero length is one border whose cells are all <= 0 with (0, 0) first: score 0 at (0, 0), no move, a path of one position.
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void sg_full_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                  int fixed_len1, int fixed_len2, SmCols cols, int gap,
                                                                  int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                                                                  uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves,
                                                                  uint32_t *__restrict__ counts, uint32_t move_words, uint32_t fixed_trips,
                                                                  const TileWork *__restrict__ work)
{
    using V = SgLinear;
    const V::Gaps gaps{gap};
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
#include "tile_sweep_body.inc"
}

}  // namespace

int sgfull_waves(int len2) { return tile::waves(len2); }

size_t sgfull_trips(int len1) { return tile::trips(len1); }

size_t sgfull_code_words(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_sgfull(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                         int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                         size_t move_words, hipStream_t stream)
{
    return tile::launch<sg_full_kernel<true>, sg_full_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes,
                                                                     d_moves, d_lengths, move_words, stream, gap);
}

int sgfull_ragged_waves(int len1, int len2) { return len1 > 0 && len2 > 0 ? tile::waves(len2) : 1; }

hipError_t launch_sgfull_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                const int8_t *sm, int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes,
                                unsigned long long *d_moves, uint32_t *d_lengths, hipStream_t stream)
{
    return tile::launch_ragged<sg_full_kernel<true, true>, sg_full_kernel<false, true>>(d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores,
                                                                                        d_ends, d_codes, d_moves, d_lengths, stream, gap);
}

}  // namespace swmi
