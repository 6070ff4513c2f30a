// wide_affine_kernels.hip -- gfx950 kernels of the WIDE-alphabet aligners (libswmi_wide.so, include/swmi_wide.h, DESIGN.md
// section 29): local (Smith-Waterman / Gotoh with the zero floor) and global / fit / overlap (the free_ends mask) alignment
// with affine gaps over 32 letters and a caller-supplied 32 x 32 int8 matrix, on a batch of mixed (len1, len2), with end
// cell, start cell and traceback or ends-only.
//
// Semantics: local_full_affine_kernels.hip's and global_full_affine_kernels.hip's, recurrence, tie rules, end cell, walk and
// code word, with ONE difference: the substitution score of cell (i, j) is sm[(seq1[i-1] & 31) * 32 + (seq2[j-1] & 31)].
// The kernels are tile_sweep_affine_body.inc with the variants LocalAffine and GlobalAffine as those two files use them, and
// with the body's WIDE seam (tile_sweep.h): this file shadows WIDE, wide_sm and wide_prof, and nothing else of the sweep, the
// (H, F) hand-over, the end rule, the code words or the staged walk knows the alphabet.
//
// The profile: a lane owns 16 fixed columns and meets a new seq1 letter every row.  Per wave the profile is 32 letter rows of
// 64 lanes x 16 bytes (1 KiB a row, 32 KiB a wave) in LDS: byte jj of wide_prof[(32 w + a) 64 + l] is sm[a * 32 + letter of
// column 16 (64 w + l) + jj + 1], or -128 past len2.  Every lane builds its own 16 bytes of all 32 rows before its sweep and
// reads back nothing else, so the profile needs no barrier.  Per row the lane reads its 16 bytes with one ds_read_b128 and a
// cell's score is one v_bfe_i32 with a constant shift: the 16 `prof` registers of the 4-letter kernels become the 16 of the
// four rows in flight, and the cell's instruction count stays.  A letter's row is a multiple of 256 bytes, so within a
// ds_read_b128's group of 16 lanes the addresses l * 16 mod 256 cover all 64 banks once whatever the lanes' letters: no bank
// conflict (derived from the LDS bank layout, not measured).  A row's letter is loaded two trips and its profile row one trip
// ahead of use.
//
// Shapes: len2 <= 4096, so W = ceil(len2 / 1024) is 1 .. 4, and there is one instantiation per W, whose static LDS is what
// that W needs: W x 32 KiB of profile, a ring of max(W - 1, 1) x 256 int2 and the reduction's words; the walk's 32 KiB
// staging block lies where wave 0's profile lay (the body reads no profile after the sweep's last barrier).  W = 4: 137 KiB
// of the CU's 160.  len1 <= 16384 as for the other tile kernels; the asymmetry is the profile's footprint.
//
// Key range: |H| <= 128 (16384 + 4096) < 2^22 for a valid cell of either kind (a path of i + j <= 20480 moves at a magnitude
// of at most 128 each: the matrix may hold -128), so kEndBias = 2^22 and the keys' `<< 6` hold as in the 4-letter kernels;
// a padded column reaches at most 1023 columns further at 127 a column, still below 2^23.  -inf = -2^30 is extended once at
// most before an open candidate replaces it.
//
// Columns past len2 are computed with every score -128, as in the 4-letter kernels, whose matrices may hold -128 as well: the
// arguments carry over unchanged.  Local kind (local_full_affine_kernels.hip): a padded cell holds 0, or its diagonal
// candidate -- a cell of the row above minus 128, so at most that cell, for every valid score is >= -128 -- or an E or F that
// derives from cells earlier in row-major order at a cost >= 0; so a padded cell above 0 is at most some valid cell earlier
// in row-major order, and the best-cell rule (strictly greater, then row, then column ascending) never picks it.  Global kind
// (global_full_affine_kernels.hip): the end rule masks columns past len2 out and reads column len2 from the lane that owns it,
// so no claim about padded values is needed.  For both, what padded columns compute flows only right and down, and the walk
// only moves up and left from a valid cell.
#include "global_full_affine_variant.h"
#include "local_full_affine_variant.h"
#include "wide_internal.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's LDS budget and bounds were written against (tile_sweep.h owns it)
static_assert(tile::kCols == 16 && tile::kUnroll == 4 && tile::kChunk == 32 && tile::kDelay == 3 && tile::kRing == 256 &&
              tile::kStageRows == 128);
static_assert(kWideMaxWaves * 64 * tile::kCols == kWideMaxLen2);

constexpr int kProfRow = 64;                       // uint4 per letter row of a wave
constexpr int kProfWave = 32 * kProfRow;           // uint4 per wave: 32 KiB, the size of a staging block of the walk
static_assert(kProfWave * sizeof(uint4) == tile::kStageRows * 32 * sizeof(unsigned long long));

// The kernels are ragged only: one TileWork per workgroup, one launch per wave count WAVES (= blockDim.x >> 6).
#define SWMI_WIDE_KERNEL_BODY(VARIANT)                                                                                          \
    using V = VARIANT;                                                                                                          \
    constexpr bool RAGGED = true, WIDE = true;                                                                                  \
    constexpr int kMaxWaves = WAVES > 1 ? WAVES : 2;      /* sizes the body's ring and reduction words */                      \
    constexpr SmCols cols{};                              /* the 4-letter profile's columns: unread */                         \
    constexpr uint32_t move_words = 0;                    /* a fixed launch's: unread */                                       \
    __shared__ uint4 wide_prof[WAVES * kProfWave];                                                                              \
    const TileWork slot = work[blockIdx.x];                                                                                     \
    const int len1 = (int)slot.len1, len2 = (int)slot.len2;                                                                     \
    const uint32_t n_trips = (uint32_t)trips(len1);                                                                             \
    (void)cols;                                                                                                                 \
    (void)move_words;

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_local_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const int8_t *__restrict__ wide_sm, int gap_open,
    int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, const TileWork *__restrict__ work)
{
    SWMI_WIDE_KERNEL_BODY(LocalAffine)
#include "tile_sweep_affine_body.inc"
}

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_global_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const int8_t *__restrict__ wide_sm, int gap_open,
    int gap_extend, unsigned free_ends, int32_t *__restrict__ scores, int32_t *__restrict__ ends,
    unsigned long long *__restrict__ codes, unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts,
    const TileWork *__restrict__ work)
{
    SWMI_WIDE_KERNEL_BODY(GlobalAffine)
#include "tile_sweep_affine_body.inc"
}
#undef SWMI_WIDE_KERNEL_BODY

template <int WAVES>
hipError_t fire_wide(WideKind kind, dim3 grid, hipStream_t st, const uint8_t *s1, const uint8_t *s2, const int8_t *sm, int open, int ext,
                     unsigned free_ends, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                     uint32_t *counts, const TileWork *work)
{
    const dim3 block(64 * WAVES);
    if (kind == kWideLocal) {
        if (moves)
            hipLaunchKernelGGL((wide_local_affine_kernel<true, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, scores, ends, codes,
                               moves, counts, work);
        else
            hipLaunchKernelGGL((wide_local_affine_kernel<false, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, scores, ends,
                               (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work);
    } else {
        if (moves)
            hipLaunchKernelGGL((wide_global_affine_kernel<true, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, free_ends, scores,
                               ends, codes, moves, counts, work);
        else
            hipLaunchKernelGGL((wide_global_affine_kernel<false, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, free_ends, scores,
                               ends, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work);
    }
    return hipGetLastError();
}

}  // namespace

size_t wide_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

int wide_ragged_waves(int len1, int len2) { return len1 == 0 || len2 == 0 ? 1 : tile::waves(len2); }

hipError_t launch_wide_affine_ragged(WideKind kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                     int waves, const int8_t *d_sm, int gap_open, int gap_extend, unsigned free_ends,
                                     int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                     uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (waves < 1 || waves > kWideMaxWaves || n > (size_t(1) << 20) || free_ends > 15u || !d_sm) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n);
#define SWMI_WIDE_FIRE(W)                                                                                                   \
    case W:                                                                                                                 \
        return fire_wide<W>(kind, grid, stream, d_seq1s, d_seq2s, d_sm, gap_open, gap_extend, free_ends, d_scores, d_ends, d_codes, \
                            d_moves, d_steps, d_work)
    switch (waves) {
        SWMI_WIDE_FIRE(1);
        SWMI_WIDE_FIRE(2);
        SWMI_WIDE_FIRE(3);
    default:
        SWMI_WIDE_FIRE(4);
    }
#undef SWMI_WIDE_FIRE
}

}  // namespace swmi
