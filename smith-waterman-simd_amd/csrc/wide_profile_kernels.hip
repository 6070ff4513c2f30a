// wide_profile_kernels.hip -- gfx950 kernels of the PROFILE aligners (libswmi_wide_profile.so, include/swmi_wide_profile.h,
// DESIGN.md section 32): local and global / fit / overlap alignment with affine gaps of a batch of sequences over 32 letters
// (the rows, mixed lengths) against ONE position-specific scoring matrix of len2 columns, with end cell, start cell and
// traceback or ends-only.
//
// Semantics: wide_affine_kernels.hip's, recurrence, tie rules, end cell, walk and code word, with ONE difference: the
// substitution score of cell (i, j) is profile[(j - 1) * 32 + (seq1[i-1] & 31)].  The kernels are tile_sweep_affine_body.inc
// with the variants LocalAffine and GlobalAffine and the body's WIDE seam as that file uses them, and with the PROFILED seam on
// top (tile_sweep.h): this file shadows WIDE, PROFILED, wide_pssm, wide_prof and an empty seq2s.  There is no seq2: the body
// neither computes nor dereferences s2, loads no column letters and reads no matrix.
//
// The profile in LDS is the wide kernels': per wave 32 letter rows of 64 lanes x 16 bytes, byte jj of
// wide_prof[(32 w + a) 64 + l] the score of letter a in column 16 (64 w + l) + jj + 1.  Here a lane does not build its 16
// bytes of a row from 16 byte loads of a matrix but loads them whole: the host has written the profile into device memory
// letter-major, 32 rows of 64 W uint4, entry G = 64 w + l of row a holding those 16 bytes, with -128 in every column past len2
// (wide_profile_internal.h).  So the build is 32 global_load_dwordx4, each coalesced over the wave (1 KiB contiguous), and 32
// LDS stores; the kernel never tests for the padding; and a lane still reads back only what it wrote, so there is still no
// barrier.  The row stride 64 W is the launch's: every slot of a launch has the same len2, hence the same W = blockDim.x >> 6.
//
// Shapes: len2 <= 4096, W = ceil(len2 / 1024) = 1 .. 4, one instantiation per kind x TB x W with the wide kernels' static LDS
// (W x 32 KiB of profile, the ring, the reduction's words; the walk stages where wave 0's profile lay).  len1 <= 16384.  A
// slot with a zero length leaves before any barrier and any load and is written for one wavefront: the host launches such
// slots (every slot when len2 = 0) as one-wavefront workgroups, in a launch of their own when W > 1.
//
// Key range: a profile may hold -128 in every entry, so |H| <= 128 (16384 + 4096) < 2^22 for a valid cell of either kind (a
// path of i + j <= 20480 moves at a magnitude of at most 128 each -- 127 for a gap), and kEndBias = 2^22 and the keys' `<< 6`
// hold as in the wide kernels; a padded column reaches at most 1023 columns further at 127 a column, still below 2^23.  No
// shape within the limits is outside the domain, so there is no domain rule.
//
// Columns past len2 score -128 against every letter, exactly what the wide kernels' padding computes, so
// wide_affine_kernels.hip's arguments for padded cells (local: never the best cell; global: masked out by the end rule) carry
// over word for word.
#include "global_full_affine_variant.h"
#include "local_full_affine_variant.h"
#include "wide_profile_internal.h"

namespace swmi {
namespace {

using namespace tile;

static_assert(tile::kCols == 16 && tile::kUnroll == 4 && tile::kChunk == 32 && tile::kDelay == 3 && tile::kRing == 256 &&
              tile::kStageRows == 128);
static_assert(kWideMaxWaves * 64 * tile::kCols == kWideMaxLen2);
static_assert(128 * (kWideMaxLen1 + kWideMaxLen2) < (1 << 22) && tile::kEndBias == (1 << 22));
static_assert(kWideProfileEntryBytes == sizeof(uint4));

constexpr int kProfRow = 64;                       // uint4 per letter row of a wave
constexpr int kProfWave = 32 * kProfRow;           // uint4 per wave: 32 KiB, the size of a staging block of the walk
static_assert(kProfWave * sizeof(uint4) == tile::kStageRows * 32 * sizeof(unsigned long long));

// Ragged only: one TileWork per workgroup, one launch per wave count WAVES (= blockDim.x >> 6).
#define SWMI_WIDE_PROFILE_KERNEL_BODY(VARIANT)                                                                                  \
    using V = VARIANT;                                                                                                          \
    constexpr bool RAGGED = true, WIDE = true, PROFILED = true;                                                                 \
    constexpr int kMaxWaves = WAVES > 1 ? WAVES : 2;      /* sizes the body's ring and reduction words */                      \
    constexpr SmCols cols{};                              /* the 4-letter profile's columns: unread */                         \
    constexpr uint32_t move_words = 0;                    /* a fixed launch's: unread */                                       \
    constexpr const uint8_t *seq2s = nullptr;             /* no seq2: unread */                                                \
    __shared__ uint4 wide_prof[WAVES * kProfWave];                                                                              \
    const TileWork slot = work[blockIdx.x];                                                                                     \
    const int len1 = (int)slot.len1, len2 = (int)slot.len2;                                                                     \
    const uint32_t n_trips = (uint32_t)trips(len1);                                                                             \
    (void)cols;                                                                                                                 \
    (void)move_words;                                                                                                           \
    (void)seq2s;

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_profile_local_kernel(
    const uint8_t *__restrict__ seq1s, const uint4 *__restrict__ wide_pssm, int gap_open, int gap_extend,
    int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, const TileWork *__restrict__ work)
{
    SWMI_WIDE_PROFILE_KERNEL_BODY(LocalAffine)
#include "tile_sweep_affine_body.inc"
}

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_profile_global_kernel(
    const uint8_t *__restrict__ seq1s, const uint4 *__restrict__ wide_pssm, int gap_open, int gap_extend, unsigned free_ends,
    int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ counts, const TileWork *__restrict__ work)
{
    SWMI_WIDE_PROFILE_KERNEL_BODY(GlobalAffine)
#include "tile_sweep_affine_body.inc"
}
#undef SWMI_WIDE_PROFILE_KERNEL_BODY

template <int WAVES>
hipError_t fire_profile(WideKind kind, dim3 grid, hipStream_t st, const uint8_t *s1, const uint4 *pssm, int open, int ext,
                        unsigned free_ends, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                        uint32_t *counts, const TileWork *work)
{
    const dim3 block(64 * WAVES);
    if (kind == kWideLocal) {
        if (moves)
            hipLaunchKernelGGL((wide_profile_local_kernel<true, WAVES>), grid, block, 0, st, s1, pssm, open, ext, scores, ends, codes,
                               moves, counts, work);
        else
            hipLaunchKernelGGL((wide_profile_local_kernel<false, WAVES>), grid, block, 0, st, s1, pssm, open, ext, scores, ends,
                               (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work);
    } else {
        if (moves)
            hipLaunchKernelGGL((wide_profile_global_kernel<true, WAVES>), grid, block, 0, st, s1, pssm, open, ext, free_ends, scores,
                               ends, codes, moves, counts, work);
        else
            hipLaunchKernelGGL((wide_profile_global_kernel<false, WAVES>), grid, block, 0, st, s1, pssm, open, ext, free_ends, scores,
                               ends, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work);
    }
    return hipGetLastError();
}

}  // namespace

size_t wide_profile_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

int wide_profile_ragged_waves(int len1, int len2) { return len1 == 0 || len2 == 0 ? 1 : tile::waves(len2); }

hipError_t launch_wide_profile_ragged(WideKind kind, const uint8_t *d_seq1s, const TileWork *d_work, size_t n, int waves,
                                      const void *d_pssm, int pssm_waves, int gap_open, int gap_extend, unsigned free_ends,
                                      int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                      uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    // (a workgroup of `waves` wavefronts reads entries below 64 x waves of each row: the rows must be at least that long)
    if (waves < 1 || waves > kWideMaxWaves || pssm_waves < waves || pssm_waves > kWideMaxWaves || n > (size_t(1) << 20) || free_ends > 15u ||
        !d_pssm || (reinterpret_cast<uintptr_t>(d_pssm) & 15))
        return hipErrorInvalidValue;
    // a launch whose rows are longer than its workgroups are wide may hold zero-length slots only, which read no profile; the
    // kernel's row stride is its own width
    if (pssm_waves != waves && waves != 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n);
    const uint4 *pssm = static_cast<const uint4 *>(d_pssm);
#define SWMI_WIDE_PROFILE_FIRE(W)                                                                                           \
    case W:                                                                                                                 \
        return fire_profile<W>(kind, grid, stream, d_seq1s, pssm, gap_open, gap_extend, free_ends, d_scores, d_ends, d_codes, d_moves, \
                               d_steps, d_work)
    switch (waves) {
        SWMI_WIDE_PROFILE_FIRE(1);
        SWMI_WIDE_PROFILE_FIRE(2);
        SWMI_WIDE_PROFILE_FIRE(3);
    default:
        SWMI_WIDE_PROFILE_FIRE(4);
    }
#undef SWMI_WIDE_PROFILE_FIRE
}

}  // namespace swmi
