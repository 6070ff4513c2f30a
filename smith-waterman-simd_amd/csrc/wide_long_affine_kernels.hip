// wide_long_affine_kernels.hip -- gfx950 kernels of the LONG wide-alphabet aligners (libswmi_wide_long.so,
// include/swmi_wide_long.h): wide_affine_kernels.hip's two kinds -- local, and global / fit / overlap by
// the free_ends mask, affine gaps, 32 letters, a caller-supplied 32 x 32 int8 matrix, mixed (len1, len2) in one launch, end
// cell, start cell and traceback or ends-only -- for 1 <= len1, len2 <= 65536.
//
// Semantics: wide_affine_kernels.hip's, cell for cell.  The kernels are tile_sweep_affine_body.inc with the variants
// LocalAffine and GlobalAffine and with three of the body's seams at once, which no other kernel combines: WIDE (the score
// profile in LDS), RAGGED (one TileWork per workgroup) and STRIPED (column stripes, DESIGN.md sections 23 and 25).
//
// Mapping: one workgroup of WAVES wavefronts per alignment, WAVES in {1, 4} whatever len2.  It sweeps
// ceil(len2 / kStripeCols) stripes of kStripeCols = 1024 WAVES columns one after another.  In a stripe lane l of wave w owns
// the 16 columns of the global lane G = stripe * (kStripeCols / 16) + 64 w + l; the profile (32 KiB a wave) is rebuilt at the
// head of every stripe, each lane its own 16 bytes of all 32 letter rows, read back by no other lane, so it needs no barrier;
// the last column's (H, F) of every row goes through the slot's carry block in device memory to the next stripe's wave 0, as
// in local_long_affine_kernels.hip.  A wave with no column in the last stripe does no chunk of work and meets every barrier
// (my_chunks = 0).  Code words keep code_index's layout over the GLOBAL wave G >> 6, so the codes, the staged walk and the
// moves do not depend on WAVES.  The walk's staging block lies where wave 0's profile lay and is first written behind the
// last stripe's last barrier.
//
// What this file shadows: WIDE, RAGGED, STRIPED; kStripeCols = 1024 WAVES; kMaxWaves = max(WAVES, 2) (the ring cannot be an empty array), which sizes the ring
// and the reduction's words only (the body takes a stripe's lanes from kStripeCols); kEndBias = 2^24; wide_prof.  It names
// wide_sm, carry_hf and carry_stride: a slot of more than one stripe owns the len1 int2 at carry_hf + slot.pad * carry_stride.
// Slots of one launch differ in len1, so `k * len1` of the fixed-shape striped kernels would overlap.  A slot of one stripe
// (len1 > 16384 with a short seq2) never touches the carry.
//
// Carry ordering and BARRIER INVARIANT: local_long_kernels.hip's argument with W = WAVES for 16.  Wave 0 reads row i's entry at
// its step i - 1, chunk (i - 1) / 32; wave W - 1 overwrites it at its step i + 62, chunk 3 (W - 1) + (i + 62) / 32, which is a
// later chunk for every W >= 1 (63 steps are more than a chunk), behind a barrier for W > 1 and behind the use of the loaded
// value in program order for W = 1, where the chunk loop holds no barrier.  The next stripe reads behind s_waitcnt vmcnt(0),
// the workgroup barrier and the agent-scope acquire fence.  Every wave executes total_chunks + 1 barriers in every stripe but
// the last and total_chunks in the last (for W = 1: one and none), total_chunks made of len1 and blockDim alone.  The carry
// is written with vector stores and read with per-lane vector loads.
//
// Key range, restated for matrices that may hold -128 (wide_affine_kernels.hip restates section 18's, this file sections 23's
// and 25's).
//   Global kind, under the DOMAIN RULE P (len1 + len2) <= 2^23 with P = max(1, max |matrix|, gap_open, gap_extend), which the
// host checks per alignment: a valid cell (i, j) is reached by a path of at most i + j moves of magnitude at most P each, so
// |H| <= P (len1 + len2) <= 2^23 -- P is 128 for a matrix that holds -128, and then len1 + len2 <= 65536.  A column past len2
// is computed only by a wave that also holds a valid column of the last stripe, so at most 1023 columns far, with every
// diagonal at -128: it is at most the largest valid cell above or left of it and at least H(i, len2) less one gap run,
// >= -2^23 - 127 * 1023.  So a key H << 6 lies below 2^29 + 2^23 in magnitude, a candidate (a key plus a score or less a gap)
// below 2^30; kMinusInf = -2^30 loses every max it should lose and is extended once at most before an open candidate
// replaces it: -2^30 - 127 * 64 > -2^31.  The reduction packs H + kEndBias with kEndBias = 2^24: positive, below 2^30, above
// two 17-bit fields that hold 65536.  The unstriped kernels' 2^22 would not do, which is why every alignment with len1 >
// 16384 runs here even where its seq2 is one stripe.  The end rule masks columns past len2 out.
//   Local kind: NO rule.  0 <= H <= 127 * 65536 < 2^23: a matrix entry of -128 only lowers a candidate and the floor is 0.
// Every computed E and F is rebuilt from H's open term in its own cell, so it is at least -127 and at most H's bound.
// A padded cell above 0 is at most some valid cell earlier in row-major order, in this or an earlier stripe (every gap costs
// >= 0, a padded diagonal costs 128), and that cell wins the pack's comparison (H desc, row asc, column asc); the per-stripe
// fold in LDS keeps the first cell over all stripes.  Padded columns feed only padded columns, never the carry, and the
// walk never enters one.
#include "global_full_affine_variant.h"
#include "local_full_affine_variant.h"
#include "wide_long_internal.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's LDS budget and bounds were written against (tile_sweep.h owns it)
static_assert(tile::kCols == 16 && tile::kUnroll == 4 && tile::kChunk == 32 && tile::kDelay == 3 && tile::kRing == 256 &&
              tile::kStageRows == 128);

constexpr int kProfWave = 32 * 64;                 // uint4 per wave: 32 KiB, the size of a staging block of the walk
static_assert(kProfWave * sizeof(uint4) == tile::kStageRows * 32 * sizeof(unsigned long long));

// A uniform pointer held in a VGPR pair instead of an SGPR pair (opaque_lane, tile_sweep.h).  The slot, ten pointers and the
// stripe loop's state are more uniform values than the traceback kernel of the global kind has SGPRs for: the compiler spilled
// 14 of them into VGPR lanes.  With at most 256 threads a workgroup has VGPRs to spare, so the pointers that are read only
// through per-lane addresses (the matrix and seq2, in the profile build and row 0 of every stripe; the codes and the carry) or once
// behind the sweep (the results) live there from the start, and nothing spills.
template <class T>
__device__ __forceinline__ T *in_vgprs(T *p)
{
    const unsigned long long u = reinterpret_cast<unsigned long long>(p);
    const uint32_t lo = (uint32_t)opaque_lane<true>((int)(uint32_t)u), hi = (uint32_t)opaque_lane<true>((int)(uint32_t)(u >> 32));
    return reinterpret_cast<T *>((unsigned long long)hi << 32 | lo);
}

#define SWMI_WIDE_LONG_KERNEL_BODY(VARIANT)                                                                                     \
    using V = VARIANT;                                                                                                          \
    const uint8_t *const seq2s = in_vgprs(seq2s_u);                                                                             \
    const int8_t *const wide_sm = in_vgprs(wide_sm_u);                                                                          \
    int32_t *const scores = in_vgprs(scores_u), *const ends = in_vgprs(ends_u);                                                 \
    unsigned long long *const moves = in_vgprs(moves_u);                                                                        \
    uint32_t *const counts = in_vgprs(counts_u);                                                                                \
    unsigned long long *const codes = in_vgprs(codes_u);                                                                        \
    int2 *const carry_hf = in_vgprs(carry_hf_u);                                                                                \
    constexpr bool RAGGED = true, WIDE = true, STRIPED = true;                                                                  \
    constexpr int kStripeCols = 64 * tile::kCols * WAVES; /* 1024 columns a wavefront */                                        \
    constexpr int kMaxWaves = WAVES > 1 ? WAVES : 2;      /* sizes the body's ring and reduction words */                      \
    constexpr int kEndBias = 1 << 24;                     /* |H| <= 2^23 (above) */                                             \
    constexpr SmCols cols{};                              /* the 4-letter profile's columns: unread */                         \
    constexpr uint32_t move_words = 0;                    /* a fixed launch's: unread */                                       \
    __shared__ uint4 wide_prof[WAVES * kProfWave];                                                                              \
    const TileWork slot = work[blockIdx.x];                                                                                     \
    const int len1 = (int)slot.len1, len2 = (int)slot.len2;                                                                     \
    const uint32_t n_trips = (uint32_t)trips(len1);                                                                             \
    (void)cols;                                                                                                                 \
    (void)move_words;                                                                                                           \
    (void)kEndBias;

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_long_local_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s_u, const int8_t *__restrict__ wide_sm_u, int gap_open,
    int gap_extend, int32_t *__restrict__ scores_u, int32_t *__restrict__ ends_u, unsigned long long *__restrict__ codes_u,
    unsigned long long *__restrict__ moves_u, uint32_t *__restrict__ counts_u, const TileWork *__restrict__ work, int2 *carry_hf_u,
    uint32_t carry_stride)
{
    SWMI_WIDE_LONG_KERNEL_BODY(LocalAffine)
#include "tile_sweep_affine_body.inc"
}

template <bool TB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void wide_long_global_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s_u, const int8_t *__restrict__ wide_sm_u, int gap_open,
    int gap_extend, unsigned free_ends, int32_t *__restrict__ scores_u, int32_t *__restrict__ ends_u,
    unsigned long long *__restrict__ codes_u, unsigned long long *__restrict__ moves_u, uint32_t *__restrict__ counts_u,
    const TileWork *__restrict__ work, int2 *carry_hf_u, uint32_t carry_stride)
{
    SWMI_WIDE_LONG_KERNEL_BODY(GlobalAffine)
#include "tile_sweep_affine_body.inc"
}
#undef SWMI_WIDE_LONG_KERNEL_BODY

template <int WAVES>
hipError_t fire_wide_long(WideKind kind, dim3 grid, hipStream_t st, const uint8_t *s1, const uint8_t *s2, const int8_t *sm, int open,
                          int ext, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned long long *codes,
                          unsigned long long *moves, uint32_t *counts, const TileWork *work, int2 *carry, uint32_t stride)
{
    const dim3 block(64 * WAVES);
    if (kind == kWideLocal) {
        if (moves)
            hipLaunchKernelGGL((wide_long_local_affine_kernel<true, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, scores, ends,
                               codes, moves, counts, work, carry, stride);
        else
            hipLaunchKernelGGL((wide_long_local_affine_kernel<false, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, scores, ends,
                               (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work, carry, stride);
    } else {
        if (moves)
            hipLaunchKernelGGL((wide_long_global_affine_kernel<true, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, free_ends,
                               scores, ends, codes, moves, counts, work, carry, stride);
        else
            hipLaunchKernelGGL((wide_long_global_affine_kernel<false, WAVES>), grid, block, 0, st, s1, s2, sm, open, ext, free_ends,
                               scores, ends, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, work,
                               carry, stride);
    }
    return hipGetLastError();
}

}  // namespace

size_t wide_long_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_wide_long_affine_ragged(WideKind kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                          int width, const int8_t *d_sm, int gap_open, int gap_extend, unsigned free_ends,
                                          int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                          uint32_t *d_steps, void *d_carry, uint32_t carry_stride, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    // (d_carry may be NULL when no slot of the launch has more than one stripe: none touches it then)
    if (n > (size_t(1) << 20) || free_ends > 15u || !d_sm) return hipErrorInvalidValue;
    const dim3 grid((unsigned)n);
    int2 *carry = static_cast<int2 *>(d_carry);
#define SWMI_WIDE_LONG_FIRE(W)                                                                                                  \
    case W:                                                                                                                     \
        return fire_wide_long<W>(kind, grid, stream, d_seq1s, d_seq2s, d_sm, gap_open, gap_extend, free_ends, d_scores, d_ends, d_codes, \
                                 d_moves, d_steps, d_work, carry, carry_stride)
    switch (width) {
        SWMI_WIDE_LONG_FIRE(1);
        SWMI_WIDE_LONG_FIRE(4);
    default:
        return hipErrorInvalidValue;
    }
#undef SWMI_WIDE_LONG_FIRE
}

}  // namespace swmi
