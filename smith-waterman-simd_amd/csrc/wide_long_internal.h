// wide_long_internal.h -- what wide_long_affine_kernels.hip and wide_api.cpp as compiled for libswmi_wide_long.so
// (include/swmi_wide_long.h, DESIGN.md sections 30 and 31) share beside wide_internal.h, whose unstriped launcher the library
// calls for the shapes of libswmi_wide.so.  libswmi_wide.so's build of wide_api.cpp includes this header too and names
// neither function declared here.
#pragma once
#include "wide_internal.h"

namespace swmi {

constexpr int kWideLongMaxLen = 65536;
// the stripe widths shipped, in wavefronts of 1024 columns (the workgroup's size: 64 x width threads).  2 was measured and won
// no row, so it is not built.
constexpr int kWideLongWidths[] = {1, 4};
constexpr int kWideLongMinWidth = 1;

// Whether the striped kernels take the alignment: everything that libswmi_wide.so's kernels do not (their kEndBias of 2^22
// covers len1 <= 16384 with len2 <= 4096 only); a zero length is a closed form of the unstriped kernels.
inline bool wide_long_striped(size_t len1, size_t len2)
{
    return len1 != 0 && len2 != 0 && (len1 > size_t(kWideMaxLen1) || len2 > size_t(kWideMaxLen2));
}

// qwords of codes of one alignment of two non-zero lengths: code_index's layout over ALL of len2's wavefronts, whatever the
// stripe width (the formula of wide_affine_code_qwords)
size_t wide_long_code_qwords(int len1, int len2);
// n slots of d_work, ALL striped (wide_long_striped), in workgroups of `width` wavefronts that sweep ceil(len2 / (1024 width))
// stripes: launch_wide_affine_ragged's arguments, and the carry: a slot with more than one stripe owns the len1 int2 at
// d_carry + slot.pad * carry_stride (its len1 <= carry_stride); a slot of one stripe touches no carry.
hipError_t launch_wide_long_affine_ragged(WideKind kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                          int width, const int8_t *d_sm, int gap_open, int gap_extend, unsigned free_ends,
                                          int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                          uint32_t *d_steps, void *d_carry, uint32_t carry_stride, hipStream_t stream);

}  // namespace swmi
