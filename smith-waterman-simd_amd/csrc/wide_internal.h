// wide_internal.h -- what wide_affine_kernels.hip and wide_api.cpp (libswmi_wide.so, include/swmi_wide.h, and
// libswmi_wide_long.so, which links the same kernels) share.  Nothing here or in those two files knows the Context of libswmi.so.
#pragma once
#include "swmi_internal.h"

namespace swmi {

enum WideKind { kWideLocal = 0, kWideGlobal = 1, kWideKinds };

constexpr int kWideMaxWaves = 4;            // wave counts of a slot: 1 .. 4
constexpr int kWideMaxLen1 = 16384;
constexpr int kWideMaxLen2 = 4096;          // 4 wavefronts x 64 lanes x 16 columns: what the profile's LDS allows

// qwords of codes of one alignment of two non-zero lengths (the 4-letter affine tile aligners')
size_t wide_affine_code_qwords(int len1, int len2);
// the wave count of a slot's workgroup, 1 .. 4; a slot with a zero length runs in a workgroup of one wavefront
int wide_ragged_waves(int len1, int len2);
// n slots of d_work (device memory), ALL of wave count `waves`: launch_local_full_affine_ragged's and
// launch_global_full_affine_ragged's arguments (kWideLocal ignores free_ends), with d_sm the 32 x 32 matrix in DEVICE memory.
hipError_t launch_wide_affine_ragged(WideKind kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                     int waves, const int8_t *d_sm, int gap_open, int gap_extend, unsigned free_ends,
                                     int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                     uint32_t *d_steps, hipStream_t stream);

}  // namespace swmi
