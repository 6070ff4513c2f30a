// wide_profile_internal.h -- what wide_profile_kernels.hip and wide_api.cpp as compiled for libswmi_wide_profile.so
// (include/swmi_wide_profile.h) share beside wide_internal.h, of which that build takes the kinds and
// the limits and names no function.
#pragma once
#include "wide_internal.h"

namespace swmi {

// The profile in device memory, lane-ready: letter-major, 32 rows of 64 x waves uint4 (16 bytes), byte jj of entry G of row a
// = profile[(16 G + jj) * 32 + a], and -128 for columns past len2.  waves = max(1, ceil(len2 / 1024)).
constexpr size_t kWideProfileEntryBytes = 16;
inline int wide_profile_waves_of(size_t len2) { return len2 == 0 ? 1 : int((len2 + 1023) / 1024); }
inline size_t wide_profile_device_bytes(size_t len2) { return size_t(32) * 64 * size_t(wide_profile_waves_of(len2)) * kWideProfileEntryBytes; }

// qwords of codes of one alignment of two non-zero lengths (wide_affine_code_qwords' formula)
size_t wide_profile_code_qwords(int len1, int len2);
// the wave count of a slot's workgroup, 1 .. 4; a slot with a zero length runs in a workgroup of one wavefront
int wide_profile_ragged_waves(int len1, int len2);
// n slots of d_work (device memory), ALL of wave count `waves` and ALL of one len2: launch_wide_affine_ragged's arguments
// without a seq2, with d_pssm the profile in DEVICE memory in the form above, 16-byte aligned, its rows 64 x `pssm_waves`
// entries long.  pssm_waves == waves, except in a launch of zero-length slots (waves = 1), which reads no profile.
hipError_t launch_wide_profile_ragged(WideKind kind, const uint8_t *d_seq1s, const TileWork *d_work, size_t n, int waves,
                                      const void *d_pssm, int pssm_waves, int gap_open, int gap_extend, unsigned free_ends,
                                      int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                      uint32_t *d_steps, hipStream_t stream);

}  // namespace swmi
