// banded_internal.h -- what banded_api.cpp (host compiler) and banded_align_kernels.hip (hipcc) of libswmi_banded.so share:
// the launcher and the size of an alignment's traceback codes (include/swmi_banded.h).
#ifndef SWMI_BANDED_INTERNAL_H
#define SWMI_BANDED_INTERNAL_H

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace swmi {
namespace banded {

constexpr int kBandMaxLen = 16384;
constexpr int kBandWidth = 128;             // diagonals -64 .. 63 around diagonals[k]
constexpr int kBandTrip = 4;                // iterations per loop trip: one code dword per lane
constexpr int kBandWalkTrips = 16;          // trips of codes a wavefront's walk window holds in LDS (64 iterations, 4 KiB)

// Bytes of codes per alignment of a traceback launch: one byte per lane and iteration (two cells of 4 bits), a dword per lane
// and trip, len1 + 63 iterations at the most (lane 0 on row 1 .. lane 63 on row len1) rounded up to whole trips.
constexpr size_t band_code_bytes(size_t len1) { return 64 * kBandTrip * ((len1 + 63 + kBandTrip - 1) / kBandTrip); }

// n alignments of one (len1, len2) on `stream`; every pointer is device memory but sm (int8[16], host).  diagonals may be
// NULL (all 0).  codes: n * band_code_bytes(len1) bytes, 16-byte aligned, with moves and steps or NULL with both (ends-only).
// moves rows are move_words uint64.  Checks nothing: the callers have.
hipError_t launch_banded_local(const uint8_t *d_seq1s, int len1, const uint8_t *d_seq2s, int len2, const int32_t *d_diagonals, size_t n,
                               const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned char *d_codes,
                               unsigned long long *d_moves, size_t move_words, uint32_t *d_steps, hipStream_t stream);

// ---- libswmi_banded_global.so (banded_global_kernels.hip, include/swmi_banded_global.h) ----
// Bytes of codes per alignment of a traceback launch of the global kernels: the same layout, but row 0 is swept too (its
// cells are real cells there), so there is one iteration more: lane 0 on row 0 .. lane 63 on row len1, len1 + 64 at the most.
constexpr size_t band_global_code_bytes(size_t len1) { return 64 * kBandTrip * ((len1 + 64 + kBandTrip - 1) / kBandTrip); }

// As launch_banded_local, with free_ends (SWMI_FREE_* | SWMI_BANDED_END_ANYWHERE, checked by the caller) and codes of
// n * band_global_code_bytes(len1) bytes.
hipError_t launch_banded_global(const uint8_t *d_seq1s, int len1, const uint8_t *d_seq2s, int len2, const int32_t *d_diagonals, size_t n,
                                const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                unsigned char *d_codes, unsigned long long *d_moves, size_t move_words, uint32_t *d_steps,
                                hipStream_t stream);

// ---- libswmi_banded_ragged.so (banded_ragged_kernels.hip, include/swmi_banded_ragged.h) ----
// One alignment of a mixed-shape launch.  off1 / off2: bytes from the launch's seq1s / seq2s; code_off: dwords from its codes;
// move_off: words from its moves; d0: the caller's diagonal clamped to +-kRaggedDiagClamp; index: where its results go in the
// launch's scores / ends / steps.  48 bytes, so a slot is three 16-byte loads.
struct RaggedSlot {
    uint64_t off1, off2, code_off, move_off;
    int32_t len1, len2, d0;
    uint32_t index;
};
static_assert(sizeof(RaggedSlot) == 48);
constexpr int kRaggedLocal = 0, kRaggedGlobal = 1;
constexpr int kRaggedDiagClamp = 65536;

constexpr size_t ragged_code_bytes(int kind, size_t len1) { return kind == kRaggedGlobal ? band_global_code_bytes(len1) : band_code_bytes(len1); }

// n slots on `stream`; every pointer is device memory but sm (int8[16], host).  codes: 16-byte aligned, with moves and steps
// or NULL with both (ends-only).  free_ends is the global kind's.  Checks nothing: the callers have.
hipError_t launch_banded_ragged(int kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n,
                                const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);

// ---- libswmi_banded_width.so (banded_width_kernels.hip, include/swmi_banded_width.h) ----
// A band of `band` diagonals, -band / 2 .. band / 2 - 1 around the alignment's, one width per launch.  A lane owns band / 64
// diagonals, so an iteration of a lane is band / 128 code bytes where the 128-wide kernels store one.
constexpr bool width_is_legal(int band) { return band == 128 || band == 256 || band == 512 || band == 1024; }

constexpr size_t width_code_bytes(int kind, size_t len1, int band) { return size_t(band / kBandWidth) * ragged_code_bytes(kind, len1); }

// The planner's key at a width, of both libraries (the ragged one's at kBandWidth): i_hi - i_lo of the kind's kernel for a
// clamped diagonal, 0 for a band that misses the table or an empty sequence.  From -band/2 <= j - i - d0 <= band/2 - 1 with
// 1 <= j <= len2 (local: interior cells) or 0 <= j <= len2 (global: row 0 and column 0 are cells):
//   i >= j - d0 - band/2 + 1  at the smallest j:  local  i_lo = max(1, 2 - band/2 - d0),  global  i_lo = max(0, 1 - band/2 - d0)
//   i <= j - d0 + band/2      at j = len2:        i_hi = min(len1, len2 + band/2 - d0)
constexpr int width_swept_rows(int kind, int len1, int len2, int d0, int band)
{
    if (len1 == 0 || len2 == 0) return 0;
    const int half = band / 2;
    const int lo_min = kind == kRaggedGlobal ? 0 : 1, lo_band = (kind == kRaggedGlobal ? 1 : 2) - half - d0;
    const int i_lo = lo_min > lo_band ? lo_min : lo_band, i_hi = len1 < len2 + half - d0 ? len1 : len2 + half - d0;
    return i_lo > i_hi ? 0 : i_hi - i_lo;
}

// As launch_banded_ragged, with the band's width (checked by the caller) and an alignment's codes at code_off dwords taking
// width_code_bytes(kind, len1, band).
hipError_t launch_banded_width(int kind, int band, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n,
                               const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                               unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);

// ---- libswmi_banded_long.so (banded_long_kernels.hip, include/swmi_banded_long.h) ----
// The width library's slots, codes and key for lengths up to kBandLongMaxLen.  Beyond +-(65536 + 512) no band touches a table,
// so a diagonal clamped at +-kLongDiagClamp gives what the caller's gives.
constexpr int kBandLongMaxLen = 65536;
constexpr int kLongDiagClamp = 131072;

// As launch_banded_width.
hipError_t launch_banded_long(int kind, int band, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n,
                              const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                              unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);

}  // namespace banded
}  // namespace swmi

#endif
