/* swmi_banded_width.h -- C ABI of libswmi_banded_width.so: the banded aligners of swmi_banded.h (LOCAL) and
 * swmi_banded_global.h (GLOBAL, FIT, OVERLAP, EXTENSION) on a batch of MIXED (len1, len2), as swmi_banded_ragged.h runs them,
 * with the BAND'S WIDTH given per call: 128, 256, 512 or 1024 diagonals.  The two fixed headers are the definitions of the two
 * kinds and swmi_banded_ragged.h the definition of a mixed batch; all three stay as they are, and this one only says what
 * `band` is.  DESIGN.md section 38.
 *
 * A library of its own beside libswmi.so, with its siblings' rules:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entries use two streams of their own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_banded_width_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_banded_width_last_error(), thread-local text.
 *
 * THE BAND.  `band` is one of 128, 256, 512, 1024 (SWMI_BANDED_WIDTH_MIN .. SWMI_BANDED_WIDTH_MAX, powers of two); any other
 * value is SWMI_ERR_INVALID_ARGUMENT.  Cell (i, j) of alignment k is in the band iff
 *     -band / 2  <=  (j - i) - diagonals[k]  <=  band / 2 - 1.
 * Everything else is the two definitions with 64 read as band / 2: outside the band H = 0 and E = F = -infinity for the local
 * kind and all three -infinity for the global kind; the border cells of the global kind, where (0, 0) is in the band iff
 * -band / 2 + 1 <= diagonals[k] <= band / 2; the first-in-row-major tie rule, SWMI_BANDED_NO_ALIGNMENT, the forced border
 * steps, and empty sequences, of which no byte is read.  With band = 128 every field and every move up to `steps` is what the
 * entry of the same name in swmi_banded_ragged.h gives.  One width serves the whole call.
 *
 * THE BATCH, the results, the layout of the moves (swmi_local_full_ragged_move_offsets, swmi_local_full_expand_moves of
 * libswmi.so; there is no second function for either) and the zero lengths are swmi_banded_ragged.h's, argument for argument:
 * each aligning entry takes that header's arguments and `band` directly before score_matrix.  diagonals is host memory, may
 * be NULL (all 0), and every int32 value is legal.  moves and steps both NULL: ENDS-ONLY, the start cell reported as (-1, -1).
 *
 * ARGUMENTS are checked in this order, before any device is touched: band (not 128, 256, 512 or 1024:
 * SWMI_ERR_INVALID_ARGUMENT), then swmi_banded_ragged.h's order: free_ends (global kind; above 19), the matrix, the gaps, the
 * moves / steps pair; then n = 0 (SWMI_OK, no device needed), the buffers, the offsets and, for the device entries, 16-byte
 * alignment of the device pointers.  Every entry returns SWMI_OK or a negative swmi_status.
 *
 * SLOTS AND SLICES are swmi_banded_ragged.h's with the codes of the width: a call runs in slices, contiguous in caller order,
 * each the longest run of the alignments left whose device bytes fit 4 383 801 344 bytes with a traceback and 256 MiB
 * ends-only, at most 2^20 alignments and at least one.  An alignment takes len1 + len2 + 48 (slot) + 20 (results) bytes and
 * with a traceback its codes, its moves, 8 SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2), and 4 of steps.  The codes are 4 bits per
 * cell of a lane's band / 64 diagonals, band / 128 bytes per lane and iteration, so
 *     (band / 128) * 256 * ceil((len1 + 63) / 4) bytes for the local kind,
 *     (band / 128) * 256 * ceil((len1 + 64) / 4) bytes for the global kind:
 * band / 128 times swmi_banded_ragged.h's.  Inside a slice the slots are ordered by the rows their sweep covers at the
 * call's width, longest first; results go to caller positions.
 *
 * KNOWN LIMITS: one band width per call, of four; 4 letters; lengths up to 16384; one mask, one matrix and one pair of gaps
 * per call. */
#ifndef SWMI_BANDED_WIDTH_H
#define SWMI_BANDED_WIDTH_H

#include <stdint.h>

#include "swmi.h"
#include "swmi_banded.h"
#include "swmi_banded_global.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_BANDED_WIDTH_LOCAL 0
#define SWMI_BANDED_WIDTH_GLOBAL 1
#define SWMI_BANDED_WIDTH_MAX_LEN 16384
#define SWMI_BANDED_WIDTH_SLOT_BYTES 48
#define SWMI_BANDED_WIDTH_MIN 128
#define SWMI_BANDED_WIDTH_MAX 1024

SWMI_API const char *swmi_banded_width_last_error(void);
SWMI_API int swmi_banded_width_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_banded_width_release_workspaces(void);

/* Host buffers, as swmi_banded_ragged_local / _global, with the band's width before the matrix. */
SWMI_API int swmi_banded_width_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                     size_t n, const int32_t *diagonals, int band, const int8_t score_matrix[16], int gap_open,
                                     int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_banded_width_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                      size_t n, const int32_t *diagonals, int band, const int8_t score_matrix[16], int gap_open,
                                      int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);

/* The same with the SEQUENCE AND RESULT buffers in device memory of the current device, 16-byte aligned; asynchronous on
 * `stream`.  The two offset arrays and the diagonals are HOST memory, read before the call returns, as in
 * swmi_banded_ragged.h.  The traceback codes and the slots go to a workspace of the library's per (device, stream), grown on
 * demand and kept until swmi_banded_width_release_workspaces(). */
SWMI_API int swmi_banded_width_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                            const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                            void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_banded_width_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                             const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                             const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                             void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* The slices a call of `kind` (SWMI_BANDED_WIDTH_LOCAL / _GLOBAL) at width `band` cuts its batch into (traceback = 0:
 * ends-only), in order; returns how many there are and writes the first `cap` sizes (NULL to count).  The arithmetic is the one
 * stated above.  Needs no device.  0 for n = 0, an unknown kind, an illegal band or offsets that the aligning entries refuse. */
SWMI_API size_t swmi_banded_width_slices_for(int kind, int band, const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n,
                                             int traceback, size_t *sizes, size_t cap);

/* Measurement helper: one untimed device call of `kind` (free_ends is ignored by the local kind), then `iters` of them back
 * to back on `stream`, bracketed by HIP events; *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_banded_width_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                           const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                           const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                           void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                           float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_BANDED_WIDTH_H */
