/* swmi_wide.h -- C ABI of libswmi_wide.so: local and global / fit / overlap alignment with AFFINE gaps over an alphabet of
 * 32 LETTERS and a caller-supplied 32 x 32 int8 substitution matrix (protein search, DNA with N or the IUPAC codes, any
 * caller with more than four symbols), on a batch of MIXED (len1, len2), with end cell, start cell and traceback or
 * ends-only.  DESIGN.md section 29.
 *
 * A library of its own beside libswmi.so, which it links for the two public functions named below and for nothing else:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entries use two streams of their own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_wide_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_wide_last_error(), thread-local text; swmi_last_error() says nothing about these calls.
 *
 * SEMANTICS: those of swmi_local_full_affine_ragged* (swmi_wide_local*) and swmi_global_full_affine_ragged*
 * (swmi_wide_global*) of swmi.h, field for field -- the recurrences, the tie rules, the end-cell rule (H descending, row
 * ascending, column ascending), ends[4] = (end_i, end_j, start_i, start_j), the ends-only start (-1, -1), the move encoding
 * and the move layout, the zero-length closed forms -- with ONE difference: the substitution score of cell (i, j) is
 *     score_matrix[(seq1[i-1] & 31) * 32 + (seq2[j-1] & 31)]
 * with score_matrix an int8[1024], row-major; every int8 value is allowed, and only the low five bits of a sequence byte
 * are read.  gap_open and gap_extend lie in [0, 127], else SWMI_ERR_DOMAIN; free_ends is a mask of SWMI_FREE_* (swmi.h),
 * at most SWMI_ENDS_OVERLAP = 15, else SWMI_ERR_INVALID_ARGUMENT.
 *
 * LENGTHS: 0 <= len1 <= SWMI_WIDE_MAX_LEN1 = 16384 and 0 <= len2 <= SWMI_WIDE_MAX_LEN2 = 4096 per alignment; a longer one
 * is SWMI_ERR_INVALID_ARGUMENT.  KNOWN LIMIT: the asymmetry is the kernels' score profile, which holds 32 KiB of LDS per
 * 1024 columns of seq2; callers put the shorter sequence second.  (Column stripes, as the *_long kernels of swmi.h sweep
 * them, are the way to lift it.)  A zero length gives exactly what the 4-letter entries give, and no sequence byte is read.
 *
 * MOVES: alignment k's words lie at moves + move_offsets[k], move_offsets from swmi_local_full_ragged_move_offsets (swmi.h,
 * libswmi.so; it needs no device and no swmi_init); a path is expanded by swmi_local_full_expand_moves (likewise).  There
 * is no second function for either.
 *
 * ARGUMENTS are checked in the order of the 4-letter ragged entries, before any device is touched: the mask, the matrix and
 * the gaps, the moves / steps pair (only one of them given is an error); then n = 0 (SWMI_OK, no device needed), the
 * buffers, and the offsets (NULL, decreasing, a length above the limit).  Device pointers must be 16-byte aligned, else
 * SWMI_ERR_ALIGNMENT.  Every entry returns SWMI_OK or a negative swmi_status. */
#ifndef SWMI_WIDE_H
#define SWMI_WIDE_H

#include "swmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_WIDE_LETTERS 32
#define SWMI_WIDE_MAX_LEN1 16384
#define SWMI_WIDE_MAX_LEN2 4096
#define SWMI_WIDE_LOCAL 0
#define SWMI_WIDE_GLOBAL 1

SWMI_API const char *swmi_wide_last_error(void);
SWMI_API int swmi_wide_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_wide_release_workspaces(void);

/* Host arrays: seq1s / seq2s concatenated, seq1_offsets / seq2_offsets of n + 1 entries each; scores[n], ends[4 n];
 * moves (swmi_local_full_ragged_move_offsets(...)[n] words) and steps[n], or both NULL for ends-only.  A batch is cut
 * into slices (swmi_wide_slices_for), two of them in flight on two sets of device buffers. */
SWMI_API int swmi_wide_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                             size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, int32_t *scores,
                             int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_wide_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                              size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, unsigned free_ends,
                              int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);

/* Device buffers of the current device, host offset arrays (read before the call returns); asynchronous on `stream`.
 * score_matrix is host memory, read before the call returns. */
SWMI_API int swmi_wide_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                    const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                    int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_wide_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                     const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                     int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves,
                                     void *d_steps, void *stream);

/* The slices a call cuts its batch into (needs no device): contiguous in caller order, each the longest run whose device
 * bytes (inputs, slots, results; with a traceback codes, moves and steps) fit the budget -- 256 MiB ends-only, with a
 * traceback what 256 alignments of 16384 x 4096 take -- at most 2^20 alignments and at least one.  Returns the number of
 * slices and writes the first `cap` sizes; 0 on offsets that an entry would refuse (text in swmi_wide_last_error). */
SWMI_API size_t swmi_wide_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int traceback,
                                     size_t *sizes, size_t cap);

/* Average milliseconds of `iters` device calls of kind SWMI_WIDE_LOCAL or SWMI_WIDE_GLOBAL (free_ends: the global kind's),
 * after one untimed call; HIP events on `stream`. */
SWMI_API int swmi_wide_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                   const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                   int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                   void *stream, int iters, float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_WIDE_H */
