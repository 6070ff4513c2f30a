/* swmi_wide_long.h -- C ABI of libswmi_wide_long.so: the wide-alphabet aligners of swmi_wide.h (32 letters, a caller-supplied
 * 32 x 32 int8 matrix, affine gaps, local and global / fit / overlap, mixed (len1, len2) in one batch, end cell, start cell and
 * traceback or ends-only) for sequences of up to 65536 letters in BOTH places.  DESIGN.md section 30.
 *
 * A third library beside libswmi.so and libswmi_wide.so, whose entries stay as they are (len2 <= 4096).  Like libswmi_wide.so:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device and on the stream it is given; the
 *     host entries use two streams of their own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_wide_long_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_wide_long_last_error(), thread-local text.
 *
 * SEMANTICS: those of swmi_wide_local* and swmi_wide_global* (swmi_wide.h), field for field -- the recurrence, the tie rules,
 * the end-cell rule, ends[4] and the ends-only (-1, -1), the move encoding, the 16 masks, the zero-length closed forms, and
 *     score_matrix[(seq1[i-1] & 31) * 32 + (seq2[j-1] & 31)]
 * as the substitution score -- for 0 <= len1, len2 <= SWMI_WIDE_LONG_MAX_LEN = 65536 per alignment, mixed freely in one
 * batch.  An alignment with len1 <= 16384 and len2 <= 4096, or with a zero length, runs in the very kernels of
 * libswmi_wide.so; every other one in kernels that sweep seq2 in column stripes.
 *
 * DOMAIN.  Global kind: with P = max(1, max |score_matrix|, gap_open, gap_extend) an alignment is accepted iff
 * P (len1 + len2) <= 2^23, else the call returns SWMI_ERR_INVALID_ARGUMENT before any launch and the text names the first
 * offending alignment (the rule of swmi_global_long*, swmi.h).  Every shape that swmi_wide_global takes passes it.  Local kind:
 * no rule, every int8 matrix at every shape.
 *
 * MOVES: alignment k's words lie at moves + move_offsets[k], move_offsets the running sum of SWMI_LOCAL_LONG_MOVE_WORDS(len1,
 * len2) (swmi.h) from swmi_wide_long_move_offsets, which needs no device (swmi_local_full_ragged_move_offsets refuses a
 * length above 16384); on the shapes of swmi_wide.h the two give the same offsets.  A path is expanded by
 * swmi_local_long_expand_moves of libswmi.so (it needs no device and no swmi_init).  There is no second expander.
 *
 * ARGUMENTS are checked in the order of swmi_wide.h, before any device is touched: the mask, the matrix and the gaps, the
 * moves / steps pair; then n = 0 (SWMI_OK, no device needed), the buffers, the offsets (NULL, decreasing, a length above
 * 65536), and last the global kind's domain rule.  Device pointers must be 16-byte aligned, else SWMI_ERR_ALIGNMENT.
 *
 * STRIPE WIDTH: a striped alignment's workgroup has 1 or 4 wavefronts and sweeps stripes of 1024 columns a wavefront.
 * Results do not depend on the width.  The library's rule: 4 wavefronts for a launch (a slice's striped alignments) of fewer
 * than 1024, else 1.  Measured: 4 wavefronts are 3.6 - 3.9x faster at 256 alignments or fewer, 1
 * wavefront 1.24 - 1.73x faster at 4096 of (1024, 8192); 2 wavefronts won no row and are not built.
 * swmi_wide_long_set_stripe_waves overrides the rule for the process.
 *
 * KNOWN LIMIT: a traceback needs 8 bytes of codes per lane and row of the padded sweep, 2.15 GB for 65536 x 65536, so a
 * traceback slice of that shape holds 16 alignments (as swmi_global_long_affine's does). */
#ifndef SWMI_WIDE_LONG_H
#define SWMI_WIDE_LONG_H

#include "swmi_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_WIDE_LONG_MAX_LEN 65536
#define SWMI_WIDE_LONG_LOCAL 0
#define SWMI_WIDE_LONG_GLOBAL 1

SWMI_API const char *swmi_wide_long_last_error(void);
SWMI_API int swmi_wide_long_version(void);   /* swmi_version()'s */
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_wide_long_release_workspaces(void);
/* The stripe width of every later call of the process: 1 or 4 wavefronts, or 0 = the library's rule (the default).  Any
 * other value: SWMI_ERR_INVALID_ARGUMENT, and the width stays. */
SWMI_API int swmi_wide_long_set_stripe_waves(int waves);
/* move_offsets[0 .. n] of a batch: the running sum of SWMI_LOCAL_LONG_MOVE_WORDS.  Needs no device.
 * SWMI_ERR_INVALID_ARGUMENT for NULL, decreasing offsets or a length above 65536. */
SWMI_API int swmi_wide_long_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, uint64_t *move_offsets);

/* Host arrays, as swmi_wide_local / swmi_wide_global; moves holds swmi_wide_long_move_offsets(...)[n] words.  A batch is cut
 * into slices (swmi_wide_long_slices_for), two of them in flight on two sets of device buffers. */
SWMI_API int swmi_wide_long_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                  size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, int32_t *scores,
                                  int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_wide_long_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                   size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, unsigned free_ends,
                                   int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);

/* Device buffers of the current device, host offset arrays (read before the call returns); asynchronous on `stream`.
 * score_matrix is host memory, read before the call returns. */
SWMI_API int swmi_wide_long_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                         const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                         int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_wide_long_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                          const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                          int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves,
                                          void *d_steps, void *stream);

/* The slices a call cuts its batch into (needs no device): contiguous in caller order, each the longest run whose device
 * bytes fit the budget -- per alignment len1 + len2, 48 of slot, 20 of results, 8 len1 of carry when the striped kernels take
 * it and len2 > 1024, and with a traceback codes, moves and steps; 256 MiB ends-only, with a traceback what 16 alignments of
 * 65536 x 65536 take -- at most 2^20 alignments and at least one.  Returns the number of slices and writes the first `cap`
 * sizes; 0 on offsets that an entry would refuse (text in swmi_wide_long_last_error). */
SWMI_API size_t swmi_wide_long_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int traceback,
                                          size_t *sizes, size_t cap);

/* Average milliseconds of `iters` device calls of kind SWMI_WIDE_LONG_LOCAL or SWMI_WIDE_LONG_GLOBAL (free_ends: the global
 * kind's), after one untimed call; HIP events on `stream`. */
SWMI_API int swmi_wide_long_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                        const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[1024], int gap_open,
                                        int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                        void *stream, int iters, float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_WIDE_LONG_H */
