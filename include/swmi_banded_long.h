/* swmi_banded_long.h -- C ABI of libswmi_banded_long.so: the banded aligners of swmi_banded_width.h -- LOCAL and GLOBAL / FIT /
 * OVERLAP / EXTENSION on a batch of MIXED (len1, len2), a diagonal per alignment, the BAND'S WIDTH (128, 256, 512 or 1024) per
 * call -- for sequences UP TO 65536 LONG.  swmi_banded_width.h is the definition, argument for argument and field for field;
 * it stays as it is, and this header only says what differs.  DESIGN.md section 41.
 *
 * A library of its own beside libswmi.so, with its siblings' rules: no swmi_init, the calling thread's CURRENT HIP device, its
 * own workspaces per (device, stream) (swmi_banded_long_release_workspaces), its own thread-local last error
 * (swmi_banded_long_last_error).
 *
 * WHAT DIFFERS.
 *   - LENGTHS: 0 <= len1, len2 <= 65536 (SWMI_BANDED_LONG_MAX_LEN); a longer sequence is SWMI_ERR_INVALID_ARGUMENT with the
 *     text "a length above 65536".  For every length up to 16384 each score, end, start, step count and move is what the
 *     entry of the same name in swmi_banded_width.h gives.
 *   - MOVES: alignment k's words lie at moves + move_offsets[k], move_offsets the running sum of
 *     SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) (swmi.h; the formula of SWMI_LOCAL_FULL_MOVE_WORDS) from
 *     swmi_banded_long_move_offsets below, which needs no device (swmi_local_full_ragged_move_offsets refuses a length above
 *     16384).  The values are swmi_wide_long_move_offsets'; no wide library is needed for them.  A path is rebuilt by
 *     swmi_local_long_expand_moves of libswmi.so (no device, no swmi_init).  There is no second expander.
 *   - DIAGONALS: every int32 value is legal, as before.  A band whose diagonal lies beyond +-(65536 + band / 2) touches no
 *     table, and gives what such a band gives in swmi_banded_width.h: score 0 (local kind), SWMI_BANDED_NO_ALIGNMENT (global).
 *
 * Everything else is swmi_banded_width.h's: the band inequality, the two kinds, the masks 0 .. 19, the tie rule (the first
 * cell in row-major order), the moves, the forced border steps, empty sequences, the order of the argument checks (the band
 * first), the slots of 48 bytes, and the slices: contiguous in caller order, each the longest run whose device bytes fit
 * 4 383 801 344 bytes with a traceback and 256 MiB ends-only, at most 2^20 alignments and at least one, an alignment taking
 * len1 + len2 + 48 + 20 bytes and with a traceback (band / 128) * 256 * ceil((len1 + 63 or 64) / 4) of codes,
 * 8 SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) of moves and 4 of steps.  One band-1024 traceback alignment of 65536 x 65536 takes
 * 33 751 112 bytes (local kind), so a slice holds 129 of them.
 *
 * NO DOMAIN RULE.  The kernels compute on plain int32.  With int8 scores, gaps in [0, 127] and lengths up to 65536 a path
 * has at most 65536 diagonal steps and 131072 gap steps, so every finite value lies in [-127 * 131072 - 254, 127 * 65536] =
 * [-16 646 398, 8 323 072].  Minus infinity is -2^29; every value made from it lies within 127 * 131072 + 254 below and
 * 127 * 65536 above it, so it stays below -2^28, the line under which a candidate counts as infeasible, and far above
 * INT32_MIN.  No combination of legal arguments overflows.
 *
 * KNOWN LIMITS: one band width per call, of four; 4 letters; one mask, one matrix and one pair of gaps per call; the walk of a
 * traceback is up to 131072 dependent steps of one wavefront. */
#ifndef SWMI_BANDED_LONG_H
#define SWMI_BANDED_LONG_H

#include <stdint.h>

#include "swmi.h"
#include "swmi_banded.h"
#include "swmi_banded_global.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_BANDED_LONG_LOCAL 0
#define SWMI_BANDED_LONG_GLOBAL 1
#define SWMI_BANDED_LONG_MAX_LEN 65536
#define SWMI_BANDED_LONG_SLOT_BYTES 48
#define SWMI_BANDED_LONG_MIN 128
#define SWMI_BANDED_LONG_MAX 1024

SWMI_API const char *swmi_banded_long_last_error(void);
SWMI_API int swmi_banded_long_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_banded_long_release_workspaces(void);

/* move_offsets[0 .. n] of a batch: the running sum of SWMI_LOCAL_LONG_MOVE_WORDS.  Needs no device.
 * SWMI_ERR_INVALID_ARGUMENT for a NULL pointer or offsets that the aligning entries refuse. */
SWMI_API int swmi_banded_long_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, uint64_t *move_offsets);

/* Host buffers, as swmi_banded_width_local / _global; moves holds swmi_banded_long_move_offsets(...)[n] words. */
SWMI_API int swmi_banded_long_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                    size_t n, const int32_t *diagonals, int band, const int8_t score_matrix[16], int gap_open,
                                    int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_banded_long_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                     size_t n, const int32_t *diagonals, int band, const int8_t score_matrix[16], int gap_open,
                                     int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);

/* As swmi_banded_width_local_device / _global_device. */
SWMI_API int swmi_banded_long_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                           const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                           const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                           void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_banded_long_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                            const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                            void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* As swmi_banded_width_slices_for, with the lengths of this header. */
SWMI_API size_t swmi_banded_long_slices_for(int kind, int band, const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n,
                                            int traceback, size_t *sizes, size_t cap);

/* As swmi_banded_width_time_device. */
SWMI_API int swmi_banded_long_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                          const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals, int band,
                                          const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                          void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                          float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_BANDED_LONG_H */
