/* swmi_banded_ragged.h -- C ABI of libswmi_banded_ragged.so: the banded aligners of swmi_banded.h (LOCAL) and
 * swmi_banded_global.h (GLOBAL, FIT, OVERLAP, EXTENSION) on a batch of MIXED (len1, len2) in one call, with a diagonal per
 * alignment.  Those two headers are the definitions of the two kinds and stay as they are; this one only says what a mixed
 * batch is.  DESIGN.md section 37.
 *
 * A library of its own beside libswmi.so, with its siblings' rules:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entries use two streams of their own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_banded_ragged_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_banded_ragged_last_error(), thread-local text.
 *
 * THE BATCH.  Sequences are concatenated, as in swmi_wide.h: alignment k is seq1 = bytes [seq1_offsets[k], seq1_offsets[k+1])
 * of seq1s against seq2 = bytes [seq2_offsets[k], seq2_offsets[k+1]) of seq2s; both offset arrays hold n + 1 non-decreasing
 * uint64 entries and every length is in [0, 16384] (SWMI_BANDED_RAGGED_MAX_LEN).  diagonals holds one int32 per alignment, NULL
 * means all 0; EVERY int32 value is legal.  One matrix, one pair of gaps and (global kind) one free_ends mask per call.
 *
 * SEMANTICS.  Alignment k of swmi_banded_ragged_local is, field for field and move for move, what swmi_banded_local gives for
 * that pair alone with diagonals[k]; alignment k of swmi_banded_ragged_global is likewise what swmi_banded_global gives under
 * the call's free_ends (0 .. 19, SWMI_BANDED_END_ANYWHERE included).  That covers SWMI_BANDED_NO_ALIGNMENT, a band that misses
 * the table, the first-in-row-major tie rule and the forced border steps.  scores[k], ends[4 k .. 4 k + 3] and steps[k] are in
 * caller order.  Alignment k's moves start at word move_offsets[k] = the sum over m < k of
 * SWMI_LOCAL_FULL_MOVE_WORDS(len1 of m, len2 of m): swmi_local_full_ragged_move_offsets (libswmi.so) gives the layout and
 * swmi_local_full_expand_moves(moves + move_offsets[k], ...) rebuilds a path; there is no second function for either.  Words of
 * an alignment's row past its last step are unspecified; words of other rows are never touched.  moves and steps both NULL:
 * ENDS-ONLY, the start cell reported as (-1, -1).
 *
 * ZERO LENGTHS follow from the two definitions extended to an empty sequence, and NO BYTE OF AN EMPTY SEQUENCE IS READ: a
 * batch whose sequences of one side are all empty may pass a buffer of 0 bytes (the pointer itself must not be NULL).
 *   - Local kind: the table has no interior cell, so the score is 0, ends (0, 0, 0, 0), ends-only (0, 0, -1, -1), 0 steps and
 *     no move word is written.
 *   - Global kind: the table is one border (row 0 for len1 = 0, column 0 for len2 = 0, the cell (0, 0) for both).  Its in-band
 *     cells hold swmi_banded_global.h's border values, the candidates are those of the mask among them, the end cell is the
 *     first best one and the walk is the border rule alone: forced steps to (0, 0) unless the border is free.  A finite
 *     candidate exists only where the band and the mask allow it; else the result is SWMI_BANDED_NO_ALIGNMENT's.
 *
 * ARGUMENTS are checked in this order, before any device is touched: free_ends (global kind; above 19 is
 * SWMI_ERR_INVALID_ARGUMENT), the matrix (NULL: SWMI_ERR_INVALID_ARGUMENT), the gaps (outside [0, 127]: SWMI_ERR_DOMAIN), the
 * moves / steps pair (only one of them given is SWMI_ERR_INVALID_ARGUMENT); then n = 0 (SWMI_OK, no device needed), the buffers
 * (seq1s, seq2s, scores or ends NULL: SWMI_ERR_INVALID_ARGUMENT; diagonals may be NULL), the offsets (NULL, decreasing, or a
 * length above 16384: SWMI_ERR_INVALID_ARGUMENT) and, for the device entries, 16-byte alignment of the device pointers
 * (SWMI_ERR_ALIGNMENT).  Every entry returns SWMI_OK or a negative swmi_status.
 *
 * SLOTS AND SLICES.  The host turns every alignment into a SLOT of SWMI_BANDED_RAGGED_SLOT_BYTES = 48 bytes -- two 64-bit
 * sequence offsets, the 64-bit offsets of its codes and of its moves, the two lengths, the diagonal clamped to +-65536, and the
 * caller index its results go to -- and uploads the slots with the launch.  A call runs in SLICES, contiguous in caller order:
 * each is the longest run of the alignments left whose device bytes fit the fixed entries' budgets, 4 383 801 344 bytes with a
 * traceback and 256 MiB ends-only, at most 2^20 alignments and at least one.  An alignment takes len1 + len2 + 48 (slot) + 20
 * (results) bytes and with a traceback its codes -- 256 ceil((len1 + 63) / 4) bytes for the local kind,
 * 256 ceil((len1 + 64) / 4) for the global kind --, its moves, 8 SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2), and 4 of steps.
 * Inside a slice the slots are ordered by the rows their sweep covers, longest first, so that the four wavefronts of a
 * workgroup carry similar work; results still go to caller positions.
 *
 * KNOWN LIMITS: a band of 128 diagonals; 4 letters; lengths up to 16384; one mask, one matrix and one pair of gaps per call;
 * the cell and the walk are the fixed kernels', not tuned again; the three banded kernel files and the two banded host sources
 * are separate. */
#ifndef SWMI_BANDED_RAGGED_H
#define SWMI_BANDED_RAGGED_H

#include <stdint.h>

#include "swmi.h"
#include "swmi_banded.h"
#include "swmi_banded_global.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_BANDED_RAGGED_LOCAL 0
#define SWMI_BANDED_RAGGED_GLOBAL 1
#define SWMI_BANDED_RAGGED_MAX_LEN 16384
#define SWMI_BANDED_RAGGED_SLOT_BYTES 48

SWMI_API const char *swmi_banded_ragged_last_error(void);
SWMI_API int swmi_banded_ragged_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_banded_ragged_release_workspaces(void);

/* Host buffers: seq1s, seq2s (concatenated), the two offset arrays (n + 1 entries each), diagonals (n int32, or NULL),
 * scores[n], ends[4 n]; moves (move_offsets[n] words) and steps[n], or both NULL for ends-only.  The batch runs in slices
 * (swmi_banded_ragged_slices_for) on two sets of device buffers, one slice's copies beside the other's kernel. */
SWMI_API int swmi_banded_ragged_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                      size_t n, const int32_t *diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                      int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_banded_ragged_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                       size_t n, const int32_t *diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                       unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);

/* The same with the SEQUENCE AND RESULT buffers in device memory of the current device, 16-byte aligned; asynchronous on
 * `stream`.  UNLIKE THE FIXED DEVICE ENTRIES (swmi_banded_local_device, swmi_banded_global_device), which take their
 * diagonals in device memory, these take the two offset arrays AND THE DIAGONALS IN HOST MEMORY, like score_matrix, all read
 * before the call returns: the host builds the slots, diagonal included, and uploads them on `stream` in front of the
 * launches.  The traceback codes and the slots go to a workspace of the library's per (device, stream), grown on demand and
 * kept until swmi_banded_ragged_release_workspaces(). */
SWMI_API int swmi_banded_ragged_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                             const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals,
                                             const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                             void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_banded_ragged_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                              const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals,
                                              const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                              void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* The slices a call of `kind` (SWMI_BANDED_RAGGED_LOCAL / _GLOBAL) cuts its batch into (traceback = 0: ends-only), in order;
 * returns how many there are and writes the first `cap` sizes (NULL to count).  The arithmetic is the one stated above.  Needs
 * no device.  0 for n = 0, an unknown kind or offsets that the aligning entries refuse. */
SWMI_API size_t swmi_banded_ragged_slices_for(int kind, const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int traceback,
                                              size_t *sizes, size_t cap);

/* Measurement helper: one untimed device call of `kind` (free_ends is ignored by the local kind), then `iters` of them back
 * to back on `stream`, bracketed by HIP events; *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_banded_ragged_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                            const uint64_t *seq2_offsets, size_t n, const int32_t *diagonals,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                            void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                            float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_BANDED_RAGGED_H */
