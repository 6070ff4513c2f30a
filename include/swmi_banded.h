/* swmi_banded.h -- C ABI of libswmi_banded.so: LOCAL alignment with AFFINE gaps restricted to a BAND of 128 diagonals, with
 * end cell, start cell and traceback or ends-only, for two lengths up to 16384 and a band that need not sit on the main
 * diagonal.  It is what swmi_score_banded_affine (swmi.h, a score only, one equal length up to 1792) lacks; that entry is
 * untouched.  DESIGN.md section 33.
 *
 * A library of its own beside libswmi.so, with libswmi_wide.so's rules:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entry uses two streams of its own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_banded_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_banded_last_error(), thread-local text.
 *
 * SEMANTICS.  n alignments; seq1 k = the len1 bytes at seq1s + len1 * k, seq2 k = the len2 bytes at seq2s + len2 * k, one
 * (len1, len2) per call, 1 <= len1, len2 <= 16384 (SWMI_BANDED_MAX_LEN).  Bases are taken modulo 4; any int8[16] matrix;
 * gap_open and gap_extend each in [0, 127], in either order; a gap of length k costs gap_open + (k-1) gap_extend.
 * diagonals holds one int32 per alignment, NULL means all 0; EVERY int32 value is legal.  Cell (i, j) is IN THE BAND of
 * alignment k iff  -64 <= (j - i) - diagonals[k] <= 63.  For in-band cells with 1 <= i <= len1 and 1 <= j <= len2, in
 * swmi_local_align_affine's convention (E vertical, F horizontal):
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)      up move
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)      left move
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 * Every cell that is out of the band or on the border has H = 0 and E = F = -infinity (what oracle/sw_oracle.c's
 * sw_oracle_banded_affine does).  scores[k] = max H, at most 127 * min(len1, len2) < 2^21.  ends[k] = (end_i, end_j, start_i,
 * start_j): the end cell is the first in-band cell in row-major order that holds the score, (0, 0) when the score is 0.  The
 * walk, its tie rules (diagonal, then E, then F; opening wins a tie), the move encoding (3 = diagonal, 2 = up, 1 = left, in
 * walking order, step t at bits 2 (t % 32) of word t / 32) and ends[4] are those of swmi_local_full_affine (swmi.h), word for
 * word; the walk cannot leave the band, because an out-of-band neighbour contributes at most -open <= 0 and state H stops at
 * H = 0 first.  moves + k * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) receives alignment k's steps and steps[k] their number; a
 * path is rebuilt by swmi_local_full_expand_moves (libswmi.so): there is no second expander.  moves and steps both NULL:
 * ENDS-ONLY -- no codes are stored or walked, the start cell is reported as (-1, -1).  A band that misses the table gives
 * score 0, ends (0, 0, 0, 0) and 0 steps, ends-only (0, 0, -1, -1).
 *
 * Ties to the other entries: with len1 = len2 in [64, 1792] and diagonals NULL, scores equals swmi_score_banded_affine's;
 * where swmi_local_full_affine's path stays inside the band every field and move equals that entry's (banded H <= full H cell
 * by cell, with equality along a path that lies in the band); with gap_open = gap_extend = g the same holds against
 * swmi_local_full with gap g.
 *
 * ARGUMENTS are checked in swmi_wide.h's order, before any device is touched: the matrix (NULL) and the gaps
 * (SWMI_ERR_DOMAIN outside [0, 127]), the moves / steps pair (only one of them given is SWMI_ERR_INVALID_ARGUMENT); then n = 0
 * (SWMI_OK, no device needed), the buffers (a NULL one is SWMI_ERR_INVALID_ARGUMENT; diagonals may be NULL) and the lengths
 * (outside [1, 16384]: SWMI_ERR_INVALID_ARGUMENT).  Device pointers must be 16-byte aligned, else SWMI_ERR_ALIGNMENT.  Every
 * entry returns SWMI_OK or a negative swmi_status.  KNOWN LIMITS: one (len1, len2) per call; 4 letters; a band of 128
 * diagonals; local alignment only. */
#ifndef SWMI_BANDED_H
#define SWMI_BANDED_H

#include "swmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_BANDED_MAX_LEN 16384
#define SWMI_BANDED_WIDTH 128          /* diagonals -64 .. 63 around diagonals[k] */

SWMI_API const char *swmi_banded_last_error(void);
SWMI_API int swmi_banded_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_banded_release_workspaces(void);

/* Host buffers: seq1s (n * len1 bytes), seq2s (n * len2), diagonals (n int32, or NULL), scores[n], ends[4 n]; moves
 * (n * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) words) and steps[n], or both NULL for ends-only.  The batch runs in SLICES
 * (swmi_banded_slices_for) on two sets of device buffers, one slice's copies beside the other's kernel. */
SWMI_API int swmi_banded_local(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int32_t *diagonals,
                               const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                               uint64_t *moves, uint32_t *steps);

/* The same with every buffer in device memory of the current device, d_diagonals included (or NULL), 16-byte aligned;
 * score_matrix is host memory, read before the call returns; asynchronous on `stream`.  The traceback codes
 * (64 bytes per iteration of the sweep, at most 64 (len1 + 66) per alignment) go to a workspace of the library's per
 * (device, stream), grown on demand up to one slice and kept until swmi_banded_release_workspaces(). */
SWMI_API int swmi_banded_local_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                      const void *d_diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                      void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* The slices a call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns how many there are and
 * writes the first `cap` sizes (NULL to count).  With a traceback a slice's device bytes stay within
 * swmi_local_affine_slices_for's budget (what 4096 alignments of len1 = 16384 take there, 4 383 801 344 bytes), ends-only
 * within 256 MiB; at most 2^20 alignments per slice and at least one.  An alignment takes len1 + len2 + 4 (diagonal) + 20
 * (results) bytes and with a traceback its codes, 256 ceil((len1 + 63) / 4), its moves and 4 of steps.  Needs no device.  0 for
 * a length outside [1, 16384]. */
SWMI_API size_t swmi_banded_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);

/* Measurement helper: one untimed swmi_banded_local_device call, then `iters` of them back to back on `stream`, bracketed by
 * HIP events; *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_banded_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const void *d_diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                     void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                     float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_BANDED_H */
