/* swmi_banded_global.h -- C ABI of libswmi_banded_global.so: GLOBAL, FIT, OVERLAP and EXTENSION alignment with AFFINE gaps
 * restricted to a BAND of 128 diagonals, with end cell, start cell and traceback or ends-only, for two lengths up to 16384 and
 * a band that need not sit on the main diagonal.  It is swmi_banded_local (swmi_banded.h) with NO ZERO FLOOR, under
 * swmi_global_full_affine's free_ends mask plus one end rule more; swmi_banded.h's entries are untouched.  DESIGN.md section 34.
 * This header is the definition: there is no reference counterpart.
 *
 * A library of its own beside libswmi.so, with libswmi_banded.so's rules:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entry uses two streams of its own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_banded_global_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_banded_global_last_error(), thread-local text.
 *
 * UNCHANGED FROM swmi_banded_local.  n alignments; seq1 k = the len1 bytes at seq1s + len1 * k, seq2 k = the len2 bytes at
 * seq2s + len2 * k, one (len1, len2) per call, 1 <= len1, len2 <= 16384 (SWMI_BANDED_GLOBAL_MAX_LEN).  Bases are taken modulo
 * 4; any int8[16] matrix; gap_open and gap_extend each in [0, 127], in either order; a gap of length k costs
 * gap_open + (k-1) gap_extend.  diagonals holds one int32 per alignment, NULL means all 0; EVERY int32 value is legal.  Cell
 * (i, j), 0 <= i <= len1, 0 <= j <= len2, is IN THE BAND of alignment k iff  -64 <= (j - i) - diagonals[k] <= 63.  E is
 * vertical (an up move) and F horizontal (a left move), as in swmi_global_full_affine.
 *
 * THE MASK.  free_ends is swmi.h's mask of SWMI_FREE_BEGIN1 / BEGIN2 / END1 / END2 (0 .. 15) with one bit more,
 * SWMI_BANDED_END_ANYWHERE (16): the end cell may be any cell of the table.  It combines with the BEGIN bits but not with END1
 * or END2, so the legal values are 0 .. 19.  SWMI_BANDED_ENDS_EXTEND (16) extends from (0, 0) to wherever the score peaks.
 *
 * CELLS.  Every cell out of the band or off the table holds H = E = F = -infinity (NOT the local aligner's H = 0).  In-band
 * border cells:
 *     H(0,0) = 0
 *     H(0,j) = 0 with SWMI_FREE_BEGIN2, else -(open + (j-1) extend) if (0,0) is in the band, else -infinity     (j >= 1)
 *     H(i,0) = 0 with SWMI_FREE_BEGIN1, else -(open + (i-1) extend) if (0,0) is in the band, else -infinity     (i >= 1)
 *     E(0,j) = F(i,0) = -infinity
 * (a border cell that is not free costs the gap from (0,0) along the border, which lies in the band only with (0,0) itself).
 * In-band cells with i, j >= 1 follow swmi_global_full_affine's recurrences, with no zero floor:
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *
 * END CELL.  The candidates are the IN-BAND cells among: (len1, len2); with SWMI_FREE_END1 (i, len2), i = 0 .. len1; with
 * SWMI_FREE_END2 (len1, j), j = 0 .. len2; with SWMI_BANDED_END_ANYWHERE every cell of the table, border included.  The end cell
 * is the candidate with the largest H, among equal ones the first in row-major order.  scores[k] = that H, which may be
 * NEGATIVE; every finite value lies in [-127 (len1 + len2), 127 min(len1, len2)].
 *
 * INFEASIBLE ALIGNMENTS.  If no candidate is in the band, or every candidate holds -infinity, scores[k] =
 * SWMI_BANDED_NO_ALIGNMENT (INT32_MIN), ends[k] = (0, 0, 0, 0) with a traceback and (0, 0, -1, -1) ends-only, steps[k] = 0.
 * The call still returns SWMI_OK: this is a per-alignment result, not an error.
 *
 * WALK, moves, ends[4] and the forced border steps are swmi_global_full_affine's (swmi.h), word for word: states H / E / F;
 * diagonal, then E, then F; opening wins a tie; at (0,0) the walk ends, on row 0 it ends with SWMI_FREE_BEGIN2 and else goes
 * left to (0,0) by forced steps, on column 0 likewise with SWMI_FREE_BEGIN1 and up steps; forced steps are counted in steps[k].
 * moves + k * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) receives the steps in walking order (3 = diagonal, 2 = up, 1 = left, step
 * t at bits 2 (t % 32) of word t / 32); a path is rebuilt by swmi_local_full_expand_moves (libswmi.so): there is no second
 * expander.  THE WALK CANNOT LEAVE THE BAND: an out-of-band neighbour contributes -infinity, which never equals a finite H, so
 * no move is taken to it; and a forced run along a border that is not free lies in the band, because that border's cells are
 * finite only when (0,0) is in the band, and the band's cells of a row or column are contiguous.  moves and steps both NULL:
 * ENDS-ONLY -- no codes are stored or walked, the start cell is reported as (-1, -1).
 *
 * IDENTITIES.
 *   1. Where the path of swmi_global_full_affine stays in the band, start cell included, every field and move equals that
 *      entry's under the same mask 0 .. 15: banded H <= full H cell by cell, with equality along an in-band path.
 *   2. With gap_open = gap_extend = g the same holds against swmi_global_full with gap g.
 *   3. When the whole table lies in the band (for example len1, len2 <= 63 with diagonal 0) every field equals the full
 *      aligner's for every pair and every mask, with no qualification.
 *   4. Mask 16 against swmi_semiglobal_full_affine, where that entry's path stays in the band: score and end cell are equal,
 *      the first lengths - 1 moves are equal, and the banded walk then adds the forced steps to (0,0).
 *
 * ARGUMENTS are checked in this order, before any device is touched: the matrix (NULL: SWMI_ERR_INVALID_ARGUMENT), the gaps
 * (SWMI_ERR_DOMAIN outside [0, 127]), free_ends (SWMI_ERR_INVALID_ARGUMENT above 19), the moves / steps pair (only one of them
 * given is SWMI_ERR_INVALID_ARGUMENT); then n = 0 (SWMI_OK, no device needed), the buffers (a NULL one is
 * SWMI_ERR_INVALID_ARGUMENT; diagonals may be NULL) and the lengths (outside [1, 16384]: SWMI_ERR_INVALID_ARGUMENT).  Device
 * pointers must be 16-byte aligned, else SWMI_ERR_ALIGNMENT.  Every entry returns SWMI_OK or a negative swmi_status.
 * KNOWN LIMITS: one (len1, len2) per call; 4 letters; a band of 128 diagonals. */
#ifndef SWMI_BANDED_GLOBAL_H
#define SWMI_BANDED_GLOBAL_H

#include <stdint.h>

#include "swmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_BANDED_GLOBAL_MAX_LEN 16384
#define SWMI_BANDED_GLOBAL_WIDTH 128          /* diagonals -64 .. 63 around diagonals[k] */
#define SWMI_BANDED_END_ANYWHERE 16u          /* the end cell is the best cell anywhere in the band */
#define SWMI_BANDED_ENDS_EXTEND 16u           /* from (0,0) to wherever the score peaks */
#define SWMI_BANDED_MAX_FREE_ENDS 19u
#define SWMI_BANDED_NO_ALIGNMENT INT32_MIN    /* the score of an infeasible alignment */

SWMI_API const char *swmi_banded_global_last_error(void);
SWMI_API int swmi_banded_global_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_banded_global_release_workspaces(void);

/* Host buffers: seq1s (n * len1 bytes), seq2s (n * len2), diagonals (n int32, or NULL), scores[n], ends[4 n]; moves
 * (n * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) words) and steps[n], or both NULL for ends-only.  The batch runs in SLICES
 * (swmi_banded_global_slices_for) on two sets of device buffers, one slice's copies beside the other's kernel. */
SWMI_API int swmi_banded_global(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int32_t *diagonals,
                                const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, int32_t *scores,
                                int32_t *ends, uint64_t *moves, uint32_t *steps);

/* The same with every buffer in device memory of the current device, d_diagonals included (or NULL), 16-byte aligned;
 * score_matrix is host memory, read before the call returns; asynchronous on `stream`.  The traceback codes (64 bytes per
 * iteration of the sweep) go to a workspace of the library's per (device, stream), grown on demand up to one slice and kept
 * until swmi_banded_global_release_workspaces(). */
SWMI_API int swmi_banded_global_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const void *d_diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                       unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* The slices a call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns how many there are and
 * writes the first `cap` sizes (NULL to count).  The budgets are swmi_banded_slices_for's: with a traceback 4 383 801 344
 * bytes, ends-only 256 MiB; at most 2^20 alignments per slice and at least one.  An alignment takes len1 + len2 + 4 (diagonal)
 * + 20 (results) bytes and with a traceback its codes, 256 ceil((len1 + 64) / 4) -- row 0 is swept, one iteration more than
 * swmi_banded_local's len1 + 63 --, its moves, 8 SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2), and 4 of steps.  Needs no device.  0
 * for a length outside [1, 16384]. */
SWMI_API size_t swmi_banded_global_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);

/* Measurement helper: one untimed swmi_banded_global_device call, then `iters` of them back to back on `stream`, bracketed by
 * HIP events; *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_banded_global_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const void *d_diagonals, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                            unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream,
                                            int iters, float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_BANDED_GLOBAL_H */
