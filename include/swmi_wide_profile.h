/* swmi_wide_profile.h -- C ABI of libswmi_wide_profile.so: a batch of n sequences over 32 LETTERS (the database, the rows,
 * MIXED lengths) against ONE position-specific scoring matrix of len2 columns (a PSSM: one column of 32 scores per query
 * position, as PSI-BLAST and profile search use; a plain query under a 32 x 32 matrix is the special case that
 * swmi_wide_profile_from_sequence writes).  Local, and global / fit / overlap by the free_ends mask; AFFINE gaps; end cell,
 * start cell and traceback or ends-only.  DESIGN.md section 32.
 *
 * A library of its own beside libswmi.so, libswmi_wide.so and libswmi_wide_long.so, with libswmi_wide.so's rules:
 *   - it needs NO swmi_init: every entry runs on the calling thread's CURRENT HIP device (hipSetDevice) and on the stream it
 *     is given; the host entries use two streams of their own per device;
 *   - its workspaces are its own, one per (device, stream); swmi_wide_profile_release_workspaces frees the current device's;
 *   - its last error is its own: swmi_wide_profile_last_error(), thread-local text.
 *
 * SEMANTICS: those of swmi_wide.h (swmi_wide_local*, swmi_wide_global*), field for field -- the recurrences, the tie rules,
 * the end-cell rule (H descending, row ascending, column ascending), ends[4] = (end_i, end_j, start_i, start_j), the
 * ends-only start (-1, -1), the move encoding, the zero-length closed forms -- with ONE difference: the substitution score of
 * cell (i, j) is
 *     profile[(j - 1) * 32 + (seq1[i-1] & 31)]
 * with profile an int8[len2 * 32] in HOST memory, position-major; every int8 value is allowed, and only the low five bits of
 * a sequence byte are read.  It is read before the call returns.  With profile[j * 32 + a] = score_matrix[a * 32 + (query[j]
 * & 31)] every output equals swmi_wide_local / swmi_wide_global on (seq1[k], query) for every k.  gap_open and gap_extend lie
 * in [0, 127], else SWMI_ERR_DOMAIN; free_ends is a mask of SWMI_FREE_* (swmi.h), at most SWMI_ENDS_OVERLAP = 15, else
 * SWMI_ERR_INVALID_ARGUMENT.  No shape within the limits is outside the kernels' domain: there is no domain rule.
 *
 * LENGTHS: 0 <= len1 <= SWMI_WIDE_PROFILE_MAX_LEN1 = 16384 per sequence and 0 <= len2 <= SWMI_WIDE_PROFILE_MAX_LEN2 = 4096;
 * more is SWMI_ERR_INVALID_ARGUMENT.  profile may be NULL if and only if len2 = 0.  A zero length gives exactly what the
 * 4-letter ragged entries give, and no sequence byte is read.  KNOWN LIMITS: len2 <= 4096 (the kernels hold 32 KiB of LDS per
 * 1024 columns; column stripes as libswmi_wide_long.so sweeps them are the way to lift it); the gap costs are not
 * position-specific; the profile is host memory and is transposed and uploaded by every call.
 *
 * MOVES: alignment k's words lie at moves + move_offsets[k], move_offsets from swmi_wide_profile_move_offsets -- the running
 * sum of SWMI_LOCAL_FULL_MOVE_WORDS(len1_k, len2), what swmi_local_full_ragged_move_offsets gives on seq2_offsets[k] = k *
 * len2; a path is expanded by swmi_local_full_expand_moves (swmi.h, libswmi.so).  There is no second expander.
 *
 * ARGUMENTS are checked in swmi_wide.h's order, before any device is touched: the mask, the profile (NULL with len2 > 0) and
 * the gaps, the moves / steps pair (only one of them given is an error); then n = 0 (SWMI_OK, no device needed), the
 * buffers, seq1_offsets (NULL, decreasing, a length above the limit) and len2.  Device pointers must be 16-byte aligned,
 * else SWMI_ERR_ALIGNMENT.  Every entry returns SWMI_OK or a negative swmi_status. */
#ifndef SWMI_WIDE_PROFILE_H
#define SWMI_WIDE_PROFILE_H

#include "swmi_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_WIDE_PROFILE_MAX_LEN1 16384
#define SWMI_WIDE_PROFILE_MAX_LEN2 4096
#define SWMI_WIDE_PROFILE_LOCAL 0
#define SWMI_WIDE_PROFILE_GLOBAL 1

SWMI_API const char *swmi_wide_profile_last_error(void);
SWMI_API int swmi_wide_profile_version(void);
/* Frees the workspaces and host-entry buffers of the calling thread's current device (synchronises the device first). */
SWMI_API int swmi_wide_profile_release_workspaces(void);

/* The profile of a plain query under a 32 x 32 matrix: profile_out[j * 32 + a] = score_matrix[a * 32 + (query[j] & 31)],
 * int8[len2 * 32].  Host only, no device.  len2 <= 4096. */
SWMI_API int swmi_wide_profile_from_sequence(const uint8_t *query, size_t len2, const int8_t score_matrix[1024], int8_t *profile_out);

/* move_offsets[0 .. n]: the running sum of SWMI_LOCAL_FULL_MOVE_WORDS(len1_k, len2).  No device. */
SWMI_API int swmi_wide_profile_move_offsets(const uint64_t *seq1_offsets, size_t n, size_t len2, uint64_t *move_offsets);

/* Host arrays: seq1s concatenated, seq1_offsets of n + 1 entries; profile int8[len2 * 32]; scores[n], ends[4 n]; moves
 * (move_offsets[n] words) and steps[n], or both NULL for ends-only.  A batch is cut into slices
 * (swmi_wide_profile_slices_for), two of them in flight on two sets of device buffers; the profile goes up once per set. */
SWMI_API int swmi_wide_profile_local(const uint8_t *seq1s, const uint64_t *seq1_offsets, size_t n, const int8_t *profile, size_t len2,
                                     int gap_open, int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_wide_profile_global(const uint8_t *seq1s, const uint64_t *seq1_offsets, size_t n, const int8_t *profile, size_t len2,
                                      int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                      uint64_t *moves, uint32_t *steps);

/* d_seq1s and the results are device buffers of the current device; seq1_offsets and profile are host memory, read before
 * the call returns; asynchronous on `stream`.  Calls issued back to back on one stream each see their own profile. */
SWMI_API int swmi_wide_profile_local_device(const void *d_seq1s, const uint64_t *seq1_offsets, size_t n, const int8_t *profile,
                                            size_t len2, int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves,
                                            void *d_steps, void *stream);
SWMI_API int swmi_wide_profile_global_device(const void *d_seq1s, const uint64_t *seq1_offsets, size_t n, const int8_t *profile,
                                             size_t len2, int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                             void *d_ends, void *d_moves, void *d_steps, void *stream);

/* The slices a call cuts its batch into (needs no device): swmi_wide_slices_for's rule and budgets -- 256 MiB ends-only, with
 * a traceback what 256 alignments of 16384 x 4096 take in libswmi_wide.so -- at most 2^20 alignments and at least one.  An
 * alignment's device bytes hold no seq2 (len1, 48 of slot, 20 of results; with a traceback codes, moves and 4 of steps); the
 * profile's device bytes, 32768 x max(1, ceil(len2 / 1024)), count once per slice.  Returns the number of slices and writes
 * the first `cap` sizes; 0 on arguments that an entry would refuse (text in swmi_wide_profile_last_error). */
SWMI_API size_t swmi_wide_profile_slices_for(const uint64_t *seq1_offsets, size_t n, size_t len2, int traceback, size_t *sizes,
                                             size_t cap);

/* Average milliseconds of `iters` device calls of kind SWMI_WIDE_PROFILE_LOCAL or _GLOBAL (free_ends: the global kind's),
 * after one untimed call; HIP events on `stream`.  Every call transposes and uploads the profile, as a device call does. */
SWMI_API int swmi_wide_profile_time_device(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, size_t n, const int8_t *profile,
                                           size_t len2, int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                           void *d_ends, void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);

#ifdef __cplusplus
}
#endif

#endif /* SWMI_WIDE_PROFILE_H */
