/* swmi_pk_form.h -- C ABI of libswmi_pk_form.so: the checks of the packed scorer (sw128_pk_kernel, libswmi.so) that tests
 * and tools call; scoring needs neither.  A small library of its own beside libswmi.so: it needs NO swmi_init, links only the
 * HIP runtime, and its GPU entry runs on the calling thread's current HIP device.
 *
 * The rule swmi_pk_cell_form reports is the one libswmi.so launches by (one inline function, csrc/pk_form.h); swmi.h,
 * "schedules", states it. */
#ifndef SWMI_PK_FORM_H
#define SWMI_PK_FORM_H

#include "swmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SWMI_PK_FORM_Q0 0      /* every s + gap >= 0 */
#define SWMI_PK_FORM_BIAS 1    /* values shifted by Q = -(min s + gap) */
#define SWMI_PK_FORM_VERT 2    /* vertical-offset form */
#define SWMI_PK_FORM_FLAG 3    /* the flag form of 2: the kernel and its name are variant 2's, the cell is variant 0's */

/* Which cell body the packed kernel runs for (score_matrix, gap_penalty): one of SWMI_PK_FORM_*.  Needs no device.
 * scale[0] = m + gap and scale[1] = the rescaled gap 255 gap / (m + gap) for SWMI_PK_FORM_FLAG, else 0, 0 (scale may be NULL).
 * SWMI_ERR_INVALID_ARGUMENT for a NULL matrix, SWMI_ERR_DOMAIN for a gap outside [0, 127]. */
SWMI_API int swmi_pk_cell_form(const int8_t score_matrix[16], int gap_penalty, int scale[2]);

/* The flag form's premise, on the current HIP device: for EVERY pair (a, b) of 16-bit integers in [0, 0x7C00) and a
 * pseudo-random finite negative half 0x8000 | v, v in [0x00FF, 0x7C00), v_pk_maximum3_f16 returns max(a, b) -- the negative
 * half in each operand position, in either half of the register.  *checked = comparisons made, *mismatches = those that
 * failed.  SWMI_OK, SWMI_ERR_INVALID_ARGUMENT (NULL) or SWMI_ERR_HIP (a HIP call failed, or there is no device). */
SWMI_API int swmi_pk_selftest_max3_negative(unsigned long long *checked, unsigned long long *mismatches);

/* The PRODUCT FORM, a sub-form of SWMI_PK_FORM_FLAG for plain match / mismatch scoring: the diagonal term of a
 * row is one 16-bit multiply-add per half, a[row base] * b[column base] + H modulo 2^16 -- H + 255 where the bases agree, a
 * finite negative half where they differ.  Returns 1 when (score_matrix, gap_penalty) is eligible -- swmi_pk_cell_form gives
 * SWMI_PK_FORM_FLAG, the entries above -2 gap are exactly the four diagonal ones, and the largest rescaled H,
 * 255 * 128 m / (m + gap), is at most the bound below -- else 0.  Needs no device.  When eligible, consts[0..3] = a,
 * consts[4..7] = b, consts[8] = the largest rescaled H the constants are verified for; otherwise nine zeros (consts may be
 * NULL).  Errors as swmi_pk_cell_form.  An eligible set runs the product form unless the environment holds
 * SWMI_PK_NO_PRODUCT at swmi_init, which keeps it on the flag form's own cell (same scores; for A/B runs). */
SWMI_API int swmi_pk_product_form(const int8_t score_matrix[16], int gap_penalty, int consts[9]);

/* The product form's premise, on the current HIP device: for all 16 (row base, column base), EVERY H in [0, bound] and both
 * halves of the register, v_pk_mad_i16 gives (a[r] * b[c] + H) mod 65536, and the v_pk_maximum3_f16 that follows against two
 * non-negative operands p, q gives max(p, q, H + 255) where r = c and max(p, q) where not.  *checked, *mismatches and the
 * return value as swmi_pk_selftest_max3_negative. */
SWMI_API int swmi_pk_selftest_product_mad(unsigned long long *checked, unsigned long long *mismatches);

#ifdef __cplusplus
}
#endif
#endif
