/* wide_profile_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the profile aligners' semantics
 * (include/swmi_wide_profile.h) for any lengths, a position-specific int8 profile of len2 columns, gap_open, gap_extend and,
 * for the global kind, the mask; compiled by the profile tests into pytest's temporary directory.  It is wide_affine_oracle.c
 * with one change, the score of a cell: profile[(j - 1) * 32 + (seq1[i-1] & 31)].
 *
 *     E(0,j) = F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)          F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *   local:   H(i,0) = H(0,j) = 0;  H(i,j) = max(0, diag, E, F);  end cell = the first cell in row-major order whose H is
 *            strictly greater than every earlier one (from 0 at (0,0));  walk: stop at H == 0, else diagonal, else E, else F
 *   global:  free_ends: 1 = BEGIN1 (H(i,0) = 0), 2 = BEGIN2 (H(0,j) = 0), 4 = END1 (end in any (i, len2)), 8 = END2 (any
 *            (len1, j));  H(i,0) / H(0,j) = -(open + (k-1) extend) where not free;  H(i,j) = max(diag, E, F);  end cell =
 *            the largest H of the allowed cells, among equal ones the first in row-major order;  walk: diagonal, else E,
 *            else F while i > 0 and j > 0; on a border it ends if that border's begin is free, else goes on to (0,0)
 *   both:    inside E: up, back to H where E opened (opening wins a tie); inside F: left, likewise.
 *
 * One whole table of H, rolling E and F, 4 bits of walk per cell; nothing here is tuned. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG_INF (-(1 << 29))

static int border(size_t k, int free_border, int open, int ext) { return k == 0 || free_border ? 0 : -(open + (int)(k - 1) * ext); }

/* kind 0 = local, 1 = global.  moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell, 3 / 2 / 1 =
 * diagonal / up / left; NULL: no walk, ends[2..3] = -1.  ends = (end_i, end_j, start_i, start_j).  *steps = the moves.
 * Returns 0, or -1 if memory runs out. */
int wide_profile_oracle(int kind, const uint8_t *seq1, size_t len1, const int8_t *profile, size_t len2, int open, int ext,
                        unsigned free_ends, int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const int local = kind == 0;
    const int begin1 = free_ends & 1, begin2 = free_ends & 2, end1 = free_ends & 4, end2 = free_ends & 8;
    const size_t W = len2 + 1;
    int32_t *H = (int32_t *)malloc((len1 + 1) * W * sizeof(int32_t));
    int32_t *e = (int32_t *)malloc(W * sizeof(int32_t));
    /* per cell: bits 0-1 H's choice (0 = the floor, 3 = diagonal, 2 = E, 1 = F), bit 2 E opened, bit 3 F opened */
    uint8_t *codes = (uint8_t *)calloc((len1 + 1) * W, 1);
    if (!H || !e || !codes) {
        free(H);
        free(e);
        free(codes);
        return -1;
    }
    for (size_t j = 0; j <= len2; ++j) {
        H[j] = local ? 0 : border(j, begin2, open, ext);
        e[j] = NEG_INF;
    }
    for (size_t i = 1; i <= len1; ++i) {
        int32_t *hp = H + (i - 1) * W, *hc = H + i * W;
        hc[0] = local ? 0 : border(i, begin1, open, ext);
        int f = NEG_INF;
        for (size_t j = 1; j <= len2; ++j) {
            const int eo = hp[j] - open, ee = e[j] - ext;
            const int fo = hc[j - 1] - open, fe = f - ext;
            const int E = eo >= ee ? eo : ee, F = fo >= fe ? fo : fe;
            const int d = hp[j - 1] + profile[(j - 1) * 32 + (seq1[i - 1] & 31)];
            int h = d;
            unsigned m = 3;
            if (E > h) {
                h = E;
                m = 2;
            }
            if (F > h) {
                h = F;
                m = 1;
            }
            if (local && h <= 0) {
                h = 0;
                m = 0;
            }
            e[j] = E;
            f = F;
            hc[j] = h;
            codes[i * W + j] = (uint8_t)(m | (eo >= ee ? 4u : 0u) | (fo >= fe ? 8u : 0u));
        }
    }
    /* the end cell: candidates in row-major order, a later one wins only when strictly greater */
    int best = 0, bi = 0, bj = 0;
    if (local) {
        for (size_t i = 1; i <= len1; ++i)
            for (size_t j = 1; j <= len2; ++j)
                if (H[i * W + j] > best) {
                    best = H[i * W + j];
                    bi = (int)i;
                    bj = (int)j;
                }
    } else {
        int have = 0;
        for (size_t i = 0; i <= len1; ++i)
            for (size_t j = 0; j <= len2; ++j) {
                const int allowed = (i == len1 && j == len2) || (end1 && j == len2) || (end2 && i == len1);
                if (allowed && (!have || H[i * W + j] > best)) {
                    have = 1;
                    best = H[i * W + j];
                    bi = (int)i;
                    bj = (int)j;
                }
            }
    }
    uint32_t t = 0;
    int i = bi, j = bj, state = 0;   /* 0 = H, 1 = E, 2 = F */
    if (moves) {
        while (i > 0 || j > 0) {
            unsigned m;
            if (i == 0 || j == 0) {
                if (local) break;
                if (i == 0) {
                    if (begin2) break;
                    m = 1;
                } else {
                    if (begin1) break;
                    m = 2;
                }
            } else {
                const unsigned c = codes[(size_t)i * W + (size_t)j];
                if (state == 0) {
                    if ((c & 3u) == 0) break;      /* the floor: only the local kind writes it */
                    state = (c & 3u) == 3u ? 0 : (c & 3u) == 2u ? 1 : 2;
                }
                if (state == 0) {
                    m = 3;
                } else if (state == 1) {
                    m = 2;
                    state = c & 4u ? 0 : 1;
                } else {
                    m = 1;
                    state = c & 8u ? 0 : 2;
                }
            }
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            i -= m != 1;
            j -= m != 2;
            ++t;
        }
    }
    free(H);
    free(e);
    free(codes);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    ends[2] = moves ? i : -1;
    ends[3] = moves ? j : -1;
    if (steps) *steps = t;
    return 0;
}

/* n sequences of a ragged batch against the one profile: seq1 k = seq1s[off1[k] .. off1[k + 1]); moves of alignment k at
 * moves + move_offsets[k] (moves NULL: ends only) */
int wide_profile_oracle_ragged(int kind, const uint8_t *seq1s, const uint64_t *off1, size_t n, const int8_t *profile, size_t len2,
                               int open, int ext, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves,
                               const uint64_t *move_offsets, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= wide_profile_oracle(kind, seq1s + off1[k], (size_t)(off1[k + 1] - off1[k]), profile, len2, open, ext, free_ends,
                                  scores + k, ends + 4 * k, moves ? moves + move_offsets[k] : NULL, steps ? steps + k : NULL);
    return rc;
}
