/* global_full_affine_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the affine global and free-end-gap aligner's
 * semantics (include/swmi.h, swmi_global_full_affine) for any lengths, int8 matrix, gap_open, gap_extend and mask, compiled by
 * the global_full_affine tests into pytest's temporary directory.  These semantics have no reference counterpart: this file
 * is their definition.
 *
 *     free_ends: 1 = BEGIN1 (H(i,0) = 0), 2 = BEGIN2 (H(0,j) = 0), 4 = END1 (end in any (i, len2)), 8 = END2 (any (len1, j))
 *     H(0,0) = 0, H(i,0) = BEGIN1 ? 0 : -(open + (i-1) extend), H(0,j) = BEGIN2 ? 0 : -(open + (j-1) extend)
 *     E(0,j) = F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     end cell  = of (len1, len2), the last column with END1 and the last row with END2 (border cells included) the largest
 *                 H; among equal ones the first in row-major order
 *     walk      = state H: diagonal if H == diag, else state E if H == E, else state F; state E: up, then H if E opened
 *                 (opening wins a tie), else E; state F: left likewise, while i > 0 and j > 0; on row 0 it ends if BEGIN2 (or
 *                 j = 0), else goes left to (0,0); on column 0 it ends if BEGIN1, else goes up to (0,0)
 *
 * Rolling rows of H and E and one running F, the last column kept aside, plus 4 bits per cell for the walk (H's choice
 * 3 / 2 / 1 = diagonal / E / F, E's open bit, F's open bit); nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG_INF (-(1 << 29))

static int border(size_t k, int free_border, int open, int ext) { return k == 0 || free_border ? 0 : -(open + (int)(k - 1) * ext); }

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell; NULL: no walk, ends[2..3] = -1.
 * ends = (end_i, end_j, start_i, start_j).  *steps = the number of moves.  Returns 0, or -1 if memory runs out. */
int global_full_affine_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, const int8_t *sm, int open,
                              int ext, unsigned free_ends, int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const int begin1 = free_ends & 1, begin2 = free_ends & 2, end1 = free_ends & 4, end2 = free_ends & 8;
    const size_t W = len2 + 1;
    int32_t *hp = (int32_t *)malloc(W * sizeof(int32_t)), *hc = (int32_t *)malloc(W * sizeof(int32_t));
    int32_t *e = (int32_t *)malloc(W * sizeof(int32_t));
    int32_t *lastcol = (int32_t *)malloc((len1 + 1) * sizeof(int32_t));
    /* 4 bits per cell (two cells per byte): bits 0-1 H's choice, bit 2 E's open bit, bit 3 F's open bit */
    uint8_t *codes = moves ? (uint8_t *)calloc(((len1 + 1) * W + 1) / 2, 1) : NULL;
    if (!hp || !hc || !e || !lastcol || (moves && !codes)) {
        free(hp);
        free(hc);
        free(e);
        free(lastcol);
        free(codes);
        return -1;
    }
    for (size_t j = 0; j <= len2; ++j) {
        hp[j] = border(j, begin2, open, ext);
        e[j] = NEG_INF;
    }
    lastcol[0] = hp[len2];
    for (size_t i = 1; i <= len1; ++i) {
        hc[0] = border(i, begin1, open, ext);
        int f = NEG_INF;
        for (size_t j = 1; j <= len2; ++j) {
            const int eo = hp[j] - open, ee = e[j] - ext;
            const int e_open = eo >= ee;
            e[j] = e_open ? eo : ee;
            const int fo = hc[j - 1] - open, fe = f - ext;
            const int f_open = fo >= fe;
            f = f_open ? fo : fe;
            const int d = hp[j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            int h = d;
            unsigned m = 3;
            if (e[j] > h) {
                h = e[j];
                m = 2;
            }
            if (f > h) {
                h = f;
                m = 1;
            }
            hc[j] = h;
            if (codes) {
                const size_t at = i * W + j;
                codes[at >> 1] |= (uint8_t)((m | (unsigned)e_open << 2 | (unsigned)f_open << 3) << (4 * (at & 1)));
            }
        }
        lastcol[i] = hc[len2];
        int32_t *t = hp;
        hp = hc;
        hc = t;
    }
    /* hp is row len1 now.  Candidates in row-major order; a later one wins only when strictly greater */
    int have = 0, best = 0, bi = 0, bj = 0;
    if (end1)
        for (size_t i = 0; i < len1; ++i)
            if (!have || lastcol[i] > best) {
                have = 1;
                best = lastcol[i];
                bi = (int)i;
                bj = (int)len2;
            }
    if (end2)
        for (size_t j = 0; j < len2; ++j)
            if (!have || hp[j] > best) {
                have = 1;
                best = hp[j];
                bi = (int)len1;
                bj = (int)j;
            }
    if (!have || hp[len2] > best) {
        best = hp[len2];
        bi = (int)len1;
        bj = (int)len2;
    }
    uint32_t t = 0;
    int i = bi, j = bj, state = 0;   /* 0 = H, 1 = E, 2 = F */
    if (moves) {
        while (i > 0 || j > 0) {
            unsigned m;
            if (i == 0) {
                if (begin2) break;
                m = 1;
            } else if (j == 0) {
                if (begin1) break;
                m = 2;
            } else {
                const size_t at = (size_t)i * W + (size_t)j;
                const unsigned c = (codes[at >> 1] >> (4 * (at & 1))) & 15u;
                if (state == 0) state = (c & 3u) == 3u ? 0 : (c & 3u) == 2u ? 1 : 2;
                if (state == 0) {
                    m = 3;
                } else if (state == 1) {
                    m = 2;
                    state = (c >> 2) & 1u ? 0 : 1;
                } else {
                    m = 1;
                    state = (c >> 3) & 1u ? 0 : 2;
                }
            }
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            i -= m != 1;
            j -= m != 2;
            ++t;
        }
    }
    free(hp);
    free(hc);
    free(e);
    free(lastcol);
    free(codes);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    ends[2] = moves ? i : -1;
    ends[3] = moves ? j : -1;
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 k, seq2 k at seq2s + len2 k; moves rows of `move_words` words (NULL: ends only) */
int global_full_affine_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                    const int8_t *sm, int open, int ext, unsigned free_ends, int32_t *scores, int32_t *ends,
                                    uint64_t *moves, size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= global_full_affine_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, sm, open, ext, free_ends,
                                        scores + k, ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL,
                                        steps ? steps + k : NULL);
    return rc;
}
