/* global_full_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the global and free-end-gap aligner's semantics
 * (include/swmi.h, swmi_global_full) for any lengths, int8 matrix, gap and mask, compiled by the global_full tests into
 * pytest's temporary directory.  These semantics have no reference counterpart: this file is their definition.
 *
 *     free_ends: 1 = BEGIN1 (H(i,0) = 0), 2 = BEGIN2 (H(0,j) = 0), 4 = END1 (end in any (i, len2)), 8 = END2 (any (len1, j))
 *     H(0,0) = 0, H(i,0) = BEGIN1 ? 0 : -i gap, H(0,j) = BEGIN2 ? 0 : -j gap
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)
 *     end cell  = of (len1, len2), the last column with END1 and the last row with END2 (border cells included) the largest
 *                 H; among equal ones the first in row-major order
 *     walk      = diagonal if H == H(i-1,j-1) + s, else up if H == H(i-1,j) - gap, else left, while i > 0 and j > 0; on row 0
 *                 it ends if BEGIN2 (or j = 0), else goes left to (0,0); on column 0 it ends if BEGIN1, else goes up to (0,0)
 *
 * Two rolling rows of H, the last column kept aside, and 2 bits per cell of which predecessor the walk takes (3 / 2 / 1 =
 * diagonal / up / left); nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell; NULL: no walk, ends[2..3] = -1.
 * ends = (end_i, end_j, start_i, start_j).  *steps = the number of moves.  Returns 0, or -1 if memory runs out. */
int global_full_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, const int8_t *sm, int gap,
                       unsigned free_ends, int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const int begin1 = free_ends & 1, begin2 = free_ends & 2, end1 = free_ends & 4, end2 = free_ends & 8;
    const size_t W = len2 + 1, row_bytes = (W + 3) / 4;
    int32_t *prev = (int32_t *)malloc(W * sizeof(int32_t)), *cur = (int32_t *)malloc(W * sizeof(int32_t));
    int32_t *lastcol = (int32_t *)malloc((len1 + 1) * sizeof(int32_t));
    uint8_t *codes = moves ? (uint8_t *)calloc((len1 + 1) * row_bytes, 1) : NULL;
    if (!prev || !cur || !lastcol || (moves && !codes)) {
        free(prev);
        free(cur);
        free(lastcol);
        free(codes);
        return -1;
    }
    for (size_t j = 0; j <= len2; ++j) prev[j] = begin2 ? 0 : -(int)j * gap;
    lastcol[0] = prev[len2];
    for (size_t i = 1; i <= len1; ++i) {
        cur[0] = begin1 ? 0 : -(int)i * gap;
        uint8_t *crow = codes ? codes + i * row_bytes : NULL;
        for (size_t j = 1; j <= len2; ++j) {
            const int d = prev[j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            const int u = prev[j] - gap;
            const int l = cur[j - 1] - gap;
            int h = d;
            unsigned m = 3;
            if (u > h) {
                h = u;
                m = 2;
            }
            if (l > h) {
                h = l;
                m = 1;
            }
            cur[j] = h;
            if (crow) crow[j >> 2] |= (uint8_t)(m << (2 * (j & 3)));
        }
        lastcol[i] = cur[len2];
        int32_t *t = prev;
        prev = cur;
        cur = t;
    }
    /* prev is row len1 now.  Candidates in row-major order; a later one wins only when strictly greater */
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
            if (!have || prev[j] > best) {
                have = 1;
                best = prev[j];
                bi = (int)len1;
                bj = (int)j;
            }
    if (!have || prev[len2] > best) {
        best = prev[len2];
        bi = (int)len1;
        bj = (int)len2;
    }
    uint32_t t = 0;
    int i = bi, j = bj;
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
                m = (codes[(size_t)i * row_bytes + (j >> 2)] >> (2 * (j & 3))) & 3u;
            }
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            i -= m != 1;
            j -= m != 2;
            ++t;
        }
    }
    free(prev);
    free(cur);
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
int global_full_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t *sm,
                             int gap, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, size_t move_words,
                             uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= global_full_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, sm, gap, free_ends, scores + k,
                                 ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL, steps ? steps + k : NULL);
    return rc;
}
