/* local_full_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the any-length local aligner's semantics
 * (include/swmi.h, swmi_local_full) for any lengths, int8 matrix and gap, compiled by the local_full tests into pytest's
 * temporary directory.
 *
 *     H(i,0) = H(0,j) = 0
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)
 *     end cell  = the first cell in row-major order whose value is strictly greater than every earlier one (from 0 at (0,0))
 *     walk      = stop if H == 0, else diagonal if H == H(i-1,j-1) + s, else up if H == H(i-1,j) - gap, else left
 *
 * Two rolling rows of H and 2 bits per cell of what the walk does there (0 = stop, 3 / 2 / 1 = diagonal / up / left),
 * instead of the whole table; nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell (NULL: ends only, start cell (-1, -1)).
 * ends = (end_i, end_j, start_i, start_j).  Returns 0, or -1 if memory runs out. */
int local_full_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, const int8_t *sm, int gap,
                      int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const size_t W = len2 + 1, row_bytes = (W + 3) / 4;
    int32_t *prev = (int32_t *)calloc(W, sizeof(int32_t)), *cur = (int32_t *)calloc(W, sizeof(int32_t));
    uint8_t *codes = moves ? (uint8_t *)calloc((len1 + 1) * row_bytes, 1) : NULL;
    if (!prev || !cur || (moves && !codes)) {
        free(prev);
        free(cur);
        free(codes);
        return -1;
    }
    int best = 0, bi = 0, bj = 0;
    for (size_t i = 1; i <= len1; ++i) {
        cur[0] = 0;
        uint8_t *crow = codes ? codes + i * row_bytes : NULL;
        for (size_t j = 1; j <= len2; ++j) {
            const int d = prev[j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            const int u = prev[j] - gap;
            const int l = cur[j - 1] - gap;
            int h = 0;
            if (d > h) h = d;
            if (u > h) h = u;
            if (l > h) h = l;
            const unsigned m = h == 0 ? 0 : h == d ? 3 : h == u ? 2 : 1;
            cur[j] = h;
            if (crow) crow[j >> 2] |= (uint8_t)(m << (2 * (j & 3)));
            if (best < h) {
                best = h;
                bi = (int)i;
                bj = (int)j;
            }
        }
        int32_t *t = prev;
        prev = cur;
        cur = t;
    }
    uint32_t t = 0;
    int i = bi, j = bj;
    if (moves) {
        while (i > 0 && j > 0) {
            const unsigned m = (codes[(size_t)i * row_bytes + (j >> 2)] >> (2 * (j & 3))) & 3u;
            if (m == 0) break;
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            i -= m != 1;
            j -= m != 2;
            ++t;
        }
    } else {
        i = j = -1;
    }
    free(prev);
    free(cur);
    free(codes);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    ends[2] = i;
    ends[3] = j;
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 k, seq2 k at seq2s + len2 k; moves rows of `move_words` words (NULL: ends only) */
int local_full_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t *sm,
                            int gap, int32_t *scores, int32_t *ends, uint64_t *moves, size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= local_full_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, sm, gap, scores + k, ends + 4 * k,
                                moves ? moves + move_words * (size_t)k : NULL, steps ? steps + k : NULL);
    return rc;
}
