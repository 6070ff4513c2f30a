/* local_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the local aligner's semantics (include/swmi.h,
 * swmi_local_align) for any int8 matrix and gap, compiled by tests/test_local_cpu.py into pytest's temporary directory.
 *
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)
 *     end cell  = the first cell in row-major order whose value is strictly greater than every earlier one (from 0 at (0,0))
 *     walk      = diagonal if H == H(i-1,j-1) + s, else up if H == H(i-1,j) - gap, else left, until H == 0
 *
 * The full matrix is kept (len1 + 1) x 129 int32; nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* moves: (len1 + 128 + 31) / 32 words or more, walking order from the end cell, 3 / 2 / 1 = diagonal / up / left.
 * ends = (end_i, end_j, start_i, start_j).  Returns 0, or -1 if memory runs out. */
int local_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, const int8_t *sm, int gap, int32_t *score,
                 int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const size_t W = 129;
    int32_t *H = (int32_t *)calloc((len1 + 1) * W, sizeof(int32_t));
    if (!H) return -1;
    int best = 0, bi = 0, bj = 0;
    for (size_t i = 1; i <= len1; ++i)
        for (size_t j = 1; j <= 128; ++j) {
            int h = 0;
            const int d = H[(i - 1) * W + j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            const int u = H[(i - 1) * W + j] - gap;
            const int l = H[i * W + j - 1] - gap;
            if (d > h) h = d;
            if (u > h) h = u;
            if (l > h) h = l;
            H[i * W + j] = h;
            if (best < h) {
                best = h;
                bi = (int)i;
                bj = (int)j;
            }
        }
    int i = bi, j = bj;
    uint32_t t = 0;
    while (i > 0 && j > 0 && H[i * W + j] != 0) {
        const int h = H[i * W + j];
        unsigned m;
        if (h == H[(i - 1) * W + j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)]) {
            m = 3;
            --i;
            --j;
        } else if (h == H[(i - 1) * W + j] - gap) {
            m = 2;
            --i;
        } else {
            m = 1;
            --j;
        }
        if (moves) {
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
        }
        ++t;
    }
    free(H);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    ends[2] = i;
    ends[3] = j;
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 * k, seq2 k at seq2s + 128 k; moves rows of `move_words` words */
int local_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t *sm, int gap,
                       int32_t *scores, int32_t *ends, uint64_t *moves, size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= local_oracle(seq1s + len1 * (size_t)k, len1, seq2s + 128 * (size_t)k, sm, gap, scores + k, ends + 4 * k,
                           moves ? moves + move_words * (size_t)k : NULL, steps ? steps + k : NULL);
    return rc;
}
