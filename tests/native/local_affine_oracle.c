/* local_affine_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the affine local aligner's semantics
 * (include/swmi.h, swmi_local_align_affine) for any int8 matrix, gap_open and gap_extend, compiled by the tests into pytest's
 * temporary directory.
 *
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     end cell  = the first cell in row-major order whose H is strictly greater than every earlier one (from 0 at (0,0))
 *     walk      = state H: stop at H == 0, else diagonal if H == H(i-1,j-1) + s, else state E if H == E, else state F;
 *                 state E: up, then state H if E == H(i-1,j) - open, else stay E; state F: left, likewise
 *
 * The three full matrices are kept (len1 + 1) x 129 int32; nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define MINUS_INF (-(1 << 28))

/* moves: (len1 + 128 + 31) / 32 words or more, walking order from the end cell, 3 / 2 / 1 = diagonal / up / left.
 * ends = (end_i, end_j, start_i, start_j).  Returns 0, or -1 if memory runs out. */
int local_affine_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, const int8_t *sm, int open, int extend,
                        int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const size_t W = 129, cells = (len1 + 1) * W;
    int32_t *H = (int32_t *)calloc(cells, sizeof(int32_t));
    int32_t *E = (int32_t *)malloc(cells * sizeof(int32_t));
    int32_t *F = (int32_t *)malloc(cells * sizeof(int32_t));
    if (!H || !E || !F) {
        free(H);
        free(E);
        free(F);
        return -1;
    }
    for (size_t c = 0; c < cells; ++c) E[c] = F[c] = MINUS_INF;
    int best = 0, bi = 0, bj = 0;
    for (size_t i = 1; i <= len1; ++i)
        for (size_t j = 1; j <= 128; ++j) {
            const size_t c = i * W + j;
            const int eo = H[c - W] - open, ee = E[c - W] - extend;
            const int fo = H[c - 1] - open, fe = F[c - 1] - extend;
            E[c] = eo > ee ? eo : ee;
            F[c] = fo > fe ? fo : fe;
            int h = 0;
            const int d = H[c - W - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            if (d > h) h = d;
            if (E[c] > h) h = E[c];
            if (F[c] > h) h = F[c];
            H[c] = h;
            if (best < h) {
                best = h;
                bi = (int)i;
                bj = (int)j;
            }
        }
    int i = bi, j = bj, state = 0;   /* 0 = H, 1 = E, 2 = F */
    uint32_t t = 0;
    while (i > 0 && j > 0) {
        const size_t c = (size_t)i * W + (size_t)j;
        unsigned m;
        if (state == 0) {
            if (H[c] == 0) break;
            if (H[c] == H[c - W - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)]) state = 0;
            else if (H[c] == E[c]) state = 1;
            else state = 2;
        }
        if (state == 0) {
            m = 3;
            --i;
            --j;
        } else if (state == 1) {
            m = 2;
            state = E[c] == H[c - W] - open ? 0 : 1;
            --i;
        } else {
            m = 1;
            state = F[c] == H[c - 1] - open ? 0 : 2;
            --j;
        }
        if (moves) {
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
        }
        ++t;
    }
    free(H);
    free(E);
    free(F);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    ends[2] = i;
    ends[3] = j;
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 * k, seq2 k at seq2s + 128 k; moves rows of `move_words` words */
int local_affine_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t *sm, int open,
                              int extend, int32_t *scores, int32_t *ends, uint64_t *moves, size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= local_affine_oracle(seq1s + len1 * (size_t)k, len1, seq2s + 128 * (size_t)k, sm, open, extend, scores + k,
                                  ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL, steps ? steps + k : NULL);
    return rc;
}
