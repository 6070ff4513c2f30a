/* local_full_affine_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the any-length affine local aligner's
 * semantics (include/swmi.h, swmi_local_full_affine) for any lengths, int8 matrix, gap_open and gap_extend, compiled by the
 * local_full_affine tests into pytest's temporary directory.
 *
 *     H(i,0) = H(0,j) = 0,  E(0,j) = F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     end cell  = the first cell in row-major order whose H is strictly greater than every earlier one (from 0 at (0,0))
 *     walk      = state H: stop at H == 0, else diagonal if H == H(i-1,j-1) + s, else state E if H == E, else state F;
 *                 state E: up, then state H if E == H(i-1,j) - open, else stay E; state F: left, likewise
 *
 * Two rolling rows of H and of E, F as a running value along the row, and 4 bits per cell of what the walk needs there
 * (bits 0-1: 0 = stop, 3 = diagonal, 2 = H is E, 1 = H is F; bit 2: E opened here; bit 3: F opened here) instead of the
 * three whole tables; nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define MINUS_INF (-(1 << 28))

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell, 3 / 2 / 1 = diagonal / up / left (NULL: ends
 * only, start cell (-1, -1)).  ends = (end_i, end_j, start_i, start_j).  Returns 0, or -1 if memory runs out. */
int local_full_affine_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, const int8_t *sm, int open,
                             int extend, int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    const size_t W = len2 + 1, row_bytes = (W + 1) / 2;
    int32_t *hp = (int32_t *)calloc(W, sizeof(int32_t)), *hc = (int32_t *)calloc(W, sizeof(int32_t));
    int32_t *e = (int32_t *)malloc(W * sizeof(int32_t));
    uint8_t *codes = moves ? (uint8_t *)calloc((len1 + 1) * row_bytes, 1) : NULL;
    if (!hp || !hc || !e || (moves && !codes)) {
        free(hp);
        free(hc);
        free(e);
        free(codes);
        return -1;
    }
    for (size_t j = 0; j < W; ++j) e[j] = MINUS_INF;
    int best = 0, bi = 0, bj = 0;
    for (size_t i = 1; i <= len1; ++i) {
        hc[0] = 0;
        int f = MINUS_INF;
        uint8_t *crow = codes ? codes + i * row_bytes : NULL;
        for (size_t j = 1; j <= len2; ++j) {
            const int eo = hp[j] - open, ee = e[j] - extend;
            const int fo = hc[j - 1] - open, fe = f - extend;
            const int E = eo > ee ? eo : ee;
            const int F = fo > fe ? fo : fe;
            const int d = hp[j - 1] + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            int h = 0;
            if (d > h) h = d;
            if (E > h) h = E;
            if (F > h) h = F;
            e[j] = E;
            f = F;
            hc[j] = h;
            if (crow) {
                const unsigned c = (h == 0 ? 0u : h == d ? 3u : h == E ? 2u : 1u) | (E == eo ? 4u : 0u) | (F == fo ? 8u : 0u);
                crow[j >> 1] |= (uint8_t)(c << (4 * (j & 1)));
            }
            if (best < h) {
                best = h;
                bi = (int)i;
                bj = (int)j;
            }
        }
        int32_t *t = hp;
        hp = hc;
        hc = t;
    }
    uint32_t t = 0;
    int i = bi, j = bj, state = 0;   /* 0 = H, 1 = E, 2 = F */
    if (moves) {
        while (i > 0 && j > 0) {
            const unsigned c = (codes[(size_t)i * row_bytes + ((size_t)j >> 1)] >> (4 * (j & 1))) & 15u;
            unsigned m;
            if (state == 0) {
                if ((c & 3u) == 0) break;
                state = (c & 3u) == 3u ? 0 : (c & 3u) == 2u ? 1 : 2;
            }
            if (state == 0) {
                m = 3;
                --i;
                --j;
            } else if (state == 1) {
                m = 2;
                state = c & 4u ? 0 : 1;
                --i;
            } else {
                m = 1;
                state = c & 8u ? 0 : 2;
                --j;
            }
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            ++t;
        }
    } else {
        i = j = -1;
    }
    free(hp);
    free(hc);
    free(e);
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
int local_full_affine_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                   const int8_t *sm, int open, int extend, int32_t *scores, int32_t *ends, uint64_t *moves,
                                   size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= local_full_affine_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, sm, open, extend,
                                       scores + k, ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL,
                                       steps ? steps + k : NULL);
    return rc;
}
