/* sgfull_affine_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the affine exact semi-global aligner's semantics
 * (include/swmi.h, swmi_semiglobal_full_affine) for any lengths, int8 matrix, gap_open and gap_extend, compiled by the tests
 * into pytest's temporary directory.
 *
 *     H(0,0) = 0, H(0,j) = -(open + (j-1) extend), H(i,0) = -(open + (i-1) extend), E(0,j) = F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     best cell = the first cell in row-major order whose H is strictly greater than every earlier one (from 0 at (0,0))
 *     walk      = state H: diagonal if H == diag, else state E if H == E, else state F; state E: up, then H if E opened
 *                 (opening wins a tie), else E; state F: left likewise; forced up / left on column 0 / row 0
 *
 * Rolling rows of H and E and one running F, plus 4 bits per cell for the walk (H's choice 3 / 2 / 1 = diagonal / E / F,
 * E's open bit, F's open bit); nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG_INF (-(1 << 29))

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the best cell.  ends = (i, j).  *length = steps + 1.
 * Returns 0, or -1 if memory runs out. */
int sgfull_affine_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, const int8_t *sm, int open, int ext,
                         int32_t *score, int32_t ends[2], uint64_t *moves, uint32_t *length)
{
    const size_t W = len2 + 1;
    int32_t *hp = (int32_t *)malloc(W * sizeof(int32_t)), *hc = (int32_t *)malloc(W * sizeof(int32_t));
    int32_t *e = (int32_t *)malloc(W * sizeof(int32_t));
    /* 4 bits per cell (two cells per byte): bits 0-1 H's choice, bit 2 E's open bit, bit 3 F's open bit */
    uint8_t *codes = moves ? (uint8_t *)calloc(((len1 + 1) * W + 1) / 2, 1) : NULL;
    if (!hp || !hc || !e || (moves && !codes)) {
        free(hp);
        free(hc);
        free(e);
        free(codes);
        return -1;
    }
    int best = 0, bi = 0, bj = 0;
    hp[0] = 0;
    for (size_t j = 1; j <= len2; ++j) hp[j] = -(open + (int)(j - 1) * ext);
    for (size_t j = 0; j <= len2; ++j) e[j] = NEG_INF;
    for (size_t i = 1; i <= len1; ++i) {
        hc[0] = -(open + (int)(i - 1) * ext);
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
    if (moves) {
        int i = bi, j = bj, state = 0;   /* 0 = H, 1 = E, 2 = F */
        while (i > 0 || j > 0) {
            unsigned m;
            if (i == 0) {
                m = 1;
            } else if (j == 0) {
                m = 2;
            } else {
                const size_t at = (size_t)i * W + j;
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
    free(codes);
    *score = best;
    ends[0] = bi;
    ends[1] = bj;
    if (length) *length = t + 1;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 k, seq2 k at seq2s + len2 k; moves rows of `move_words` words (NULL: ends only) */
int sgfull_affine_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t *sm,
                               int open, int ext, int32_t *scores, int32_t *ends, uint64_t *moves, size_t move_words,
                               uint32_t *lengths)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= sgfull_affine_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, sm, open, ext, scores + k,
                                   ends + 2 * k, moves ? moves + move_words * (size_t)k : NULL, lengths ? lengths + k : NULL);
    return rc;
}
