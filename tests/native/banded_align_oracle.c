/* banded_align_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the banded local aligner's contract
 * (include/swmi_banded.h), compiled by the banded_align tests into pytest's temporary directory.
 *
 *     cell (i, j) is in the band iff lo <= (j - i) - d0 <= hi            (the contract: lo = -64, hi = 63)
 *     for in-band cells with 1 <= i <= len1, 1 <= j <= len2:
 *         E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *         F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *         H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     every other cell: H = 0, E = F = -inf
 *     end cell = the first cell in row-major order whose H is strictly greater than every earlier one (from 0 at (0,0))
 *     walk     = state H: stop at H == 0, else diagonal if H == H(i-1,j-1) + s, else state E if H == E, else state F;
 *                state E: up, then state H if E == H(i-1,j) - open, else stay E; state F: left, likewise
 *
 * Band-only storage: three matrices of (len1 + 1) x (hi - lo + 3) int32 (130 columns for the contract's band), column
 * 1 + (j - i) - d0 - lo of row i; a full table at 16384 x 16384 would not fit.  lo and hi are arguments so that a test can
 * show what a band that is off by one gets wrong.  Nothing here is tuned.  Bases are taken modulo 4. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define MINUS_INF (-(1 << 28))

typedef struct {
    int32_t *h, *e, *f;
    size_t len1, len2, width;
    long long d0;
    int lo, hi;
} band_t;

/* the slot of (i, j), or -1 where the cell is on the border, outside the table or outside the band */
static long long slot(const band_t *b, long long i, long long j)
{
    if (i < 1 || j < 1 || i > (long long)b->len1 || j > (long long)b->len2) return -1;
    const long long d = (j - i) - b->d0;
    if (d < b->lo || d > b->hi) return -1;
    return i * (long long)b->width + 1 + (d - b->lo);
}
static int H(const band_t *b, long long i, long long j) { const long long s = slot(b, i, j); return s < 0 ? 0 : b->h[s]; }
static int E(const band_t *b, long long i, long long j) { const long long s = slot(b, i, j); return s < 0 ? MINUS_INF : b->e[s]; }
static int F(const band_t *b, long long i, long long j) { const long long s = slot(b, i, j); return s < 0 ? MINUS_INF : b->f[s]; }

/* moves: (len1 + len2 + 31) / 32 words or more, walking order from the end cell, 3 / 2 / 1 = diagonal / up / left (NULL: ends
 * only, start cell (-1, -1)).  ends = (end_i, end_j, start_i, start_j).  Returns 0, or -1 if memory runs out. */
int banded_align_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, int32_t diagonal, int lo, int hi,
                        const int8_t *sm, int open, int extend, int32_t *score, int32_t ends[4], uint64_t *moves, uint32_t *steps)
{
    band_t b;
    b.len1 = len1;
    b.len2 = len2;
    b.width = (size_t)(hi - lo + 3);
    b.d0 = diagonal;
    b.lo = lo;
    b.hi = hi;
    const size_t cells = (len1 + 1) * b.width;
    b.h = (int32_t *)calloc(cells, sizeof(int32_t));
    b.e = (int32_t *)calloc(cells, sizeof(int32_t));
    b.f = (int32_t *)calloc(cells, sizeof(int32_t));
    if (!b.h || !b.e || !b.f) {
        free(b.h);
        free(b.e);
        free(b.f);
        return -1;
    }
    int best = 0;
    long long bi = 0, bj = 0;
    for (long long i = 1; i <= (long long)len1; ++i) {
        long long j_lo = i + b.d0 + lo, j_hi = i + b.d0 + hi;
        if (j_lo < 1) j_lo = 1;
        if (j_hi > (long long)len2) j_hi = (long long)len2;
        for (long long j = j_lo; j <= j_hi; ++j) {
            const long long s = slot(&b, i, j);
            const int eo = H(&b, i - 1, j) - open, ee = E(&b, i - 1, j) - extend;
            const int fo = H(&b, i, j - 1) - open, fe = F(&b, i, j - 1) - extend;
            const int e = eo > ee ? eo : ee, f = fo > fe ? fo : fe;
            const int d = H(&b, i - 1, j - 1) + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
            int h = 0;
            if (d > h) h = d;
            if (e > h) h = e;
            if (f > h) h = f;
            b.h[s] = h;
            b.e[s] = e;
            b.f[s] = f;
            if (best < h) {
                best = h;
                bi = i;
                bj = j;
            }
        }
    }
    uint32_t t = 0;
    long long i = bi, j = bj;
    int state = 0; /* 0 = H, 1 = E, 2 = F */
    if (moves) {
        for (;;) {
            unsigned m;
            if (state == 0) {
                const int h = H(&b, i, j);
                if (h == 0) break;
                if (h == H(&b, i - 1, j - 1) + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)]) state = 0;
                else if (h == E(&b, i, j)) state = 1;
                else state = 2;
            }
            if (state == 0) {
                m = 3;
                --i;
                --j;
            } else if (state == 1) {
                m = 2;
                state = E(&b, i, j) == H(&b, i - 1, j) - open ? 0 : 1;
                --i;
            } else {
                m = 1;
                state = F(&b, i, j) == H(&b, i, j - 1) - open ? 0 : 2;
                --j;
            }
            if ((t & 31) == 0) moves[t >> 5] = 0;
            moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
            ++t;
        }
    } else {
        i = j = -1;
    }
    free(b.h);
    free(b.e);
    free(b.f);
    *score = best;
    ends[0] = (int32_t)bi;
    ends[1] = (int32_t)bj;
    ends[2] = (int32_t)i;
    ends[3] = (int32_t)j;
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 k, seq2 k at seq2s + len2 k; diagonals NULL: all 0; moves rows of `move_words` words
 * (NULL: ends only) */
int banded_align_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int32_t *diagonals,
                              int lo, int hi, const int8_t *sm, int open, int extend, int32_t *scores, int32_t *ends, uint64_t *moves,
                              size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= banded_align_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, diagonals ? diagonals[k] : 0, lo, hi, sm,
                                  open, extend, scores + k, ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL,
                                  steps ? steps + k : NULL);
    return rc;
}
