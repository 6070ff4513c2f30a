/* banded_global_oracle.c -- TEST INFRASTRUCTURE ONLY: a plain restatement of the banded global / fit / overlap / extension
 * aligner's contract (include/swmi_banded_global.h), compiled by the banded_global tests into pytest's temporary directory.
 *
 *     cell (i, j), 0 <= i <= len1, 0 <= j <= len2, is in the band iff lo <= (j - i) - d0 <= hi     (the contract: -64, 63)
 *     free_ends: 1 = BEGIN1, 2 = BEGIN2, 4 = END1, 8 = END2, 16 = END_ANYWHERE
 *     every cell out of the band or off the table: H = E = F = -inf
 *     in-band border: H(0,0) = 0; H(0,j) = BEGIN2 ? 0 : (0,0) in the band ? -(open + (j-1) extend) : -inf; H(i,0) likewise with
 *                     BEGIN1; E = F = -inf
 *     in-band cells with i, j >= 1:
 *         E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)
 *         F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)
 *         H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 *     end cell = of the in-band cells among (len1, len2), column len2 with END1, row len1 with END2, every cell with
 *                END_ANYWHERE the largest H, the first in row-major order among equal ones; none, or -inf: NO ALIGNMENT
 *                (score INT32_MIN, ends 0 0 0 0 or 0 0 -1 -1, no steps)
 *     walk     = while i > 0 and j > 0: state H: diagonal if H == H(i-1,j-1) + s, else state E if H == E, else state F;
 *                state E: up, then state H if E == H(i-1,j) - open, else stay E; state F: left, likewise.  On row 0 it ends if
 *                BEGIN2 (or j = 0), else goes left to (0,0); on column 0 it ends if BEGIN1, else goes up to (0,0).
 *
 * Band-only storage: three matrices of (len1 + 1) x (hi - lo + 1) int64, column (j - i) - d0 - lo of row i.  -inf is -2^50
 * and absorbing: whatever is added to it or taken from it, it stays -2^50, and nothing finite comes near -2^40.
 * lo and hi are arguments so that a test can show what a band that is off by one gets wrong.  Nothing here is tuned. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define NEG (-(1LL << 50))
#define IS_NEG(v) ((v) < -(1LL << 40))

typedef struct {
    int64_t *h, *e, *f;
    long long len1, len2, width, d0;
    int lo, hi;
} band_t;

/* the slot of (i, j), or -1 where the cell is off the table or outside the band */
static long long slot(const band_t *b, long long i, long long j)
{
    if (i < 0 || j < 0 || i > b->len1 || j > b->len2) return -1;
    const long long d = (j - i) - b->d0;
    if (d < b->lo || d > b->hi) return -1;
    return i * b->width + (d - b->lo);
}
static int64_t get(const band_t *b, const int64_t *m, long long i, long long j)
{
    const long long s = slot(b, i, j);
    return s < 0 ? NEG : m[s];
}
static int64_t max2(int64_t a, int64_t b) { return a > b ? a : b; }
/* -inf stays -inf whatever is taken from it */
static int64_t minus(int64_t v, int by) { return IS_NEG(v) ? NEG : v - by; }

int banded_global_oracle(const uint8_t *seq1, size_t len1, const uint8_t *seq2, size_t len2, int32_t diagonal, int lo, int hi,
                         const int8_t *sm, int open, int extend, unsigned free_ends, int32_t *score, int32_t ends[4], uint64_t *moves,
                         uint32_t *steps)
{
    const int begin1 = free_ends & 1, begin2 = free_ends & 2, end1 = free_ends & 4, end2 = free_ends & 8, anywhere = free_ends & 16;
    band_t b;
    b.len1 = (long long)len1;
    b.len2 = (long long)len2;
    b.width = hi - lo + 1;
    b.d0 = diagonal;
    b.lo = lo;
    b.hi = hi;
    const size_t cells = (len1 + 1) * (size_t)b.width;
    b.h = (int64_t *)malloc(cells * sizeof(int64_t));
    b.e = (int64_t *)malloc(cells * sizeof(int64_t));
    b.f = (int64_t *)malloc(cells * sizeof(int64_t));
    if (!b.h || !b.e || !b.f) {
        free(b.h);
        free(b.e);
        free(b.f);
        return -1;
    }
    for (size_t x = 0; x < cells; ++x) b.h[x] = b.e[x] = b.f[x] = NEG;
    const int origin = slot(&b, 0, 0) >= 0;
    int have = 0;
    int64_t best = NEG;
    long long bi = 0, bj = 0;
    for (long long i = 0; i <= b.len1; ++i) {
        long long j_lo = i + b.d0 + lo, j_hi = i + b.d0 + hi;
        if (j_lo < 0) j_lo = 0;
        if (j_hi > b.len2) j_hi = b.len2;
        for (long long j = j_lo; j <= j_hi; ++j) {
            const long long s = slot(&b, i, j);
            int64_t h, e = NEG, f = NEG;
            if (i == 0 && j == 0) {
                h = 0;
            } else if (i == 0) {
                h = begin2 ? 0 : origin ? -((int64_t)open + (j - 1) * extend) : NEG;
            } else if (j == 0) {
                h = begin1 ? 0 : origin ? -((int64_t)open + (i - 1) * extend) : NEG;
            } else {
                e = max2(minus(get(&b, b.h, i - 1, j), open), minus(get(&b, b.e, i - 1, j), extend));
                f = max2(minus(get(&b, b.h, i, j - 1), open), minus(get(&b, b.f, i, j - 1), extend));
                const int64_t up_left = get(&b, b.h, i - 1, j - 1);
                const int64_t d = IS_NEG(up_left) ? NEG : up_left + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)];
                h = max2(d, max2(e, f));
            }
            b.h[s] = h;
            b.e[s] = e;
            b.f[s] = f;
            const int candidate = anywhere || (i == b.len1 && j == b.len2) || (end1 && j == b.len2) || (end2 && i == b.len1);
            if (candidate && !IS_NEG(h) && (!have || h > best)) {
                have = 1;
                best = h;
                bi = i;
                bj = j;
            }
        }
    }
    uint32_t t = 0;
    long long i = bi, j = bj;
    if (!have) {
        *score = INT32_MIN;
        ends[0] = ends[1] = 0;
        ends[2] = ends[3] = moves ? 0 : -1;
    } else {
        int state = 0; /* 0 = H, 1 = E, 2 = F */
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
                    if (state == 0) {
                        const int64_t h = get(&b, b.h, i, j), up_left = get(&b, b.h, i - 1, j - 1);
                        if (!IS_NEG(up_left) && h == up_left + sm[(seq1[i - 1] & 3) * 4 + (seq2[j - 1] & 3)]) state = 0;
                        else if (h == get(&b, b.e, i, j)) state = 1;
                        else state = 2;
                    }
                    if (state == 0) {
                        m = 3;
                    } else if (state == 1) {
                        m = 2;
                        state = get(&b, b.e, i, j) == minus(get(&b, b.h, i - 1, j), open) ? 0 : 1;
                    } else {
                        m = 1;
                        state = get(&b, b.f, i, j) == minus(get(&b, b.h, i, j - 1), open) ? 0 : 2;
                    }
                }
                if ((t & 31) == 0) moves[t >> 5] = 0;
                moves[t >> 5] |= (uint64_t)m << (2 * (t & 31));
                i -= m != 1;
                j -= m != 2;
                ++t;
            }
        }
        *score = (int32_t)best;
        ends[0] = (int32_t)bi;
        ends[1] = (int32_t)bj;
        ends[2] = moves ? (int32_t)i : -1;
        ends[3] = moves ? (int32_t)j : -1;
    }
    free(b.h);
    free(b.e);
    free(b.f);
    if (steps) *steps = t;
    return 0;
}

/* n alignments, seq1 k at seq1s + len1 k, seq2 k at seq2s + len2 k; diagonals NULL: all 0; moves rows of `move_words` words
 * (NULL: ends only) */
int banded_global_oracle_batch(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int32_t *diagonals,
                               int lo, int hi, const int8_t *sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                               uint64_t *moves, size_t move_words, uint32_t *steps)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(| : rc)
    for (long k = 0; k < (long)n; ++k)
        rc |= banded_global_oracle(seq1s + len1 * (size_t)k, len1, seq2s + len2 * (size_t)k, len2, diagonals ? diagonals[k] : 0, lo, hi, sm,
                                   open, extend, free_ends, scores + k, ends + 4 * k, moves ? moves + move_words * (size_t)k : NULL,
                                   steps ? steps + k : NULL);
    return rc;
}
