// local_full_affine_kernels.hip -- gfx950 kernel of the local aligner for two sequences of any length with AFFINE gaps, end
// cell, start cell and traceback (swmi_local_full_affine*).
//
// Semantics (include/swmi.h): swmi_local_full's borders and zero floor with Gotoh's gaps, a gap of
// length k costing open + (k-1) extend:
//     H(i,0) = H(0,j) = 0,  E(0,j) = F(i,0) = -inf
//     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap (an up move)
//     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap (a left move)
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j)),   i = 1..len1, j = 1..len2
// The end cell is the first cell in row-major order holding max H ((0,0) when that is 0).  The walk goes back from it in
// state H: it stops at the first cell holding 0 (the test comes first), else takes a diagonal, else enters E, else F; inside
// E / F it takes up / left steps and returns to H where the gap opened (opening wins a tie).
//
// Mapping, ring timing, best-cell rule and code layout: tile_sweep.h, which also holds the constants, the helpers and the
// launcher.  The sweep and the walk are written out here and not taken from tile_sweep_body.inc: with the (H, F) carry and
// the two-dword code behind the body's types the compiler allocated other registers and other loops (DESIGN.md section
// 13), so this kernel keeps the code it had.
// E runs down a column and stays with the lane; F runs along the row, so the Carry from lane l - 1 (and through the ring) is
// its H(i, 16 G) and its F(i, 16 G), as in sgfull_affine_kernels.hip.
//
// The cell as KEYS: key = value << 6 | tag << 4 | low.  A stored H key has tag 2 and low = 15 - jj (jj = the column within
// the lane); with a traceback E is kept masked to tag 1 and F to tag 0 (one v_and_or_b32 after their max).  Every candidate
// is one add away from a neighbour's key:
//     floor     = 0 << 6 | 3 << 4              tag 3: the constant 48, an inline operand
//     diag      = key(i-1,j-1) + s << 6        tag 2              E's open = key(i-1,j) - open << 6    tag 2
//     E(i,j)    as kept                        tag 1              E's ext  = E(i-1,j) - extend << 6   tag 1
//     F(i,j)    as kept                        tag 0              F's open = key(i,j-1) - open << 6    tag 2
//                                                                 F's ext  = F(i,j-1) - extend << 6   tag 0
// so one v_max3_i32 and one v_max_i32 pick H's largest candidate and, among equal values, the floor before diagonal before
// E before F: at value 0 every other candidate is at most 0 << 6 | 2 << 4 | 15 = 47 < 48, so the floor wins every tie at 0,
// and a candidate below 0 is a negative key.  The winner's tag is the cell's CODE: 3 = stop, 2 = diagonal, 1 = E, 0 = F.
// Each of E's and F's maxes prefers opening on equal values (tag 2 above tag 1 and tag 0), and bit 5 of its winner is the
// open bit.  The low 4 bits never carry into the tag and never decide between two candidates (their tags differ).
// Ends-only only H's values and the best key's column matter, so E and F are not masked.  H lies in [0, 2^21)
// (127 * 16384 < 2^21), and wherever E or F derives from an H it is at least -open >= -127 and at most H, so apart from the
// sentinel every key lies in (-2^14, 2^27); -inf = -2^30 is only ever extended once before an open candidate replaces it
// (E(1,j) and F(i,1) always open), so -2^30 - (127 << 6) is the lowest key: no overflow, and far below every real key.
//
// Borders: row 0 and column 0 hold the stored key of H = 0, a constant; E on row 0 and F into wave 0's lane 0 are -inf, so
// E(1,j) and F(i,1) always open.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128; with the floor they hold values
// >= 0.  Induction over the cells in row-major order: a padded cell p = (i, j) holds 0, or its diagonal candidate (a cell of
// the row above, valid or padded, minus 128), or E(i,j) = the largest of H(k,j) - open - (i-1-k) extend over k < i (each
// H(k,j) a padded cell of an earlier row, or H(0,j) = 0), or F(i,j) = the largest of H(i,k) - open - (j-1-k) extend over
// k < j (each H(i,k) a valid cell of the same row or a padded cell left of p, all before p).  Every gap cost is >= 0, so each
// source is a valid cell earlier in row-major order or a padded cell earlier in it, which by induction is at most some
// valid cell earlier still.  So a padded cell above 0 is at most some valid cell EARLIER in row-major order -- also at
// open = 0, where "at most" may be "equal" -- and a padded cell holding 0 never beats the initial best of 0.  The best-cell
// rule (strictly greater; then row, then column ascending) never picks a padded cell.  What padded columns compute flows
// only right and down, into other padded columns, and the walk only moves up and left from a valid cell, so it never
// enters one.
//
// Codes: section 16's 4 bits per cell, one qword per lane and row: the low dword holds H's code of the lane's 16 columns
// (2 bits each), the high one E's open bit of column jj at bit jj and F's at bit 16 + jj.
//
// Walk: a staging block is 128 rows x 32 lanes (512 columns) of qwords; the walking lane carries its state (H / E / F) from
// block to block.  The walk ends on a stop code read in state H (inside E or F the cell's H code is not consulted), on row 0
// or on column 0 (border cells hold 0 and have no code); since E(1,j) and F(i,1) always open, it arrives on a border in
// state H.
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

// The geometry this file's proofs, bounds and code word were written against (tile_sweep.h owns it; a change there must
// revisit them)
namespace written_for {
constexpr int kCols = 16;
constexpr int kMaxWaves = 16;
constexpr int kUnroll = 4;
constexpr int kChunk = 32;
constexpr int kDelay = 3;
constexpr int kRing = 256;
constexpr int kStageRows = 128;
static_assert(kCols == tile::kCols && kMaxWaves == tile::kMaxWaves && kUnroll == tile::kUnroll && kChunk == tile::kChunk &&
              kDelay == tile::kDelay && kRing == tile::kRing && kStageRows == tile::kStageRows);
}  // namespace written_for

constexpr int kStageLanes = 32;
constexpr int kFloor = 3 << 4;         // the floor candidate: H = 0, tag 3
constexpr int kStored = 2 << 4;        // tag of a stored H key (= the diagonal's and both open candidates')
constexpr int kTagE = 1 << 4;
constexpr int kTagF = 0 << 4;
constexpr int kOpenBit = 5;            // of E's and of F's winner: set when the gap opens here
constexpr uint32_t kStop = 3;          // code of a cell whose floor won
constexpr int kMinusInf = -(1 << 30);  // E on row 0, F on column 0

// RAGGED: one TileWork per workgroup (work[blockIdx.x]) names the alignment, and the launch's own shape (fixed_*, move_words)
// is unused; else `work` is NULL and unread (tile_sweep.h).
template <bool TB, bool RAGGED = false>
__global__ __launch_bounds__(64 * kMaxWaves) void local_full_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int fixed_len1, int fixed_len2, SmCols cols, int gap_open,
    int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends, unsigned long long *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps, uint32_t move_words, uint32_t fixed_trips,
    const TileWork *__restrict__ work)
{
    const TileWork slot = load_slot<RAGGED>(work);
    const int len1 = RAGGED ? (int)slot.len1 : fixed_len1, len2 = RAGGED ? (int)slot.len2 : fixed_len2;
    const uint32_t n_trips = RAGGED ? (uint32_t)trips(len1) : fixed_trips;
    __shared__ int2 ring[(kMaxWaves - 1) * kRing];
    __shared__ unsigned long long red[kMaxWaves];
    __shared__ int walk_at[3];
    __shared__ unsigned long long stage[TB ? kStageRows * kStageLanes : 1];

    const int W = blockDim.x >> 6;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, G = tid;
    const size_t k = RAGGED ? (size_t)slot.k : (size_t)blockIdx.x;
    const uint8_t *s1 = seq1s + (RAGGED ? (size_t)slot.s1_off : k * (size_t)len1);
    const uint8_t *s2 = seq2s + (RAGGED ? (size_t)slot.s2_off : k * (size_t)len2);
    if constexpr (RAGGED) {
        // a slot with a zero length: the whole workgroup (one wavefront) leaves here, before any barrier and any sequence load
        if (len1 == 0 || len2 == 0) {
            if (tid == 0) {
                scores[k] = 0;
                ends[4 * k + 0] = 0;
                ends[4 * k + 1] = 0;
                ends[4 * k + 2] = TB ? 0 : -1;
                ends[4 * k + 3] = TB ? 0 : -1;
                if constexpr (TB) steps[k] = 0;
            }
            return;
        }
    }
    const int jbase = kCols * G;                        // the lane's columns are jbase + 1 .. jbase + 16

    uint32_t prof[kCols];
    int key[kCols], e[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const int j = jbase + jj + 1;
        const uint32_t b = s2[j <= len2 ? j - 1 : 0] & 3u;
        prof[jj] = j > len2 ? 0x80808080u : b == 0 ? cols.c[0] : b == 1 ? cols.c[1] : b == 2 ? cols.c[2] : cols.c[3];
        key[jj] = kStored | (kCols - 1 - jj);           // row 0 holds 0
        e[jj] = kMinusInf;
    }
    const int g_open = -(gap_open << 6);
    const int g_ext = -(gap_extend << 6);
    int diag_in = kStored;                              // key(0, jbase): H = 0
    int f_last = kMinusInf;                             // F(i, jbase + 16) of the lane's last row, for lane l + 1
    int best = kStored, best_row = 0;                   // H = 0 at (0, 0)

    const int local_chunks = (len1 + 63 + kChunk - 1) / kChunk;
    const int total_chunks = local_chunks + kDelay * (W - 1);
    const int2 *ring_in = ring + (w > 0 ? w - 1 : 0) * kRing;  // read by waves 1.. (wave 0's left column is the border)
    int2 *ring_out = ring + (w < W - 1 ? w : 0) * kRing;       // written by waves ..W-2
    unsigned long long *cw_out = TB ? codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)W * n_trips * 256)) +
                                          ((size_t)w * n_trips * 64 + l) * 4
                                    : nullptr;

    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) sh_next[t] = base_shift(s1, t - l, len1);

    for (int c = 0; c < total_chunks; ++c) {
        const int lc = c - kDelay * w;
        if (lc >= 0 && lc < local_chunks) {
            for (int q = 0; q < kChunk / kUnroll; ++q) {
                const int s0 = lc * kChunk + q * kUnroll;
                int sh[kUnroll], bound_h[kUnroll], bound_f[kUnroll], edge_h[kUnroll], edge_f[kUnroll];
                uint32_t cw[kUnroll], co[kUnroll];
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    sh[t] = sh_next[t];
                    sh_next[t] = base_shift(s1, s0 + kUnroll + t - l, len1);
                    // lane 0's left column for row s0 + t + 1: the ring, or the border's H = 0 and F = -inf
                    if (w > 0) {
                        const int2 v = ring_in[(s0 + t) & (kRing - 1)];
                        bound_h[t] = v.x;
                        bound_f[t] = v.y;
                    } else {
                        bound_h[t] = kStored;
                        bound_f[t] = kMinusInf;
                    }
                    cw[t] = 0;
                    co[t] = 0;
                }
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    const int left_in = from_left(bound_h[t], key[kCols - 1]);   // lane l-1's key(i, jbase), one step ago
                    const int f_in = from_left(bound_f[t], f_last);              // ... and its F(i, jbase)
                    const int row = s0 + t - l + 1;
                    if (row >= 1 && row <= len1) {
                        int d = diag_in, lft = left_in, f = f_in, rk = 0;
#pragma unroll
                        for (int jj = 0; jj < kCols; ++jj) {
                            const int sc = __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                            const int ev = imax(key[jj] + g_open, e[jj] + g_ext);
                            const int fv = imax(lft + g_open, f + g_ext);
                            int ec = ev, fc = fv;
                            if constexpr (TB) {
                                ec = (ev & ~63) | kTagE;
                                fc = (fv & ~63) | kTagF;
                            }
                            const int m = imax(max3(d + (sc << 6), ec, fc), kFloor);
                            const int nk = (m & ~63) | (kStored | (kCols - 1 - jj));
                            if constexpr (TB) {
                                cw[t] |= ((uint32_t)(m >> 4) & 3u) << (2 * jj);
                                co[t] |= (((uint32_t)ev >> kOpenBit) & 1u) << jj;
                                co[t] |= (((uint32_t)fv >> kOpenBit) & 1u) << (16 + jj);
                            }
                            d = key[jj];
                            key[jj] = nk;
                            e[jj] = ec;
                            f = fc;
                            lft = nk;
                            rk = rk > nk ? rk : nk;
                        }
                        f_last = f;
                        if (rk > (best | 63)) {
                            best = rk;
                            best_row = row;
                        }
                    }
                    edge_h[t] = key[kCols - 1];
                    edge_f[t] = f_last;
                    diag_in = left_in;
                }
                if (w < W - 1 && l == 63) {
#pragma unroll
                    for (int t = 0; t < kUnroll; ++t) {
                        const int row = s0 + t - 62;
                        if (row >= 1 && row <= len1) ring_out[(row - 1) & (kRing - 1)] = make_int2(edge_h[t], edge_f[t]);
                    }
                }
                if constexpr (TB) {
                    uint4 *o = reinterpret_cast<uint4 *>(cw_out + (size_t)(s0 >> 2) * 256);
                    o[0] = make_uint4(cw[0], co[0], cw[1], co[1]);
                    o[1] = make_uint4(cw[2], co[2], cw[3], co[3]);
                }
            }
        }
        if (W > 1) __syncthreads();
    }

    // best cell: (H desc, row asc, column asc) over the lanes, then over the waves
    const int h = best >> 6;
    const int col = h > 0 ? jbase + (kCols - 1 - (best & 15)) + 1 : 0;
    unsigned long long r = ((unsigned long long)(uint32_t)h << 34) | ((unsigned long long)(0x1FFFF - best_row) << 17) |
                           (unsigned long long)(0x1FFFF - col);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long v = __shfl_xor(r, o, 64);
        r = v > r ? v : r;
    }
    if (l == 0) red[w] = r;
    if constexpr (TB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's code stores have reached L2
    __syncthreads();
    r = red[0];
    for (int x = 1; x < W; ++x) r = red[x] > r ? red[x] : r;
    const int score = (int)(r >> 34);
    const int end_i = score > 0 ? 0x1FFFF - (int)((r >> 17) & 0x1FFFF) : 0;
    const int end_j = score > 0 ? 0x1FFFF - (int)(r & 0x1FFFF) : 0;
    if (tid == 0) {
        scores[k] = score;
        ends[4 * k + 0] = end_i;
        ends[4 * k + 1] = end_j;
        if constexpr (!TB) {
            ends[4 * k + 2] = -1;
            ends[4 * k + 3] = -1;
        }
    }
    if constexpr (TB) {
        const unsigned long long *cd = codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)W * n_trips * 256));
        unsigned long long *mv = moves + (RAGGED ? (size_t)slot.move_base : k * (size_t)move_words);
        int i = end_i, j = end_j, stopped = 0;
        int state = 0;                                  // 0 = H, 1 = E, 2 = F (thread 0's only)
        uint32_t t = 0;
        unsigned long long acc = 0;
        while (!stopped && i > 0 && j > 0) {            // uniform: every thread holds the same (i, j, stopped)
            const int g1 = (j - 1) >> 4;
            const int i_lo = i - kStageRows + 1 > 1 ? i - kStageRows + 1 : 1;
            const int g_lo = g1 - kStageLanes + 1 > 0 ? g1 - kStageLanes + 1 : 0;
            const int rows = i - i_lo + 1, lanes = g1 - g_lo + 1;
            for (int x = tid; x < rows * lanes; x += blockDim.x) {
                const int rr = x / lanes, gg = x - rr * lanes;
                stage[rr * kStageLanes + gg] = __builtin_nontemporal_load(cd + code_index(i_lo + rr, g_lo + gg, n_trips));
            }
            __syncthreads();
            if (tid == 0) {
                int st = 0;
                while (i > 0 && j > 0 && i >= i_lo && ((j - 1) >> 4) >= g_lo) {
                    const unsigned long long wd = stage[(i - i_lo) * kStageLanes + ((j - 1) >> 4) - g_lo];
                    const int cc = (j - 1) & 15;
                    if (state == 0) {
                        const uint32_t hc = (uint32_t)(wd >> (2 * cc)) & 3u;
                        if (hc == kStop) {              // the cell holds 0: the start cell
                            st = 1;
                            break;
                        }
                        state = hc == 2u ? 0 : hc == 1u ? 1 : 2;
                    }
                    uint32_t mvc;
                    if (state == 0) {
                        mvc = 3;                        // diagonal
                        --i;
                        --j;
                    } else if (state == 1) {
                        mvc = 2;                        // up, inside E; back to H where E opened
                        state = (wd >> (32 + cc)) & 1u ? 0 : 1;
                        --i;
                    } else {
                        mvc = 1;                        // left, inside F; back to H where F opened
                        state = (wd >> (48 + cc)) & 1u ? 0 : 2;
                        --j;
                    }
                    acc |= (unsigned long long)mvc << (2 * (t & 31));
                    ++t;
                    if ((t & 31) == 0) {
                        mv[(t >> 5) - 1] = acc;
                        acc = 0;
                    }
                }
                walk_at[0] = i;
                walk_at[1] = j;
                walk_at[2] = st;
            }
            __syncthreads();
            i = walk_at[0];
            j = walk_at[1];
            stopped = walk_at[2];
        }
        if (tid == 0) {
            if (t & 31) mv[t >> 5] = acc;
            steps[k] = t;
            ends[4 * k + 2] = i;
            ends[4 * k + 3] = j;
        }
    }
}

}  // namespace

// qwords of codes per alignment: 4 bits per cell of every lane's 16 columns, for every step of the padded sweep
size_t local_full_affine_code_qwords(int len1, int len2) { return tile::code_words(len1, len2); }

hipError_t launch_local_full_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                    int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, size_t move_words, hipStream_t stream)
{
    return tile::launch<local_full_affine_kernel<true>, local_full_affine_kernel<false>>(d_seq1s, d_seq2s, len1, len2, n, sm, d_scores, d_ends, d_codes, d_moves, d_steps,
        move_words, stream, gap_open, gap_extend);
}

hipError_t launch_local_full_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                           int waves, const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores,
                                           int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                           uint32_t *d_steps, hipStream_t stream)
{
    return tile::launch_ragged<local_full_affine_kernel<true, true>, local_full_affine_kernel<false, true>>(
        d_seq1s, d_seq2s, d_work, n, waves, sm, d_scores, d_ends, d_codes, d_moves, d_steps, stream, gap_open, gap_extend);
}

}  // namespace swmi
