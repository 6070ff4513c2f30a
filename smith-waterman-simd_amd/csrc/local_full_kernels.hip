// local_full_kernels.hip -- gfx950 kernel of the local aligner for two sequences of any length, with end cell, start cell
// and traceback (swmi_local_full*).
//
// Semantics: swmi_local_align's (the reference's SmithWaterman_111_long, source.cpp:1526-1576) with a seq2 of len2 bases
// instead of 128, any int8 matrix and gap:
//     H(i,0) = H(0,j) = 0
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),   i = 1..len1, j = 1..len2
// The end cell is the first cell in row-major order holding max H ((0,0) when that is 0); the walk from it stops at the
// first cell holding 0 (the test comes first), else takes a diagonal, else an up, else a left step.  DESIGN.md section 17.
//
// Mapping: that of sgfull_kernels.hip, unchanged.  ONE workgroup per alignment,
// W = ceil(len2 / 1024) wavefronts; lane l of wave w owns the 16 columns 16 G + 1 .. 16 G + 16 of G = 64 w + l and computes
// row s - l + 1 at the wave's local step s; the column left of the lane comes from lane l - 1 one step earlier (one
// v_mov_b32_dpp wave_shr:1 per step), lane 0 of wave w > 0 takes it from lane 63 of wave w - 1 through an LDS ring of 256
// rows per wave boundary.  The waves run in chunks of 32 steps separated by a workgroup barrier, wave w three chunks behind
// wave w - 1; section 13's timing argument (every ring entry is written a chunk before it is read, 256 entries never wrap
// onto an unread one) carries over word for word, because neither the step at which a lane computes a row nor the ring's
// indexing depends on the recurrence.
//
// The cell as KEYS: key = H << 6 | tag << 4 | (15 - jj) (jj = the column within the lane).  H >= 0 and
// H <= 127 * 16384 < 2^21, so every stored key is positive and below 2^27.  A stored key has tag 2; the four candidates are
//     floor = 0 << 6 | 3 << 4                          (tag 3: the constant 48, an inline operand)
//     diag  = key(i-1,j-1) + s << 6                     (tag stays 2)
//     up    = key(i-1,j)   - gap << 6 - 1 << 4          (tag 1)
//     left  = key(i,j-1)   - gap << 6 - 2 << 4          (tag 0)
// so one v_max3_i32 and one v_max_i32 pick the largest value and, among equal values, the floor before diagonal before up
// before left: at value 0 the other candidates are at most 0 << 6 | 2 << 4 | 15 = 47 < 48, so the floor wins every tie at
// 0, and a candidate below 0 is a negative key.  The winner's tag is the cell's CODE: 3 = stop, 2 / 1 / 0 = diagonal / up /
// left (the move is code + 1).  The walker has no H to test: a stored stop code is what ends the walk.  One v_and_or_b32
// turns the winner back into a stored key.  The low 4 bits never carry into the tag and never decide between two
// candidates (their tags differ).
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128; with the floor they hold values
// >= 0.  Induction over the cells in row-major order: a padded cell holds 0, or its diagonal candidate (a cell of the row
// above, valid or padded, minus 128), or its up candidate (a padded cell of the row above minus gap >= 0), or its left
// candidate (the row's last valid cell or a padded cell left of it, minus gap >= 0).  Each of those is a valid cell earlier
// in row-major order or a padded cell earlier in it, which by induction is at most some valid cell earlier still.  So a
// padded cell above 0 is at most some valid cell EARLIER in row-major order -- also at gap 0, where "at most" may be
// "equal" -- and a padded cell holding 0 never beats the initial best of 0.  Valid columns are all smaller than padded
// ones, so the best-cell rule (strictly greater; then row, then column ascending) never picks a padded cell.  What padded
// columns compute flows only right and down, into other padded columns, and the walk only moves up and left from a valid
// cell, so it never enters one.
//
// Best cell: section 13's rule.  Per row, one max chain over the lane's 16 keys gives the row's largest H and its FIRST
// column (the low bits hold 15 - jj); it replaces the lane's best only when its H is strictly greater (compared against
// best | 63), so the lane keeps the first row.  Lanes and waves are reduced at the end (value desc, row asc, column asc).
//
// Codes: 2 bits per cell, one dword per lane and row; a lane keeps the 4 dwords of a trip (4 steps) and stores them as one
// 16-byte store: dword ((w * n_trips + s / 4) * 64 + l) * 4 + s % 4 of the alignment's codes holds row s - l + 1 of lane l.
//
// Walk: after the sweep every wave drains its stores (s_waitcnt vmcnt(0): a workgroup-scope fence lowers to nothing here,
// DESIGN.md section 12) and the workgroup meets at a barrier; then the whole workgroup loads a block of 128 rows x 64 lanes
// (1024 columns) of codes ending at the walk's cell into LDS, and one lane walks inside the block until it reads a stop
// code or reaches row 0 or column 0 (border cells hold 0 and have no code).
#include "swmi_internal.h"

namespace swmi {
namespace {

constexpr int kCols = 16;              // columns per lane
constexpr int kMaxWaves = 16;          // 16 x 64 x 16 = 16384 columns
constexpr int kUnroll = 4;             // steps per trip (one 16-byte code store)
constexpr int kChunk = 32;             // steps between two workgroup barriers
constexpr int kDelay = 3;              // chunks between wave w - 1 and wave w
constexpr int kRing = 256;             // rows of each wave boundary's LDS ring
constexpr int kStageRows = 128;        // walk staging block: rows x lanes (x 16 columns)
constexpr int kStageLanes = 64;
constexpr int kFloor = 3 << 4;         // the floor candidate: H = 0, tag 3
constexpr int kStored = 2 << 4;        // tag of a stored key (= the diagonal candidate's)
constexpr uint32_t kStop = 3;          // code of a cell whose floor won

__device__ __forceinline__ int max3(int a, int b, int c)
{
    const int m = a > b ? a : b;
    return m > c ? m : c;
}

// 8 * (seq1[idx] & 3), the load clamped into the sequence (so that it issues a trip ahead of its use)
__device__ __forceinline__ int base_shift(const uint8_t *s1, int idx, int len1)
{
    const int c = idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx;
    return 8 * (s1[c] & 3);
}

// cols[b] = bytes a = 0..3: sm[a*4 + b] -- the column of the score matrix that a seq2 base b selects
struct SmCols {
    uint32_t c[4];
};

__device__ __forceinline__ size_t code_index(int i, int G, uint32_t n_trips)
{
    const int w = G >> 6, l = G & 63, s = i + l - 1;
    return (((size_t)w * n_trips + (uint32_t)(s >> 2)) * 64 + l) * 4 + (s & 3);
}

template <bool TB>
__global__ __launch_bounds__(64 * kMaxWaves) void local_full_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                     int len1, int len2, SmCols cols, int gap, int32_t *__restrict__ scores,
                                                                     int32_t *__restrict__ ends, uint32_t *__restrict__ codes,
                                                                     unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps,
                                                                     uint32_t move_words, uint32_t n_trips)
{
    __shared__ int ring[(kMaxWaves - 1) * kRing];
    __shared__ unsigned long long red[kMaxWaves];
    __shared__ int walk_at[3];
    __shared__ uint32_t stage[TB ? kStageRows * kStageLanes : 1];

    const int W = blockDim.x >> 6;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, G = tid;
    const size_t k = blockIdx.x;
    const uint8_t *s1 = seq1s + k * (size_t)len1;
    const uint8_t *s2 = seq2s + k * (size_t)len2;
    const int jbase = kCols * G;                        // the lane's columns are jbase + 1 .. jbase + 16

    uint32_t prof[kCols];
    int key[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const int j = jbase + jj + 1;
        const uint32_t b = s2[j <= len2 ? j - 1 : 0] & 3u;
        prof[jj] = j > len2 ? 0x80808080u : b == 0 ? cols.c[0] : b == 1 ? cols.c[1] : b == 2 ? cols.c[2] : cols.c[3];
        key[jj] = kStored | (kCols - 1 - jj);           // row 0 holds 0
    }
    const int g_up = -(gap << 6) - (1 << 4);
    const int g_left = -(gap << 6) - (2 << 4);
    int diag_in = kStored;                              // key(0, jbase): H = 0
    int best = kStored, best_row = 0;                   // H = 0 at (0, 0)

    const int local_chunks = (len1 + 63 + kChunk - 1) / kChunk;
    const int total_chunks = local_chunks + kDelay * (W - 1);
    const int *ring_in = ring + (w > 0 ? w - 1 : 0) * kRing;   // read by waves 1.. (wave 0's left column is the border)
    int *ring_out = ring + (w < W - 1 ? w : 0) * kRing;        // written by waves ..W-2
    uint32_t *cw_out = TB ? codes + k * ((size_t)W * n_trips * 256) + ((size_t)w * n_trips * 64 + l) * 4 : nullptr;

    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) sh_next[t] = base_shift(s1, t - l, len1);

    for (int c = 0; c < total_chunks; ++c) {
        const int lc = c - kDelay * w;
        if (lc >= 0 && lc < local_chunks) {
            for (int q = 0; q < kChunk / kUnroll; ++q) {
                const int s0 = lc * kChunk + q * kUnroll;
                int sh[kUnroll], bound[kUnroll], edge[kUnroll];
                uint32_t cw[kUnroll];
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    sh[t] = sh_next[t];
                    sh_next[t] = base_shift(s1, s0 + kUnroll + t - l, len1);
                    // lane 0's left column for row s0 + t + 1: the ring, or the border's 0
                    bound[t] = w > 0 ? ring_in[(s0 + t) & (kRing - 1)] : kStored;
                    cw[t] = 0;
                }
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    const int left_in = __builtin_amdgcn_update_dpp(bound[t], key[kCols - 1], 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
                    const int row = s0 + t - l + 1;
                    if (row >= 1 && row <= len1) {
                        int d = diag_in, lft = left_in, rk = 0;
#pragma unroll
                        for (int jj = 0; jj < kCols; ++jj) {
                            const int sc = __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                            const int m3 = max3(d + (sc << 6), key[jj] + g_up, lft + g_left);
                            const int m = m3 > kFloor ? m3 : kFloor;
                            const int nk = (m & ~63) | (kStored | (kCols - 1 - jj));
                            if constexpr (TB) cw[t] |= ((uint32_t)(m >> 4) & 3u) << (2 * jj);
                            d = key[jj];
                            key[jj] = nk;
                            lft = nk;
                            rk = rk > nk ? rk : nk;
                        }
                        if (rk > (best | 63)) {
                            best = rk;
                            best_row = row;
                        }
                    }
                    edge[t] = key[kCols - 1];
                    diag_in = left_in;
                }
                if (w < W - 1 && l == 63) {
#pragma unroll
                    for (int t = 0; t < kUnroll; ++t) {
                        const int row = s0 + t - 62;
                        if (row >= 1 && row <= len1) ring_out[(row - 1) & (kRing - 1)] = edge[t];
                    }
                }
                if constexpr (TB)
                    *reinterpret_cast<uint4 *>(cw_out + (size_t)(s0 >> 2) * 256) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
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
        const uint32_t *cd = codes + k * ((size_t)W * n_trips * 256);
        unsigned long long *mv = moves + k * (size_t)move_words;
        int i = end_i, j = end_j, stopped = 0;
        uint32_t t = 0;
        unsigned long long acc = 0;
        while (!stopped && i > 0 && j > 0) {            // uniform: every thread holds the same (i, j, stopped)
            const int g1 = (j - 1) >> 4;
            const int i_lo = i - kStageRows + 1 > 1 ? i - kStageRows + 1 : 1;
            const int g_lo = g1 - kStageLanes + 1 > 0 ? g1 - kStageLanes + 1 : 0;
            const int rows = i - i_lo + 1, lanes = g1 - g_lo + 1;
            for (int e = tid; e < rows * lanes; e += blockDim.x) {
                const int rr = e / lanes, gg = e - rr * lanes;
                stage[rr * kStageLanes + gg] = __builtin_nontemporal_load(cd + code_index(i_lo + rr, g_lo + gg, n_trips));
            }
            __syncthreads();
            if (tid == 0) {
                int st = 0;
                while (i > 0 && j > 0 && i >= i_lo && ((j - 1) >> 4) >= g_lo) {
                    const uint32_t wd = stage[(i - i_lo) * kStageLanes + ((j - 1) >> 4) - g_lo];
                    const uint32_t cc = (wd >> (2 * ((j - 1) & 15))) & 3u;
                    if (cc == kStop) {                  // the cell holds 0: the start cell
                        st = 1;
                        break;
                    }
                    const uint32_t m = cc + 1;          // 3 / 2 / 1 = diagonal / up / left
                    acc |= (unsigned long long)m << (2 * (t & 31));
                    i -= m != 1u;
                    j -= m != 2u;
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

int local_full_waves(int len2) { return (len2 + 64 * kCols - 1) / (64 * kCols); }

size_t local_full_trips(int len1) { return (size_t)((len1 + 63 + kChunk - 1) / kChunk) * (kChunk / kUnroll); }

size_t local_full_code_words(int len1, int len2) { return (size_t)local_full_waves(len2) * local_full_trips(len1) * 256; }

hipError_t launch_local_full(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                             int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                             size_t move_words, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    SmCols cols;
    for (int b = 0; b < 4; ++b) {
        uint32_t c = 0;
        for (int a = 0; a < 4; ++a) c |= uint32_t(uint8_t(sm[4 * a + b])) << (8 * a);
        cols.c[b] = c;
    }
    const dim3 grid((unsigned)n), block(64 * local_full_waves(len2));
    const uint32_t trips = (uint32_t)local_full_trips(len1);
    if (d_moves)
        hipLaunchKernelGGL(local_full_kernel<true>, grid, block, 0, stream, d_seq1s, d_seq2s, len1, len2, cols, gap, d_scores, d_ends,
                           d_codes, d_moves, d_steps, (uint32_t)move_words, trips);
    else
        hipLaunchKernelGGL(local_full_kernel<false>, grid, block, 0, stream, d_seq1s, d_seq2s, len1, len2, cols, gap, d_scores, d_ends,
                           nullptr, nullptr, nullptr, 0u, trips);
    return hipGetLastError();
}

}  // namespace swmi
