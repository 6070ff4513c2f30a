// local_kernels.hip -- gfx950 kernels of the local aligner with end cell, start cell and traceback (swmi_local_align*).
//
// Semantics: the reference's SmithWaterman_111_long (source.cpp:1526-1576) generalised to any int8 matrix and gap:
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)
// for i = 1..len1 (seq1, any length up to 16384) and j = 1..128 (seq2); score = max H; the end cell is the first cell in
// row-major order that holds it ((0,0) for score 0); the walk goes back from it, diagonal before up before left, until a
// cell holds 0 (the start cell).  DESIGN.md section 12.
//
// Mapping: L = 16 lanes per alignment (one DPP row), 4 alignments per wavefront.  Lane l owns the 8 columns 8l+1 .. 8l+8
// and at step s computes the 8 cells of row i = s - l + 1, left to right; the value of column 8l that it needs comes from
// lane l - 1, which computed row i one step earlier (one v_mov_b32_dpp row_shr:1 per step).  A row therefore leaves the
// pipeline 15 steps after it entered: len1 + 15 steps in all, whatever len1 is.
//
// The cell as KEYS.  Every cell value is held as one int32
//     key = H << 17 | 2 << 15 | (0x7FFF - i)
// and every candidate of the max is formed from the keys of the three neighbours by ONE add:
//     diag = key(i-1,j-1) + s << 17        (field at bits 15-16 stays 2)
//     up   = key(i-1,j)   - gap << 17 - 1 << 15   (field 1)
//     left = key(i,j-1)   - gap << 17 - 2 << 15   (field 0)
//     zero = 3 << 15                        (field 3, H = 0)
// so one max3 + one max picks the largest value AND, among equal values, the reference's order: the zero floor first, then
// diagonal, up, left (source.cpp:1541-1543, :1555-1568).  The field of the winner is the cell's 2-bit predecessor code
// (3 = stop, 2 = diagonal, 1 = up, 0 = left; the walk turns it into the moves encoding 0/3/2/1), and one v_and_or_b32 turns
// the winner back into a key.  The low 15 bits never carry into the field (row < 2^15) and never decide between two
// candidates (their fields differ).  The running best is a v_max_i32 of keys per column: the largest H, and on a tie the
// smallest row; the columns are reduced (value desc, row asc, column asc) at the end -- the row-major-first rule of
// source.cpp:1545.  |H + s| < 2^14 (the score is at most 127 * 128, every diagonal step uses up a column), so nothing
// overflows.
//
// Codes: 2 bits per cell, 16 bits per lane and step; two steps make one dword, and the 16 lanes of an alignment store the
// 64 contiguous bytes of a step pair with one instruction.  The cell (i, j) sits at step s = i + (j-1)/8 - 1: dword
// (s/2)*16 + (j-1)/8, bits 16 (s%2) + 2 ((j-1)%8).  The walk (one lane per alignment) reads them back in the same launch:
// the sweep's stores are drained by an explicit s_waitcnt vmcnt(0) and the walk's loads are non-temporal, which bypass the
// CU's L1 and read the XCD's L2, where the stores landed.
#include "tile_sweep.h"   // imax, max3, SmCols, sm_cols

namespace swmi {
namespace {

constexpr int kLanes = 16;              // lanes per alignment: one DPP row
constexpr int kCols = 8;                // columns per lane
constexpr int kAlnPerWave = 64 / kLanes;
constexpr int kWavesPerBlock = 4;
constexpr int kAlnPerBlock = kAlnPerWave * kWavesPerBlock;
constexpr int kUnroll = 8;              // steps per loop trip (four step pairs of codes)
constexpr int kBoundary = 2 << 15;      // key of a boundary cell: H = 0, field 2
constexpr int kFloor = 3 << 15;         // the zero floor: H = 0, field 3 (wins every tie at 0)

// key of the same register in lane l - 1 of the row; the first lane of a row gets the boundary column's key
__device__ __forceinline__ int from_left(int v)
{
    return __builtin_amdgcn_update_dpp(kBoundary, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
}

// 8 * (seq1[idx] & 3), or 0 outside the sequence.  The load itself is clamped into the sequence instead of predicated, so
// that it issues a whole trip ahead of its use (a predicated load is waited for on the spot).
__device__ __forceinline__ int base_shift(const uint8_t *s1, int idx, int len1)
{
    const int c = idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx;
    const int b = s1[c];
    return (idx >= 0 && idx < len1) ? 8 * (b & 3) : 0;
}

// base_shift for a length that may be 0 (ragged launches): the load is clamped to s1[0] then, which the caller points at a
// readable byte that is not seq1
__device__ __forceinline__ int base_shift_any(const uint8_t *s1, int idx, int len1)
{
    const int c = idx >= len1 ? len1 - 1 : idx;
    const int b = s1[c < 0 ? 0 : c];
    return (idx >= 0 && idx < len1) ? 8 * (b & 3) : 0;
}

// RAGGED: slot k of the launch computes the alignment work[k] names (its own length, seq1, codes and moves, results at
// work[k].k); otherwise alignment k of len1 bytes at seq1s + len1 k, codes and moves at k code_words / k move_words.
template <bool TB, bool RAGGED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sw_local_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s,
                                                                       int len1, uint32_t n, SmCols cols, int gap, int32_t *__restrict__ scores,
                                                                       int32_t *__restrict__ ends, uint32_t *__restrict__ codes,
                                                                       unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps,
                                                                       uint32_t move_words, uint32_t code_words,
                                                                       const LocalWork *__restrict__ work)
{
    const int lane = threadIdx.x & 63;
    const int l = lane & (kLanes - 1);
    uint32_t k = blockIdx.x * kAlnPerBlock + (threadIdx.x >> 6) * kAlnPerWave + (lane >> 4);
    if (k >= n) return;                                 // uniform over the 16 lanes of an alignment

    const uint8_t *s1;
    uint32_t code_base = 0, move_base = 0;             // RAGGED only (the fixed layout computes its offsets where it uses them)
    if constexpr (RAGGED) {
        const LocalWork w = work[k];
        k = w.k;
        len1 = (int)w.len1;
        s1 = len1 ? seq1s + w.s1_off : seq2s + (size_t)k * 128;     // length 0: the clamped loads read the seq2, never seq1
        code_base = w.code_base;
        move_base = w.move_base;
    } else {
        s1 = seq1s + (size_t)k * (size_t)len1;
    }
    // the lane's 8 columns of seq2 (8-byte aligned: seq2 k starts at 128 k) -> 8 query-profile dwords
    const uint2 b8 = *reinterpret_cast<const uint2 *>(seq2s + (size_t)k * 128 + kCols * l);
    uint32_t prof[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const uint32_t b = ((jj < 4 ? b8.x : b8.y) >> (8 * (jj & 3))) & 3u;
        prof[jj] = b == 0 ? cols.c[0] : b == 1 ? cols.c[1] : b == 2 ? cols.c[2] : cols.c[3];
    }
    const int g_up = -(gap << 17) - (1 << 15);
    const int g_left = -(gap << 17) - (2 << 15);

    int key[kCols], best[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        key[jj] = kBoundary;                            // row 0
        best[jj] = 0;
    }
    int diag_in = kBoundary;                            // key(i-1, 8l) of the lane's current row i
    uint32_t *cw_out = TB ? codes + (RAGGED ? code_base : (size_t)k * code_words) + l : nullptr;

    const int n_steps = len1 + kLanes - 1;
    // seq1 bases of the lane's rows for the next trip, as bit offsets 8 * base into a profile dword (0 past either end)
    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) {
        sh_next[t] = RAGGED ? base_shift_any(s1, t - l, len1) : base_shift(s1, t - l, len1);   // row t - l + 1 at step t
    }
    for (int s0 = 0; s0 < n_steps; s0 += kUnroll) {
        int sh[kUnroll];
#pragma unroll
        for (int t = 0; t < kUnroll; ++t) {
            sh[t] = sh_next[t];
            sh_next[t] = RAGGED ? base_shift_any(s1, s0 + kUnroll + t - l, len1) : base_shift(s1, s0 + kUnroll + t - l, len1);
        }
        uint32_t cw[kUnroll / 2] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < kUnroll; ++t) {
            const int left_in = from_left(key[kCols - 1]);      // lane l-1's key(i, 8l), computed one step ago
            const int row = s0 + t - l + 1;
            if (row >= 1 && row <= len1) {
                const int ci = (2 << 15) + 0x7FFF - row;
                int d = diag_in, lft = left_in;
#pragma unroll
                for (int jj = 0; jj < kCols; ++jj) {
                    const int sc = __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                    const int diag = d + (sc << 17);
                    const int up = key[jj] + g_up;
                    const int left = lft + g_left;
                    const int du = max3(diag, up, kFloor);
                    const int m = du > left ? du : left;
                    const int nk = (m & (int)0xFFFE0000) | ci;
                    if constexpr (TB) cw[t >> 1] |= ((uint32_t)(m >> 15) & 3u) << (16 * (t & 1) + 2 * jj);
                    best[jj] = best[jj] > nk ? best[jj] : nk;
                    d = key[jj];
                    key[jj] = nk;
                    lft = nk;
                }
            }
            diag_in = left_in;
        }
        if constexpr (TB) {
#pragma unroll
            for (int p = 0; p < kUnroll / 2; ++p) cw_out[(size_t)((s0 >> 1) + p) * kLanes] = cw[p];
        }
    }

    // end cell: per lane the first column holding the lane's best key, then over the 16 lanes (value desc, row asc, col asc)
    int bk = best[0], bj = 0;
#pragma unroll
    for (int jj = 1; jj < kCols; ++jj)
        if (best[jj] > bk) {
            bk = best[jj];
            bj = jj;
        }
    unsigned long long r = ((unsigned long long)(uint32_t)bk << 8) | (unsigned long long)(255 - (kCols * l + bj));
#pragma unroll
    for (int o = 1; o < kLanes; o <<= 1) {
        const unsigned long long v = __shfl_xor(r, o, kLanes);
        r = v > r ? v : r;
    }
    const int key_best = (int)(uint32_t)(r >> 8);
    const int score = key_best >> 17;
    const int end_i = score ? 0x7FFF - (key_best & 0x7FFF) : 0;
    const int end_j = score ? 255 - (int)(r & 255) + 1 : 0;

    if (l != 0) return;
    scores[k] = score;
    ends[4 * (size_t)k + 0] = end_i;
    ends[4 * (size_t)k + 1] = end_j;
    if constexpr (!TB) {
        ends[4 * (size_t)k + 2] = -1;
        ends[4 * (size_t)k + 3] = -1;
    } else {
        // The 16 lanes' code stores must have reached L2 before the walk reads them back with non-temporal loads (which
        // skip the CU's L1).  On gfx950 vmcnt also counts stores, decremented when L2 has acknowledged the write, so one
        // s_waitcnt vmcnt(0) is that guarantee (a workgroup-scope fence lowers to nothing here); the "memory" clobber keeps
        // the compiler from moving a walk load above it.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t *cd = codes + (RAGGED ? code_base : (size_t)k * code_words);
        unsigned long long *mv = moves + (RAGGED ? move_base : (size_t)k * move_words);
        int i = end_i, j = end_j;
        uint32_t t = 0;
        unsigned long long acc = 0;
        while (i > 0 && j > 0) {
            const int ln = (j - 1) >> 3;
            const int s = i + ln - 1;
            const uint32_t w = __builtin_nontemporal_load(cd + (size_t)(s >> 1) * kLanes + ln);
            const uint32_t c = (w >> (16 * (s & 1) + 2 * ((j - 1) & 7))) & 3u;
            if (c == 3u) break;                          // H(i,j) == 0: the start cell
            acc |= (unsigned long long)(c + 1) << (2 * (t & 31));   // 2/1/0 -> 3/2/1 = diagonal/up/left
            i -= c != 0u;
            j -= c != 1u;
            ++t;
            if ((t & 31) == 0) {
                mv[(t >> 5) - 1] = acc;
                acc = 0;
            }
        }
        if (t & 31) mv[t >> 5] = acc;
        steps[k] = t;
        ends[4 * (size_t)k + 2] = i;
        ends[4 * (size_t)k + 3] = j;
    }
}

}  // namespace

size_t local_code_words(int len1)
{
    const int n_steps = len1 + kLanes - 1;
    const int trips = (n_steps + kUnroll - 1) / kUnroll;
    return (size_t)trips * (kUnroll / 2) * kLanes;
}

hipError_t launch_local(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, size_t n, const int8_t *sm, int gap,
                        int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                        size_t move_words, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)((n + kAlnPerBlock - 1) / kAlnPerBlock)), block(64 * kWavesPerBlock);
    const uint32_t cw = (uint32_t)local_code_words(len1);
    if (d_moves)
        hipLaunchKernelGGL((sw_local_kernel<true, false>), grid, block, 0, stream, d_seq1s, d_seq2s, len1, (uint32_t)n, cols, gap,
                           d_scores, d_ends, d_codes, d_moves, d_steps, (uint32_t)move_words, cw, nullptr);
    else
        hipLaunchKernelGGL((sw_local_kernel<false, false>), grid, block, 0, stream, d_seq1s, d_seq2s, len1, (uint32_t)n, cols, gap,
                           d_scores, d_ends, nullptr, nullptr, nullptr, 0u, cw, nullptr);
    return hipGetLastError();
}

hipError_t launch_local_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const LocalWork *d_work, size_t n, const int8_t *sm,
                               int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                               uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)((n + kAlnPerBlock - 1) / kAlnPerBlock)), block(64 * kWavesPerBlock);
    if (d_moves)
        hipLaunchKernelGGL((sw_local_kernel<true, true>), grid, block, 0, stream, d_seq1s, d_seq2s, 0, (uint32_t)n, cols, gap, d_scores,
                           d_ends, d_codes, d_moves, d_steps, 0u, 0u, d_work);
    else
        hipLaunchKernelGGL((sw_local_kernel<false, true>), grid, block, 0, stream, d_seq1s, d_seq2s, 0, (uint32_t)n, cols, gap, d_scores,
                           d_ends, nullptr, nullptr, nullptr, 0u, 0u, d_work);
    return hipGetLastError();
}

}  // namespace swmi
