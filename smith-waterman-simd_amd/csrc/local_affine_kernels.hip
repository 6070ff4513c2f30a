// local_affine_kernels.hip -- gfx950 kernels of the affine-gap local aligner with end cell, start cell and traceback
// (swmi_local_align_affine*).
//
// Semantics (include/swmi.h): Gotoh's recurrences, a gap of length k costing open + (k-1) extend,
//     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap (an up move)
//     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap (a left move)
//     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
// for i = 1..len1, j = 1..128, H = 0 and E = F = -inf on the boundary; the end cell is the first cell in row-major order
// that holds max H; the walk goes back from it in state H (floor, diagonal, E, F) and through E / F runs (opening wins a tie).
//
// Mapping: that of local_kernels.hip: 16 lanes per alignment (one DPP row), lane l owns columns
// 8l+1 .. 8l+8 and at step s computes row s - l + 1.  E runs down a column and stays in the lane's registers; F runs along
// the row, so a step passes lane l - 1's H(i, 8l) AND its F(i, 8l) to lane l: two v_mov_b32_dpp row_shr:1 per step.
//
// The cell as KEYS, as in local_kernels.hip: key = H << 17 | field << 15 | (0x7FFF - i), and every candidate of H's max is one
// add away from a neighbour's key, its 2-bit field the tie order: 3 = the zero floor, 2 = diagonal, 1 = E, 0 = F.
// E and F carry the open/extend tie the same way.  With a traceback they are kept as keys whose low 17 bits hold the field of
// H's max (1 for E, 0 for F: one v_and_or_b32 after their own max), so the extend candidate E - extend << 17 has bits 15-16 at
// most 1, while the open candidate H(i-1,j) key - open << 17 has field 2 there: on equal values opening wins, and bit 16 of the
// winner is the open bit.  Ends-only the low bits need no order (only H's value and the row of the best key matter), so E and F
// are not masked.  |H|, |E|, |F| + 127 < 2^14 past the boundary, which itself is -2^30 for E and F.
//
// Codes: 4 bits per cell, a lane's 8 cells in one dword per step -- bits 2c..2c+1 = H's field of column 8l+1+c, bit 16 + c =
// E's open bit, bit 24 + c = F's open bit -- so the 16 lanes of an alignment store the 64 contiguous bytes of one step with
// one instruction.  The cell (i, j) sits at step s = i + (j-1)/8 - 1, dword 16 s + (j-1)/8.  The walk (one lane per
// alignment, a state of H / E / F) reads them back in the same launch after an s_waitcnt vmcnt(0), with non-temporal loads.
#include "tile_sweep.h"   // imax, max3, SmCols, sm_cols

namespace swmi {
namespace {

constexpr int kLanes = 16;              // lanes per alignment: one DPP row
constexpr int kCols = 8;                // columns per lane
constexpr int kAlnPerWave = 64 / kLanes;
constexpr int kWavesPerBlock = 4;
constexpr int kAlnPerBlock = kAlnPerWave * kWavesPerBlock;
constexpr int kUnroll = 8;              // steps per loop trip (eight code dwords per lane)
constexpr int kBoundary = 2 << 15;      // key of a boundary cell: H = 0, field 2
constexpr int kFloor = 3 << 15;         // the zero floor: H = 0, field 3 (wins every tie at 0)
constexpr int kMinusInf = -(1 << 30);   // E on row 0, F on column 0
constexpr int kValue = (int)0xFFFE0000; // the value bits of a key

// the same register in lane l - 1 of the row; the first lane of a row gets `edge`
__device__ __forceinline__ int from_left(int edge, int v)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
}

// 8 * (seq1[idx] & 3), or 0 outside the sequence (clamped load: it issues a whole trip ahead of its use)
__device__ __forceinline__ int base_shift(const uint8_t *s1, int idx, int len1)
{
    const int c = idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx;
    const int b = s1[c];
    return (idx >= 0 && idx < len1) ? 8 * (b & 3) : 0;
}

// the same for a length that may be 0 (ragged launches): the load is clamped to s1[0] then, which is not seq1 (local_kernels.hip)
__device__ __forceinline__ int base_shift_any(const uint8_t *s1, int idx, int len1)
{
    const int c = idx >= len1 ? len1 - 1 : idx;
    const int b = s1[c < 0 ? 0 : c];
    return (idx >= 0 && idx < len1) ? 8 * (b & 3) : 0;
}

// RAGGED: slot k computes the alignment work[k] names, as in local_kernels.hip
template <bool TB, bool RAGGED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void sw_local_affine_kernel(
    const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, int len1, uint32_t n, SmCols cols, int gap_open,
    int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends, uint32_t *__restrict__ codes,
    unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps, uint32_t move_words, uint32_t code_words,
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
    const uint2 b8 = *reinterpret_cast<const uint2 *>(seq2s + (size_t)k * 128 + kCols * l);
    uint32_t prof[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const uint32_t b = ((jj < 4 ? b8.x : b8.y) >> (8 * (jj & 3))) & 3u;
        prof[jj] = b == 0 ? cols.c[0] : b == 1 ? cols.c[1] : b == 2 ? cols.c[2] : cols.c[3];
    }
    // open candidates come from H keys (field 2); extend candidates from masked E (field 1) / F (field 0) keys with a
    // traceback, which these constants bring back to field 0
    const int g_open = -(gap_open << 17);
    const int g_ext_e = -(gap_extend << 17) - (TB ? 1 << 15 : 0);
    const int g_ext_f = -(gap_extend << 17);

    int key[kCols], e[kCols], best[kCols];
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        key[jj] = kBoundary;                            // row 0
        e[jj] = kMinusInf;
        best[jj] = 0;
    }
    int diag_in = kBoundary;                            // key(i-1, 8l) of the lane's current row i
    int f_last = kMinusInf;                             // F(i, 8l + 8) of the lane's last row, for lane l + 1
    uint32_t *cw_out = TB ? codes + (RAGGED ? code_base : (size_t)k * code_words) + l : nullptr;

    const int n_steps = len1 + kLanes - 1;
    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) sh_next[t] = RAGGED ? base_shift_any(s1, t - l, len1) : base_shift(s1, t - l, len1);
    for (int s0 = 0; s0 < n_steps; s0 += kUnroll) {
        int sh[kUnroll];
#pragma unroll
        for (int t = 0; t < kUnroll; ++t) {
            sh[t] = sh_next[t];
            sh_next[t] = RAGGED ? base_shift_any(s1, s0 + kUnroll + t - l, len1) : base_shift(s1, s0 + kUnroll + t - l, len1);
        }
        uint32_t cw[kUnroll];
#pragma unroll
        for (int t = 0; t < kUnroll; ++t) {
            cw[t] = 0;
            const int left_in = from_left(kBoundary, key[kCols - 1]);   // lane l-1's key(i, 8l), computed one step ago
            const int f_in = from_left(kMinusInf, f_last);              // ... and its F(i, 8l)
            const int row = s0 + t - l + 1;
            if (row >= 1 && row <= len1) {
                const int ci = (2 << 15) + 0x7FFF - row;
                int d = diag_in, lft = left_in, f = f_in;
#pragma unroll
                for (int jj = 0; jj < kCols; ++jj) {
                    const int sc = __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                    const int diag = d + (sc << 17);
                    const int ev = imax(key[jj] + g_open, e[jj] + g_ext_e);
                    const int fv = imax(lft + g_open, f + g_ext_f);
                    int ec = ev, fc = fv;
                    if constexpr (TB) {
                        ec = (ev & kValue) | (1 << 15);
                        fc = fv & kValue;
                    }
                    const int m = imax(max3(diag, ec, fc), kFloor);
                    const int nk = (m & kValue) | ci;
                    if constexpr (TB) {
                        cw[t] |= (((uint32_t)m >> 15) & 3u) << (2 * jj);
                        cw[t] |= (((uint32_t)ev >> 16) & 1u) << (16 + jj);
                        cw[t] |= (((uint32_t)fv >> 16) & 1u) << (24 + jj);
                    }
                    best[jj] = imax(best[jj], nk);
                    d = key[jj];
                    key[jj] = nk;
                    e[jj] = ec;
                    f = fc;
                    lft = nk;
                }
                f_last = f;
            }
            diag_in = left_in;
        }
        if constexpr (TB) {
#pragma unroll
            for (int t = 0; t < kUnroll; ++t) cw_out[(size_t)(s0 + t) * kLanes] = cw[t];
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
        // the 16 lanes' code stores reach L2 before the walk's non-temporal loads read them (local_kernels.hip)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t *cd = codes + (RAGGED ? code_base : (size_t)k * code_words);
        unsigned long long *mv = moves + (RAGGED ? move_base : (size_t)k * move_words);
        int i = end_i, j = end_j;
        int state = 0;                                  // 0 = H, 1 = E, 2 = F
        uint32_t t = 0;
        unsigned long long acc = 0;
        while (i > 0 && j > 0) {
            const int ln = (j - 1) >> 3, c = (j - 1) & 7;
            const uint32_t w = __builtin_nontemporal_load(cd + (size_t)(i + ln - 1) * kLanes + ln);
            unsigned mvc;
            if (state == 0) {
                const uint32_t h = (w >> (2 * c)) & 3u;
                if (h == 3u) break;                      // H(i,j) == 0: the start cell
                state = h == 2u ? 0 : h == 1u ? 1 : 2;
            }
            if (state == 0) {
                mvc = 3;                                 // diagonal
                --i;
                --j;
            } else if (state == 1) {
                mvc = 2;                                 // up, inside E; back to H where E opened
                state = (w >> (16 + c)) & 1u ? 0 : 1;
                --i;
            } else {
                mvc = 1;                                 // left, inside F
                state = (w >> (24 + c)) & 1u ? 0 : 2;
                --j;
            }
            acc |= (unsigned long long)mvc << (2 * (t & 31));
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

size_t local_affine_code_words(int len1)
{
    const int n_steps = len1 + kLanes - 1;
    const int trips = (n_steps + kUnroll - 1) / kUnroll;
    return (size_t)trips * kUnroll * kLanes;
}

hipError_t launch_local_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, size_t n, const int8_t *sm, int gap_open,
                               int gap_extend, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                               uint32_t *d_steps, size_t move_words, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)((n + kAlnPerBlock - 1) / kAlnPerBlock)), block(64 * kWavesPerBlock);
    const uint32_t cw = (uint32_t)local_affine_code_words(len1);
    if (d_moves)
        hipLaunchKernelGGL((sw_local_affine_kernel<true, false>), grid, block, 0, stream, d_seq1s, d_seq2s, len1, (uint32_t)n, cols,
                           gap_open, gap_extend, d_scores, d_ends, d_codes, d_moves, d_steps, (uint32_t)move_words, cw, nullptr);
    else
        hipLaunchKernelGGL((sw_local_affine_kernel<false, false>), grid, block, 0, stream, d_seq1s, d_seq2s, len1, (uint32_t)n, cols,
                           gap_open, gap_extend, d_scores, d_ends, nullptr, nullptr, nullptr, 0u, cw, nullptr);
    return hipGetLastError();
}

hipError_t launch_local_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const LocalWork *d_work, size_t n,
                                      const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends,
                                      uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)((n + kAlnPerBlock - 1) / kAlnPerBlock)), block(64 * kWavesPerBlock);
    if (d_moves)
        hipLaunchKernelGGL((sw_local_affine_kernel<true, true>), grid, block, 0, stream, d_seq1s, d_seq2s, 0, (uint32_t)n, cols, gap_open,
                           gap_extend, d_scores, d_ends, d_codes, d_moves, d_steps, 0u, 0u, d_work);
    else
        hipLaunchKernelGGL((sw_local_affine_kernel<false, true>), grid, block, 0, stream, d_seq1s, d_seq2s, 0, (uint32_t)n, cols,
                           gap_open, gap_extend, d_scores, d_ends, nullptr, nullptr, nullptr, 0u, 0u, d_work);
    return hipGetLastError();
}

}  // namespace swmi
