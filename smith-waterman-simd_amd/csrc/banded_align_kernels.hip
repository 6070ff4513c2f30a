// banded_align_kernels.hip -- the kernels of libswmi_banded.so (include/swmi_banded.h): local alignment
// with affine gaps on the 128 diagonals -64 <= (j - i) - d0 <= 63 of a len1 x len2 table, with end cell, start cell and
// traceback or ends-only.
//
// MAPPING (section 9's, with the int32 cell).  One wavefront sweeps ONE alignment's anti-diagonals; lane m owns band diagonals
// 2m (its even cell) and 2m + 1 (its odd cell).  In iteration t lane m sits on row i = 1 - m + t; its even cell is column
// j = i + 2m - 64 + d0 and its odd cell column j + 1 (section 9's u is t - 32).  Neighbours:
//   even cell: diagonal = own even cell of t - 1, up = own odd cell of t - 1, left = lane m - 1's odd cell of t - 1
//   odd cell:  diagonal = own odd cell of t - 1,  left = own even cell of t,  up = lane m + 1's even cell of t
// Only rows that meet the band are swept: i_lo = max(1, -62 - d0) .. i_hi = min(len1, len2 + 64 - d0), that is iterations
// t0 = i_lo - 1 .. i_hi + 62 in whole trips of kBandTrip = 4.  A band that misses the table (i_lo > i_hi) writes its closed form
// and returns before any other load or store.  d0 is clamped to +-65536 first: beyond +-(16384 + 64) every band misses.
//
// SEQUENCES: no LDS stage.  Every lane loads its own row base (seq1[t - m]) and column base (seq2[t + m - 63 + d0], the odd
// cell's: the even cell's is last iteration's odd one) one trip ahead, four bytes of each per trip, from indices clamped into
// the sequence.  A wavefront's 64 bytes of one load are consecutive, so they cost one or two cache lines; the LDS a wavefront
// takes does not depend on the lengths (the traceback kernels hold the walk window there, the ends-only kernels nothing).
//
// CELLS OUTSIDE THE TABLE (row < 1 or > len1, column < 1 or > len2) are computed like any other and then replaced by what the
// contract gives them: H = 0, E = F = -infinity, that is the hand-over values of a cell holding H = 0, and code "stop".  They
// never reach the best (0 is never greater) and never a code that the walk reads.  Outside the BAND lie lane 0's left and
// lane 63's upper neighbour; the lane shift delivers nothing there and a select puts the same hand-over value in its place.
//
// GAPS are folded as in section 9, on signed int32 without saturation.  A cell hands ONE value down (me) and one to the right
// (mf); with fold = |open - extend| and cost = min(open, extend):
//   open >= extend:  a = H - fold, me = max(a, E), mf = max(a, F)            and the receiver takes  E' = me - extend
//   open <  extend:  a = H,        me = max(a, E - fold), mf = max(a, F - fold)   and                E' = me - open
// E' opened (came from H) iff a >= its partner: the tie goes to the opening.  That bit is known where the value is made, so it
// is stored in the code of the cell that HANDS OVER, and the walk reads it after its up or left move, in the cell it arrives
// at, which it has to read anyway.  A cell that hands over H = 0, E = F = -infinity hands over base = (open >= extend ? -fold : 0).
// Every value is at least -127 - 127 and at most 127 * 16384: int32 never wraps.
//
// CODES: 4 bits per cell: bits 0-1 H's source (0 stop, 3 diagonal, 2 E, 1 F, tested in that order), bit 2 "the E handed down
// opens", bit 3 "the F handed right opens".  A lane's two cells of an iteration are one byte, its four iterations of a trip one
// dword: dword (trip * 64 + lane) of the alignment's codes, a 256-byte store per wavefront and trip.
//
// BEST: within a lane rows grow with t and the even cell lies left of the odd one, so a strict > in arrival order keeps the
// lane's first cell in row-major order.  Across lanes the 64 (H, i, j) are reduced as a 64-bit key H : ~(i << 15 | j).
//
// WALK: all 64 lanes walk the same cell (wave-uniform; lane 0 stores).  The codes of kBandWalkTrips trips ending at the walk's
// trip are loaded into LDS by the whole wavefront; every move goes to iteration t or t - 1, so a window serves at least 64 steps.
#include "banded_internal.h"

#include <hip/hip_runtime.h>

namespace swmi {
namespace banded {
namespace {

constexpr int kWaves = 4;                   // wavefronts (alignments) per workgroup

struct Rows {
    uint32_t r[4];                          // r[a] = sm[4a .. 4a + 3], one byte per column base
};

// lane m - 1's / lane m + 1's v; 0 where there is no such lane (the callers select)
__device__ __forceinline__ int from_below(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true); }
__device__ __forceinline__ int from_above(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true); }

__device__ __forceinline__ int max_i(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

struct Cell {
    int h, me, mf;
};

// One cell from its diagonal H, the values handed to it and its substitution row / column one-hot.
template <bool kOge, bool kTb>
__device__ __forceinline__ Cell cell(int arow, int boh, int h_diag, int me_up, int mf_left, int cost, int fold, int base, bool valid,
                                     uint32_t &code)
{
    const int e = me_up - cost, f = mf_left - cost;
    const int d = __builtin_amdgcn_sdot4(arow, boh, h_diag, false);
    const int h = max_i(max_i(d, e), max_i(f, 0));
    const int a = kOge ? h - fold : h;
    const int eb = kOge ? e : e - fold, fb = kOge ? f : f - fold;
    if constexpr (kTb) {
        const uint32_t src = h == 0 ? 0u : h == d ? 3u : h == e ? 2u : 1u;
        const uint32_t c = src | (a >= eb ? 4u : 0u) | (a >= fb ? 8u : 0u);
        code = valid ? c : 12u;
    }
    Cell out;
    out.h = valid ? h : 0;
    out.me = valid ? max_i(a, eb) : base;
    out.mf = valid ? max_i(a, fb) : base;
    return out;
}

template <bool kOge, bool kTb>
__global__ void __launch_bounds__(64 * kWaves)
banded_local_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const int32_t *__restrict__ diagonals,
                    uint32_t n, int len1, int len2, Rows rows, int gap_open, int gap_extend, int32_t *__restrict__ scores,
                    int32_t *__restrict__ ends, uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves, uint32_t move_words,
                    uint32_t *__restrict__ steps)
{
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const uint32_t pair = blockIdx.x * kWaves + wv;
    if (pair >= n) return;                  // wave-uniform; only wave-level synchronisation below

    int d0 = diagonals ? diagonals[pair] : 0;
    d0 = clamp_i(d0, -65536, 65536);        // before any arithmetic: every int32 is legal
    d0 = __builtin_amdgcn_readfirstlane(d0);
    const int i_lo = max_i(1, -62 - d0), i_hi = len1 < len2 + 64 - d0 ? len1 : len2 + 64 - d0;
    if (i_lo > i_hi) {                      // the band misses the table
        if (lane == 0) {
            scores[pair] = 0;
            int32_t *e = ends + 4 * (size_t)pair;
            e[0] = e[1] = 0;
            e[2] = e[3] = kTb ? 0 : -1;
            if constexpr (kTb) steps[pair] = 0;
        }
        return;
    }
    const int t0 = i_lo - 1;
    const int n_trips = (i_hi - i_lo + 64 + kBandTrip - 1) / kBandTrip;

    const uint8_t *s1 = seq1s + (size_t)pair * (size_t)len1;
    const uint8_t *s2 = seq2s + (size_t)pair * (size_t)len2;
    uint32_t *cd = nullptr;
    if constexpr (kTb) cd = codes + (size_t)pair * (band_code_bytes((size_t)len1) / 4);

    const int cost = kOge ? gap_extend : gap_open;
    const int fold = kOge ? gap_open - gap_extend : gap_extend - gap_open;
    const int base = kOge ? -fold : 0;

    // row scores of a seq1 byte, one-hot of a seq2 byte
    auto row_of = [&](uint32_t a) {
        const uint32_t lo = (a & 1u) ? rows.r[1] : rows.r[0], hi = (a & 1u) ? rows.r[3] : rows.r[2];
        return (int)((a & 2u) ? hi : lo);
    };
    auto hot_of = [](uint32_t b) { return (int)(1u << (8u * (b & 3u))); };
    auto load1 = [&](int idx) { return (uint32_t)s1[clamp_i(idx, 0, len1 - 1)]; };
    auto load2 = [&](int idx) { return (uint32_t)s2[clamp_i(idx, 0, len2 - 1)]; };

    // 0-based: r = row index i - 1 of the lane at the trip's first iteration, ce = column index of its even cell there
    int r = t0 - lane, ce = t0 + lane - 64 + d0;
    int b_even = hot_of(load2(ce));
    uint32_t a_nxt[kBandTrip], b_nxt[kBandTrip];
#pragma unroll
    for (int k = 0; k < kBandTrip; ++k) {
        a_nxt[k] = load1(r + k);
        b_nxt[k] = load2(ce + 1 + k);
    }

    Cell c0{0, base, base}, c1{0, base, base};        // the lane's last even and odd cell
    int best = 0;
    uint32_t best_pos = 0;                             // i << 15 | j

#pragma unroll 1
    for (int trip = 0; trip < n_trips; ++trip) {
        int a_row[kBandTrip], b_hot[kBandTrip];
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            a_row[k] = row_of(a_nxt[k]);
            b_hot[k] = hot_of(b_nxt[k]);
        }
        // the next trip's bytes (clamped indices: behind the last trip they are loaded and not used)
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            a_nxt[k] = load1(r + kBandTrip + k);
            b_nxt[k] = load2(ce + 1 + kBandTrip + k);
        }
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            const bool row_ok = (uint32_t)(r + k) < (uint32_t)len1;
            const bool ok0 = row_ok && (uint32_t)(ce + k) < (uint32_t)len2;
            const bool ok1 = row_ok && (uint32_t)(ce + k + 1) < (uint32_t)len2;
            const uint32_t pos = ((uint32_t)(r + k + 1) << 15) + (uint32_t)(ce + k + 1);
            uint32_t code0 = 0, code1 = 0;
            // even cell: left = lane m - 1's odd cell of the last iteration.  The shift stands outside the select: under a
            // branch on the lane it would run with lane 0 switched off, and lane 1 would read 0 from it
            const int left_in = from_below(c1.mf);
            const int left = lane == 0 ? base : left_in;
            c0 = cell<kOge, kTb>(a_row[k], b_even, c0.h, c1.me, left, cost, fold, base, ok0, code0);
            if (c0.h > best) {
                best = c0.h;
                best_pos = pos;
            }
            // odd cell: up = lane m + 1's even cell of this iteration
            const int up_in = from_above(c0.me);
            const int up = lane == 63 ? base : up_in;
            c1 = cell<kOge, kTb>(a_row[k], b_hot[k], c1.h, up, c0.mf, cost, fold, base, ok1, code1);
            if (c1.h > best) {
                best = c1.h;
                best_pos = pos + 1;
            }
            b_even = b_hot[k];
            if constexpr (kTb) word |= (code0 | (code1 << 4)) << (8 * k);
        }
        if constexpr (kTb) cd[(size_t)trip * 64 + lane] = word;
        r += kBandTrip;
        ce += kBandTrip;
    }

    // the first cell in row-major order among the lanes' bests
    uint32_t key_hi = (uint32_t)best, key_lo = ~best_pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)key_hi, o), lo = (uint32_t)__shfl_xor((int)key_lo, o);
        const bool take = hi > key_hi || (hi == key_hi && lo > key_lo);
        key_hi = take ? hi : key_hi;
        key_lo = take ? lo : key_lo;
    }
    best = (int)key_hi;
    best_pos = ~key_lo;
    const int bi = (int)(best_pos >> 15), bj = (int)(best_pos & 32767u);
    int32_t *e_out = ends + 4 * (size_t)pair;
    if constexpr (!kTb) {
        if (lane == 0) {
            scores[pair] = best;
            e_out[0] = bi;
            e_out[1] = bj;
            e_out[2] = e_out[3] = -1;
        }
        return;
    } else {
        __shared__ uint32_t window[kWaves][kBandWalkTrips * 64];
        uint32_t *win = window[wv];
        const unsigned char *win8 = reinterpret_cast<const unsigned char *>(win);
        // this wave's code stores have reached L2, and the window's loads do not take them from the L1
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned long long *mv = moves + (size_t)pair * (size_t)move_words;
        int i = bi, j = bj, state = 0;      // state: 0 = H, 2 = in a vertical gap (E), 1 = in a horizontal gap (F)
        int w_lo = n_trips;                 // the window holds trips [w_lo, w_lo + kBandWalkTrips): nothing yet
        uint32_t t = 0;
        unsigned long long word = 0;
        while (i >= 1 && j >= 1) {          // a border cell holds 0: the walk stops there in state H
            const int dl = j - i - d0 + 64; // the band diagonal, 0 .. 127
            if ((uint32_t)dl > 127u) break;                     // (never: the walk cannot leave the band)
            const int ln = dl >> 1, rel = i - 1 + ln - t0;      // the lane and iteration that hold the cell
            if (rel < 0 || rel >= n_trips * kBandTrip) break;   // (never: every cell of the table in the band was swept)
            const int q = rel >> 2;
            if (q < w_lo || q >= w_lo + kBandWalkTrips) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();            // every lane is past its reads of the old window
                w_lo = max_i(q - (kBandWalkTrips - 1), 0);
                const int cnt = n_trips - w_lo < kBandWalkTrips ? n_trips - w_lo : kBandWalkTrips;
                for (int x = 0; x < cnt; ++x) win[x * 64 + lane] = __builtin_nontemporal_load(cd + (size_t)(w_lo + x) * 64 + lane);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            const uint32_t byte = win8[((q - w_lo) * 64 + ln) * 4 + (rel & 3)];
            const uint32_t c = (byte >> (4 * (dl & 1))) & 15u;
            // arrived in a gap: it ends here if the value this cell handed over opened it
            if (state == 2 && (c & 4u)) state = 0;
            if (state == 1 && (c & 8u)) state = 0;
            int dir = state;
            if (state == 0) {
                dir = (int)(c & 3u);
                if (dir == 0) break;        // H = 0: the start cell
            }
            word |= (unsigned long long)dir << (2 * (t & 31u));
            ++t;
            if ((t & 31u) == 0) {
                if (lane == 0) mv[(t >> 5) - 1] = word;
                word = 0;
            }
            if (dir == 3) {
                --i;
                --j;
                state = 0;
            } else if (dir == 2) {
                --i;
                state = 2;
            } else {
                --j;
                state = 1;
            }
        }
        if (lane == 0) {
            if (t & 31u) mv[t >> 5] = word;
            scores[pair] = best;
            e_out[0] = bi;
            e_out[1] = bj;
            e_out[2] = i;
            e_out[3] = j;
            steps[pair] = t;
        }
    }
}

}  // namespace

hipError_t launch_banded_local(const uint8_t *d_seq1s, int len1, const uint8_t *d_seq2s, int len2, const int32_t *d_diagonals, size_t n,
                               const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned char *d_codes,
                               unsigned long long *d_moves, size_t move_words, uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    Rows rows;
    for (int a = 0; a < 4; ++a) {
        rows.r[a] = 0;
        for (int b = 0; b < 4; ++b) rows.r[a] |= (uint32_t)(uint8_t)sm[4 * a + b] << (8 * b);
    }
    const dim3 grid((unsigned)((n + kWaves - 1) / kWaves)), block(64 * kWaves);
    const bool tb = d_moves != nullptr, oge = gap_open >= gap_extend;
    uint32_t *codes = reinterpret_cast<uint32_t *>(d_codes);
#define BANDED_LAUNCH(OGE, TB)                                                                                                       \
    hipLaunchKernelGGL((banded_local_kernel<OGE, TB>), grid, block, 0, stream, d_seq1s, d_seq2s, d_diagonals, (uint32_t)n, len1, len2, rows, \
                       gap_open, gap_extend, d_scores, d_ends, codes, d_moves, (uint32_t)move_words, d_steps)
    if (tb) {
        if (oge) BANDED_LAUNCH(true, true);
        else BANDED_LAUNCH(false, true);
    } else {
        if (oge) BANDED_LAUNCH(true, false);
        else BANDED_LAUNCH(false, false);
    }
#undef BANDED_LAUNCH
    return hipGetLastError();
}

}  // namespace banded
}  // namespace swmi
