// banded_align_kernels.hip -- the kernels of libswmi_banded.so (include/swmi_banded.h): local alignment
// with affine gaps on the 128 diagonals -64 <= (j - i) - d0 <= 63 of a len1 x len2 table, with end cell, start cell and
// traceback or ends-only.
//
// The lane mapping, the loads, the gap folding, the codes and the walk window are banded_sweep.h's.  What is this file's:
//
// ROWS AND ITERATIONS.  In iteration t lane m sits on row i = 1 - m + t; its even cell is column j = i + 2m - 64 + d0 and its
// odd cell column j + 1 (section 9's u is t - 32).  Only rows that meet the band are swept: i_lo = max(1, -62 - d0) ..
// i_hi = min(len1, len2 + 64 - d0), that is iterations t0 = i_lo - 1 .. i_hi + 62 in whole trips of kBandTrip = 4.  A lane loads
// its row base seq1[t - m] and its column base seq2[t + m - 63 + d0].  A band that misses the table (i_lo > i_hi) writes its
// closed form and returns before any other load or store.  d0 is clamped to +-65536 first: beyond +-(16384 + 64) every band
// misses.
//
// THE FLOOR AND CELLS OUTSIDE THE TABLE (row < 1 or > len1, column < 1 or > len2).  H has a floor at 0.  A cell outside the
// table is computed like any other and then replaced by what the contract gives it: H = 0, E = F = -infinity, that is the
// hand-over values of a cell holding H = 0, base = (open >= extend ? -fold : 0), and code "stop".  They never reach the best (0
// is never greater) and never a code that the walk reads.  Lane 0's left and lane 63's upper neighbour take base as well.
// Every value is at least -127 - 127 and at most 127 * 16384: int32 never wraps.
//
// BEST: within a lane rows grow with t and the even cell lies left of the odd one, so a strict > in arrival order keeps the
// lane's first cell in row-major order.  Across lanes the 64 (H, i, j) are reduced as a 64-bit key H : ~(i << 15 | j).
//
// WALK: it stops in state H at a cell whose source is "stop" (H = 0: the start cell); a border cell holds 0.
#include "banded_sweep.h"

namespace swmi {
namespace banded {
namespace {

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
            c0 = cell<true, kOge, kTb>(a_row[k], b_even, c0.h, c1.me, left, cost, fold, ok0, 0, code0);
            if (c0.h > best) {
                best = c0.h;
                best_pos = pos;
            }
            // odd cell: up = lane m + 1's even cell of this iteration
            const int up_in = from_above(c0.me);
            const int up = lane == 63 ? base : up_in;
            c1 = cell<true, kOge, kTb>(a_row[k], b_hot[k], c1.h, up, c0.mf, cost, fold, ok1, 0, code1);
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
    const Rows rows = pack_rows(sm);
    uint32_t *codes = reinterpret_cast<uint32_t *>(d_codes);
    return launch_variant(gap_open >= gap_extend, d_moves != nullptr, n, [&](auto oge, auto tb, dim3 grid, dim3 block) {
        hipLaunchKernelGGL((banded_local_kernel<decltype(oge)::value, decltype(tb)::value>), grid, block, 0, stream, d_seq1s, d_seq2s,
                           d_diagonals, (uint32_t)n, len1, len2, rows, gap_open, gap_extend, d_scores, d_ends, codes, d_moves,
                           (uint32_t)move_words, d_steps);
    });
}

}  // namespace banded
}  // namespace swmi
