// banded_ragged_kernels.hip -- the kernels of libswmi_banded_ragged.so (include/swmi_banded_ragged.h):
// the banded local aligner (banded_align_kernels.hip, section 33) and the banded global / fit / overlap / extension aligner
// (banded_global_kernels.hip, section 34) on a batch of mixed (len1, len2): a wavefront takes its shape from a SLOT, not from
// the launch.
//
// The lane mapping, the loads, the gap folding, the codes and the walk window are banded_sweep.h's, and the two sweeps, bests
// and walks are those of the two fixed files, line for line: one wavefront per alignment, four per workgroup, lane m on band
// diagonals 2m and 2m + 1, byte loads one trip ahead, 256 contiguous code bytes per wavefront and trip, a walk window of 64
// iterations in LDS.  They are new text in a new file because moving even the prefetch of the fixed kernels into a shared
// function reschedules their whole sweep (section 35).  What is this file's:
//
// THE SLOT.  The wave index is made wave-uniform first (readfirstlane), so the slot's address is uniform and its 48 bytes are
// read once into SGPRs: the two sequence offsets, the two lengths, the diagonal (clamped to +-65536 by the host, and again here
// before any arithmetic), the offsets of the alignment's codes and moves, and the index its results go to.  Everything that
// was wave-uniform in the fixed kernels -- lengths, diagonal, i_lo, i_hi, the trip count -- still is.
//
// EMPTY SEQUENCES.  The fixed kernels clamp load indices into [0, len - 1], which names byte -1 or 0 of a sequence that has
// none.  The local kernel takes its closed form (that of a band that misses the table: the table has no interior cell) before
// any load.  The global kernel sweeps the one border the table consists of, so that border values, candidates and the forced
// steps stay the one code path; its loads of an empty sequence are turned to byte 0 of the wavefront's own slot (the upper
// clamp is max(len - 1, 0)): every cell they feed is a border cell or off the table and is replaced by its fixed value.
//
// THE TRAPS of sections 33 and 34 apply unchanged: the lane shifts run unconditionally with a select behind them, -2^29 is a
// value, and the two "never" bounds checks of the walk stay.
#include "banded_sweep.h"

namespace swmi {
namespace banded {
namespace {

constexpr int kNeg = -(1 << 29);            // minus infinity (global kind)
constexpr int kInfeasible = -(1 << 28);     // every finite value is above, every value made from kNeg below
constexpr unsigned kBegin1 = 1u, kBegin2 = 2u, kEnd1 = 4u, kEnd2 = 8u, kAnywhere = 16u;
constexpr int kNoAlignment = -2147483647 - 1;

// REGISTERS.  With the slot in SGPRs the sequence, code and move pointers are scalar too, and left to itself the scheduler
// then hoists the unrolled trip's lane masks until the global traceback kernels spill SGPRs (100 VGPRs, 16 SGPR spills).  Asking
// for six wavefronts per SIMD -- what the fixed traceback kernels reach unasked, at 72 and 79 VGPRs -- brings all eight kernels
// to the fixed kernels' registers with no spill (the table in DESIGN.md section 37).
constexpr int kRaggedWavesPerSimd = 6;

struct Shape {
    const uint8_t *s1, *s2;
    uint32_t *cd;
    unsigned long long *mv;
    int len1, len2, d0;
    uint32_t index;
};

// the wavefront's slot, wave-uniform
__device__ __forceinline__ Shape shape_of(const RaggedSlot *__restrict__ slots, uint32_t at, const uint8_t *seq1s, const uint8_t *seq2s,
                                          uint32_t *codes, unsigned long long *moves)
{
    const RaggedSlot s = slots[at];
    Shape out;
    out.s1 = seq1s + s.off1;
    out.s2 = seq2s + s.off2;
    out.cd = codes + s.code_off;
    out.mv = moves + s.move_off;
    out.len1 = __builtin_amdgcn_readfirstlane(s.len1);
    out.len2 = __builtin_amdgcn_readfirstlane(s.len2);
    out.d0 = __builtin_amdgcn_readfirstlane(clamp_i(s.d0, -kRaggedDiagClamp, kRaggedDiagClamp));   // before any arithmetic
    out.index = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.index);
    return out;
}

template <bool kOge, bool kTb>
__global__ void __launch_bounds__(64 * kWaves, kRaggedWavesPerSimd)
banded_ragged_local_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const RaggedSlot *__restrict__ slots,
                           uint32_t n, Rows rows, int gap_open, int gap_extend, int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                           uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t at = blockIdx.x * kWaves + (uint32_t)wv;
    if (at >= n) return;                    // wave-uniform; only wave-level synchronisation below

    const Shape sh = shape_of(slots, at, seq1s, seq2s, codes, moves);
    const int len1 = sh.len1, len2 = sh.len2, d0 = sh.d0;
    const uint32_t pair = sh.index;
    const int i_lo = max_i(1, -62 - d0), i_hi = len1 < len2 + 64 - d0 ? len1 : len2 + 64 - d0;
    if (len1 == 0 || len2 == 0 || i_lo > i_hi) {       // no interior cell in the band: before any load
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

    const uint8_t *s1 = sh.s1;
    const uint8_t *s2 = sh.s2;
    uint32_t *cd = nullptr;
    if constexpr (kTb) cd = sh.cd;

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
        unsigned long long *mv = sh.mv;
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

template <bool kOge, bool kTb>
__global__ void __launch_bounds__(64 * kWaves, kRaggedWavesPerSimd)
banded_ragged_global_kernel(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const RaggedSlot *__restrict__ slots,
                            uint32_t n, Rows rows, int gap_open, int gap_extend, uint32_t free_ends, int32_t *__restrict__ scores,
                            int32_t *__restrict__ ends, uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves,
                            uint32_t *__restrict__ steps)
{
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t at = blockIdx.x * kWaves + (uint32_t)wv;
    if (at >= n) return;                    // wave-uniform; only wave-level synchronisation below

    const Shape sh = shape_of(slots, at, seq1s, seq2s, codes, moves);
    const int len1 = sh.len1, len2 = sh.len2, d0 = sh.d0;
    const uint32_t pair = sh.index;
    const bool begin1 = free_ends & kBegin1, begin2 = free_ends & kBegin2, end1 = free_ends & kEnd1, end2 = free_ends & kEnd2;
    const bool anywhere = free_ends & kAnywhere;
    int32_t *e_out = ends + 4 * (size_t)pair;
    auto no_alignment = [&]() {
        if (lane == 0) {
            scores[pair] = kNoAlignment;
            e_out[0] = e_out[1] = 0;
            e_out[2] = e_out[3] = kTb ? 0 : -1;
            if constexpr (kTb) steps[pair] = 0;
        }
    };
    const int i_lo = max_i(0, -63 - d0), i_hi = min_i(len1, len2 + 64 - d0);
    {
        // the candidates in the band: the corner; column len2's rows with END1; row len1's columns with END2; any cell
        const int dc = len2 - len1 - d0;
        const bool corner = dc >= -64 && dc <= 63;
        const bool col = end1 && max_i(0, len2 - d0 - 63) <= min_i(len1, len2 - d0 + 64);
        const bool row = end2 && max_i(0, len1 + d0 - 64) <= min_i(len2, len1 + d0 + 63);
        if (i_lo > i_hi || !(corner || col || row || anywhere)) {
            no_alignment();
            return;
        }
    }
    const int n_trips = (i_hi - i_lo + 64 + kBandTrip - 1) / kBandTrip;

    // an empty sequence has no byte: its loads go to byte 0 of this wavefront's slot, and feed only cells that are replaced
    const uint8_t *own = reinterpret_cast<const uint8_t *>(slots + at);
    const uint8_t *s1 = len1 ? sh.s1 : own;
    const uint8_t *s2 = len2 ? sh.s2 : own;
    const int top1 = max_i(len1 - 1, 0), top2 = max_i(len2 - 1, 0);
    uint32_t *cd = nullptr;
    if constexpr (kTb) cd = sh.cd;

    const int cost = kOge ? gap_extend : gap_open;
    const int fold = kOge ? gap_open - gap_extend : gap_extend - gap_open;
    // the borders' closed forms: H(0, j) = row0_at - (j - 1) row0_step, H(i, 0) = col0_at - (i - 1) col0_step
    const bool origin = d0 >= -63 && d0 <= 64;                 // (0,0) is in the band
    const int row0_at = begin2 ? 0 : origin ? -gap_open : kNeg, row0_step = !begin2 && origin ? gap_extend : 0;
    const int col0_at = begin1 ? 0 : origin ? -gap_open : kNeg, col0_step = !begin1 && origin ? gap_extend : 0;

    // row scores of a seq1 byte, one-hot of a seq2 byte
    auto row_of = [&](uint32_t a) {
        const uint32_t lo = (a & 1u) ? rows.r[1] : rows.r[0], hi = (a & 1u) ? rows.r[3] : rows.r[2];
        return (int)((a & 2u) ? hi : lo);
    };
    auto hot_of = [](uint32_t b) { return (int)(1u << (8u * (b & 3u))); };
    auto load1 = [&](int idx) { return (uint32_t)s1[clamp_i(idx, 0, top1)]; };
    auto load2 = [&](int idx) { return (uint32_t)s2[clamp_i(idx, 0, top2)]; };

    // 0-based: r = i - 1 of the lane at the trip's first iteration (-1 on row 0), ce = j - 1 of its even cell there
    int r = i_lo - 1 - lane, ce = i_lo - 1 + lane - 64 + d0;
    int b_even = hot_of(load2(ce));
    uint32_t a_nxt[kBandTrip], b_nxt[kBandTrip];
#pragma unroll
    for (int k = 0; k < kBandTrip; ++k) {
        a_nxt[k] = load1(r + k);
        b_nxt[k] = load2(ce + 1 + k);
    }

    Cell c0{kNeg, kNeg, kNeg}, c1{kNeg, kNeg, kNeg};    // the lane's last even and odd cell: off the table
    int best = kNeg;
    uint32_t best_pos = 0;                               // i << 15 | j

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
            const int i = r + k + 1, j0 = ce + k + 1, j1 = j0 + 1;
            const bool row_in = (uint32_t)i <= (uint32_t)len1;
            const bool in0 = row_in && (uint32_t)j0 <= (uint32_t)len2, in1 = row_in && (uint32_t)j1 <= (uint32_t)len2;
            const bool int0 = in0 && i >= 1 && j0 >= 1, int1 = in1 && i >= 1 && j1 >= 1;
            // what a cell that is not interior holds: off the table kNeg, (0,0) 0, else its border's closed form
            const int col0 = i == 0 ? 0 : col0_at - (i - 1) * col0_step;
            const int row0_0 = row0_at - (j0 - 1) * row0_step;
            const int fix0 = !in0 ? kNeg : j0 == 0 ? col0 : row0_0;
            const int fix1 = !in1 ? kNeg : j1 == 0 ? col0 : row0_0 - row0_step;
            const bool last_row = i == len1;
            const bool cand_row = anywhere || (end2 && last_row);
            const bool cand0 = in0 && (cand_row || (j0 == len2 && (end1 || last_row)));
            const bool cand1 = in1 && (cand_row || (j1 == len2 && (end1 || last_row)));
            const uint32_t pos = ((uint32_t)i << 15) + (uint32_t)j0;
            uint32_t code0 = 0, code1 = 0;
            // even cell: left = lane m - 1's odd cell of the last iteration.  The shift stands outside the select: under a
            // branch on the lane it would run with lane 0 switched off, and lane 1 would read 0 from it
            const int left_in = from_below(c1.mf);
            const int left = lane == 0 ? kNeg : left_in;
            c0 = cell<false, kOge, kTb>(a_row[k], b_even, c0.h, c1.me, left, cost, fold, int0, fix0, code0);
            if (cand0 && c0.h > best) {
                best = c0.h;
                best_pos = pos;
            }
            // odd cell: up = lane m + 1's even cell of this iteration
            const int up_in = from_above(c0.me);
            const int up = lane == 63 ? kNeg : up_in;
            c1 = cell<false, kOge, kTb>(a_row[k], b_hot[k], c1.h, up, c0.mf, cost, fold, int1, fix1, code1);
            if (cand1 && c1.h > best) {
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

    // the first cell in row-major order among the lanes' bests; H is signed, so it is biased before the unsigned compare
    uint32_t key_hi = (uint32_t)best ^ 0x80000000u, key_lo = ~best_pos;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)key_hi, o), lo = (uint32_t)__shfl_xor((int)key_lo, o);
        const bool take = hi > key_hi || (hi == key_hi && lo > key_lo);
        key_hi = take ? hi : key_hi;
        key_lo = take ? lo : key_lo;
    }
    best = (int)(key_hi ^ 0x80000000u);
    best_pos = ~key_lo;
    if (best < kInfeasible) {               // wave-uniform: no candidate, or every candidate holds -infinity
        no_alignment();
        return;
    }
    const int bi = (int)(best_pos >> 15), bj = (int)(best_pos & 32767u);
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
        unsigned long long *mv = sh.mv;
        int i = bi, j = bj, state = 0;      // state: 0 = H, 2 = in a vertical gap (E), 1 = in a horizontal gap (F)
        int w_lo = n_trips;                 // the window holds trips [w_lo, w_lo + kBandWalkTrips): nothing yet
        uint32_t t = 0;
        unsigned long long word = 0;
        auto step = [&](int dir) {
            word |= (unsigned long long)dir << (2 * (t & 31u));
            ++t;
            if ((t & 31u) == 0) {
                if (lane == 0) mv[(t >> 5) - 1] = word;
                word = 0;
            }
        };
        bool lost = false;
        while (i >= 1 && j >= 1) {          // E(1, j) and F(i, 1) always open: the border is reached in state H
            const int dl = j - i - d0 + 64; // the band diagonal, 0 .. 127
            if ((uint32_t)dl > 127u) { lost = true; break; }                    // (never: the walk cannot leave the band)
            const int ln = dl >> 1, rel = i + ln - i_lo;                        // the lane and iteration that hold the cell
            if (rel < 0 || rel >= n_trips * kBandTrip) { lost = true; break; }  // (never: every cell of the table in the band was swept)
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
            if (state == 0) dir = (int)(c & 3u);
            if (dir == 0) { lost = true; break; }                               // (never: an interior cell's source is 1, 2 or 3)
            step(dir);
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
        // the border rule: a border that is not free is walked to (0,0) by forced steps
        if (!lost) {
            if (i == 0 && !begin2)
                for (; j > 0; --j) step(1);
            if (j == 0 && !begin1)
                for (; i > 0; --i) step(2);
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

hipError_t launch_banded_ragged(int kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n,
                                const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const Rows rows = pack_rows(sm);
    uint32_t *codes = reinterpret_cast<uint32_t *>(d_codes);
    return launch_variant(gap_open >= gap_extend, d_moves != nullptr, n, [&](auto oge, auto tb, dim3 grid, dim3 block) {
        if (kind == kRaggedGlobal)
            hipLaunchKernelGGL((banded_ragged_global_kernel<decltype(oge)::value, decltype(tb)::value>), grid, block, 0, stream, d_seq1s,
                               d_seq2s, d_slots, (uint32_t)n, rows, gap_open, gap_extend, (uint32_t)free_ends, d_scores, d_ends, codes,
                               d_moves, d_steps);
        else
            hipLaunchKernelGGL((banded_ragged_local_kernel<decltype(oge)::value, decltype(tb)::value>), grid, block, 0, stream, d_seq1s,
                               d_seq2s, d_slots, (uint32_t)n, rows, gap_open, gap_extend, d_scores, d_ends, codes, d_moves, d_steps);
    });
}

}  // namespace banded
}  // namespace swmi
