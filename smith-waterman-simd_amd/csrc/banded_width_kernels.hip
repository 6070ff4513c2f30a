// banded_width_kernels.hip -- the kernels of libswmi_banded_width.so (include/swmi_banded_width.h): the
// two banded kinds of banded_ragged_kernels.hip (section 37) on a batch of mixed (len1, len2), with a band of 128 K diagonals,
// K = 1, 2, 4 or 8, chosen per launch.  One template, <K, kind, open >= extend, traceback>: 32 kernels.
//
// MAPPING.  Section 33's row skew with a wider lane.  With delta = j - i - d0 + 64 K the band diagonal, 0 .. 128 K - 1, lane m
// owns the C = 2 K diagonals delta = C m .. C m + C - 1: its cells 0 .. C - 1, left to right in one row.  In iteration t the
// lane sits on row i_lo - m + t, so cell c is column j = i + C m + c - 64 K + d0.  Neighbours:
//   cell 0:      left = lane m - 1's cell C - 1 of t - 1        (one lane shift, taken before any cell of t is made)
//   cell c > 0:  left = own cell c - 1 of t
//   cell c:      diagonal = own cell c of t - 1
//   cell c < C - 1:  up = own cell c + 1 of t - 1               (the cells are made in order 0 .. C - 1, so it is still the old one)
//   cell C - 1:  up = lane m + 1's cell 0 of t                  (a second lane shift, behind cell 0)
// An iteration is two lane shifts and C cells whatever K; there are (swept rows + 63) iterations, in trips of kBandTrip = 4.
// With K = 1 this is banded_sweep.h's mapping and banded_ragged_kernels.hip's sweep.
//
// COLUMN BASES.  A lane holds the one-hots of its C columns; from one iteration to the next they move down one cell and one
// new base arrives for cell C - 1.  The trip's four iterations are unrolled, so inside a trip iteration k's cell c reads
// entry k + c of an array of C + 3 one-hots and nothing moves; at the trip's end C - 1 entries move down by four: (C - 1) / 4
// moves per iteration where a rotation takes C - 1, and no work per cell, which 2-bit packed bases would add (an extract and a
// shift per cell).  The row base and the one new column base are loaded one trip ahead, four bytes of each per lane and trip,
// as in section 33.  The 64 column loads of a wavefront are C - 1 bytes apart: 64 (C - 1) bytes, eight 128-byte lines at K = 8
// where K = 1 touches one or two.
//
// BOUNDS.  Each of 62 / 63 / 64 in the 128-wide kernels is the band inequality -64 K <= j - i - d0 <= 64 K - 1 solved for a row
// or a column (banded_internal.h, width_swept_rows); they are derived again where they stand below.
//
// CODES.  4 bits per cell, so K bytes per lane and iteration and 4 K per lane and trip, stored whole (one 4-, 8- or 16-byte
// store, two of 16 at K = 8): the alignment's bytes [(trip * 64 + lane) * 4 K ..), iteration k's at + k K, cells 2 x and 2 x + 1
// in byte x.  A wavefront's trip is 256 K contiguous bytes.
//
// WALK.  Wave-uniform as before.  The cell (i, j) is lane delta / C, cell delta mod C, iteration i - i_lo + lane.  A move
// changes delta by at most 1 and goes to iteration t or t - 1.  The LDS window stays 4 KiB per wavefront at every width: 16
// trips of the 64 / K lanes around the walk's lane, which are 256 contiguous bytes of each trip.  The walk is at least
// (32 / K - 1) C = 64 - 2 K diagonals from the window's lane borders after a load, so a window serves at least 48 steps.
//
// THE TRAPS of sections 33, 34 and 37 apply unchanged: the lane shifts run unconditionally with a select behind them, -2^29 is
// a value, a slot is read once into SGPRs, no byte of an empty sequence is read, the two "never" checks of the walk stay.
//
// TWO OBJECTS.  banded_long_kernels.hip compiles this text a second time with SWMI_BANDED_LONG_KERNELS for
// libswmi_banded_long.so (include/swmi_banded_long.h, section 41): lengths up to 65536.  Everything in which the two objects
// differ stands in the one block below the constants; the body tests kLong and nothing else.  There the best cell's position is
// i << 10 | delta (27 bits at i = 65536; within a row delta order is column order, so "first in row-major order" is kept),
// made behind the loop from the lane's iteration and cell (within a lane arrival order is row-major order, and the strict >
// keeps the first), where the 16384 kernels pack i << 15 | j, and the diagonal is clamped at +-131072, beyond +-(65536 + 512) of which no band
// touches a table.  INT32 RANGE at len1 = len2 = 65536, band 1024 (kHalf = 512), |d0| <= 131072: i_lo, i_hi and len2 + kHalf -
// d0 lie within +-197 122; r and ce within +-(65536 + 15 * 63 + 512 + 131072) < 2^18; the border closed forms reach 127 rows or
// columns of that size, below 2^25; rel = i - i_lo + lane < 65536 + 64 and n_trips <= 16400; the position is below 2^27; an
// alignment's codes are n_trips * 64 * K <= 8 396 800 dwords, indexed in size_t from a 64-bit code_off.  The values: with int8
// scores, gaps in [0, 127] and 65536 rows every finite H, E, F lies in [-127 * 131072 - 254, 127 * 65536], above kInfeasible;
// every value made from kNeg lies in [kNeg - 127 * 131072 - 254, kNeg + 127 * 65536], below kInfeasible and above INT32_MIN.
#include "banded_sweep.h"

namespace swmi {
namespace banded {
namespace {

constexpr int kNeg = -(1 << 29);            // minus infinity (global kind)
constexpr int kInfeasible = -(1 << 28);     // every finite value is above, every value made from kNeg below
constexpr unsigned kBegin1 = 1u, kBegin2 = 2u, kEnd1 = 4u, kEnd2 = 8u, kAnywhere = 16u;
constexpr int kNoAlignment = -2147483647 - 1;

typedef uint32_t Dwords2 __attribute__((ext_vector_type(2)));
typedef uint32_t Dwords4 __attribute__((ext_vector_type(4)));

// wavefronts per SIMD the kernels are compiled for: section 37's six at K = 1, and what the lane's 2 K cells leave above it
constexpr int width_waves_per_simd(int k) { return k == 1 ? 6 : k == 2 ? 4 : 3; }

// ---- what the two objects differ in: the kernel's and the launcher's name, the clamp of a diagonal, how a position is packed ----
#ifdef SWMI_BANDED_LONG_KERNELS
#define BANDED_KERNEL banded_long_kernel
#define BANDED_LAUNCHER launch_banded_long
constexpr bool kLong = true;
constexpr int kDiagClamp = kLongDiagClamp, kPosShift = 10;      // i << 10 | delta, delta < 1024
// The wavefronts per SIMD a kernel is compiled for: no fewer than the 16384 kernel of the same instantiation reaches.  Left at
// width_waves_per_simd, some local kernels come out a wavefront or two below theirs -- the ends-only ones (theirs: 8, 8 and 7, 7,
// 5 and 6 at K = 1, 2, 4, 8) and the K = 1 traceback one with open >= extend (7); every other instantiation reaches its
// sibling's or more on its own.
constexpr int kernel_waves(int k, bool global, bool oge, bool tb)
{
    if (global) return width_waves_per_simd(k);
    if (tb) return k == 1 && oge ? 7 : width_waves_per_simd(k);
    return k == 1 ? 8 : k == 2 ? (oge ? 8 : 7) : k == 4 ? 7 : oge ? 6 : 5;
}
#else
#define BANDED_KERNEL banded_width_kernel
#define BANDED_LAUNCHER launch_banded_width
constexpr bool kLong = false;
constexpr int kDiagClamp = kRaggedDiagClamp, kPosShift = 15;    // i << 15 | j, j < 32768
constexpr int kernel_waves(int k, bool, bool, bool) { return width_waves_per_simd(k); }
#endif
// ---- below this line the two objects are one text ----

template <int K, bool kGlobal, bool kOge, bool kTb>
__global__ void __launch_bounds__(64 * kWaves, kernel_waves(K, kGlobal, kOge, kTb))
BANDED_KERNEL(const uint8_t *__restrict__ seq1s, const uint8_t *__restrict__ seq2s, const RaggedSlot *__restrict__ slots, uint32_t n,
                    Rows rows, int gap_open, int gap_extend, uint32_t free_ends, int32_t *__restrict__ scores, int32_t *__restrict__ ends,
                    uint32_t *__restrict__ codes, unsigned long long *__restrict__ moves, uint32_t *__restrict__ steps)
{
    constexpr int C = 2 * K, kHalf = 64 * K, kBand = 128 * K;
    constexpr int kWinLanes = 64 / K;       // lanes of a trip the walk window holds: 256 bytes of codes
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t at = blockIdx.x * kWaves + (uint32_t)wv;
    if (at >= n) return;                    // wave-uniform; only wave-level synchronisation below

    // the wavefront's slot, wave-uniform
    const RaggedSlot slot = slots[at];
    const int len1 = __builtin_amdgcn_readfirstlane(slot.len1), len2 = __builtin_amdgcn_readfirstlane(slot.len2);
    const int d0 = __builtin_amdgcn_readfirstlane(clamp_i(slot.d0, -kDiagClamp, kDiagClamp));   // before any arithmetic
    const uint32_t pair = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot.index);
    const bool begin1 = free_ends & kBegin1, begin2 = free_ends & kBegin2, end1 = free_ends & kEnd1, end2 = free_ends & kEnd2;
    const bool anywhere = free_ends & kAnywhere;
    int32_t *e_out = ends + 4 * (size_t)pair;
    // the result of a band without a cell (local: score 0) or without a finite candidate (global: NO_ALIGNMENT)
    auto nothing = [&]() {
        if (lane == 0) {
            scores[pair] = kGlobal ? kNoAlignment : 0;
            e_out[0] = e_out[1] = 0;
            e_out[2] = e_out[3] = kTb ? 0 : -1;
            if constexpr (kTb) steps[pair] = 0;
        }
    };
    // The rows that hold a cell of the band.  j - i - d0 <= kHalf - 1 at the smallest column (1: interior cells, local kind; 0:
    // column 0 is a cell, global kind) gives i >= j - d0 - kHalf + 1; j - i - d0 >= -kHalf at column len2 gives i <= len2 + kHalf - d0.
    const int i_lo = max_i(kGlobal ? 0 : 1, (kGlobal ? 1 : 2) - kHalf - d0), i_hi = min_i(len1, len2 + kHalf - d0);
    if constexpr (kGlobal) {
        // the candidates in the band: the corner; column len2's rows with END1 (-kHalf <= len2 - i - d0 <= kHalf - 1); row len1's
        // columns with END2 (-kHalf <= j - len1 - d0 <= kHalf - 1); any cell
        const int dc = len2 - len1 - d0;
        const bool corner = dc >= -kHalf && dc <= kHalf - 1;
        const bool col = end1 && max_i(0, len2 - d0 - kHalf + 1) <= min_i(len1, len2 - d0 + kHalf);
        const bool row = end2 && max_i(0, len1 + d0 - kHalf) <= min_i(len2, len1 + d0 + kHalf - 1);
        if (i_lo > i_hi || !(corner || col || row || anywhere)) {
            nothing();
            return;
        }
    } else {
        if (len1 == 0 || len2 == 0 || i_lo > i_hi) {   // no interior cell in the band: before any load
            nothing();
            return;
        }
    }
    const int n_trips = (i_hi - i_lo + 64 + kBandTrip - 1) / kBandTrip;

    // an empty sequence (global kind) has no byte: its loads go to byte 0 of this wavefront's slot, and feed only cells that
    // are replaced
    const uint8_t *own = reinterpret_cast<const uint8_t *>(slots + at);
    const uint8_t *s1 = len1 ? seq1s + slot.off1 : own;
    const uint8_t *s2 = len2 ? seq2s + slot.off2 : own;
    const int top1 = max_i(len1 - 1, 0), top2 = max_i(len2 - 1, 0);
    uint32_t *cd = nullptr;
    if constexpr (kTb) cd = codes + slot.code_off;

    const int cost = kOge ? gap_extend : gap_open;
    const int fold = kOge ? gap_open - gap_extend : gap_extend - gap_open;
    // what a cell outside the band holds and hands over: local H = 0 (handed over folded), global -infinity
    const int out_h = kGlobal ? kNeg : 0, out_m = kGlobal ? kNeg : kOge ? -fold : 0;
    // the global borders' closed forms: H(0, j) = row0_at - (j - 1) row0_step, H(i, 0) = col0_at - (i - 1) col0_step.
    // (0, 0) is in the band iff -kHalf <= -d0 <= kHalf - 1
    const bool origin = d0 >= -kHalf + 1 && d0 <= kHalf;
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

    // 0-based: r = i - 1 of the lane at the trip's first iteration, ce = j - 1 of its cell 0 there: i = i_lo - lane,
    // j = i + C lane - kHalf + d0
    int r = i_lo - 1 - lane, ce = i_lo - 1 + (C - 1) * lane - kHalf + d0;
    int b_col[C - 1];                       // the one-hots of cells 0 .. C - 2 at the trip's first iteration
#pragma unroll
    for (int c = 0; c < C - 1; ++c) b_col[c] = hot_of(load2(ce + c));
    uint32_t a_nxt[kBandTrip], b_nxt[kBandTrip];
#pragma unroll
    for (int k = 0; k < kBandTrip; ++k) {
        a_nxt[k] = load1(r + k);
        b_nxt[k] = load2(ce + C - 1 + k);
    }

    int h[C], me[C], mf_last = out_m;      // the lane's last cells; mf of the last one, which lane m + 1 takes
#pragma unroll
    for (int c = 0; c < C; ++c) {
        h[c] = out_h;
        me[c] = out_m;
    }
    int best = kGlobal ? kNeg : 0;
    uint32_t best_pos = 0;                  // i << 15 | j; kLong: (iteration, cell), behind the loop i << 10 | delta

#pragma unroll 1
    for (int trip = 0; trip < n_trips; ++trip) {
        int a_row[kBandTrip], hot[C - 1 + kBandTrip];
#pragma unroll
        for (int c = 0; c < C - 1; ++c) hot[c] = b_col[c];
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            a_row[k] = row_of(a_nxt[k]);
            hot[C - 1 + k] = hot_of(b_nxt[k]);
        }
        // the next trip's bytes (clamped indices: behind the last trip they are loaded and not used)
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            a_nxt[k] = load1(r + kBandTrip + k);
            b_nxt[k] = load2(ce + C - 1 + kBandTrip + k);
        }
        uint32_t word[K];
#pragma unroll
        for (int x = 0; x < K; ++x) word[x] = 0;
#pragma unroll
        for (int k = 0; k < kBandTrip; ++k) {
            const int i = r + k + 1, j0 = ce + k + 1;
            const bool row_int = (uint32_t)(i - 1) < (uint32_t)len1;           // an interior row
            // Global kind, per row.  A cell that is not interior holds its border's closed form: column 0 col0 ((0,0): 0), row
            // 0 row0 - c row0_step.  A cell OFF the table takes the same select: no cell of the table has a neighbour off it
            // that is not itself a border cell, which is fixed, so what it holds is never read (all of it is bounded).
            const int col0 = i == 0 ? 0 : col0_at - (i - 1) * col0_step;
            int row0 = i == 0 ? row0_at - (j0 - 1) * row0_step : kNeg;
            // the candidates of this row are columns [cand_lo, cand_lo + cand_n): all of 0 .. len2 where any cell of the row
            // competes, column len2 alone where the last column's cell does, none off the table
            const bool last_row = i == len1, row_in = (uint32_t)i <= (uint32_t)len1;
            const bool cand_all = row_in && (anywhere || (end2 && last_row)), cand_end = row_in && (end1 || last_row);
            const int cand_lo = cand_all ? 0 : len2;
            const uint32_t cand_n = cand_all ? (uint32_t)len2 + 1u : cand_end ? 1u : 0u;
            // (kLong: inside the loop a position is the lane's iteration and cell, which is wave-uniform and takes no VGPR; the
            // lane turns its best one into i << 10 | delta behind the loop)
            uint32_t pos = kLong ? (uint32_t)((trip * kBandTrip + k) * C) : ((uint32_t)i << kPosShift) + (uint32_t)j0;
            // (... and is made per iteration: left alone the compiler keeps a trip's 8 K positions in SGPRs and spills three at K = 8)
            if constexpr (kLong) asm volatile("" : "+s"(pos));
            // cell 0's left = lane m - 1's last cell of the last iteration.  The shift stands outside the select: under a
            // branch on the lane it would run with lane 0 switched off, and lane 1 would read 0 from it
            const int left_in = from_below(mf_last);
            int mf = lane == 0 ? out_m : left_in;
            int up_in = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                int j = j0 + c;
                // K = 8, global kind: left alone the compiler makes the row's 16 x 4 lane masks ahead of its cells and spills
                // SGPRs.  Tying the column to the value that runs through the row makes each cell's tests behind the cell before.
                if constexpr (kGlobal && K == 8) asm volatile("" : "+v"(j), "+v"(mf));
                const bool keep = row_int && (uint32_t)(j - 1) < (uint32_t)len2;    // an interior cell
                bool cand = true;
                int fixed = 0;
                if constexpr (kGlobal) {
                    fixed = j == 0 ? col0 : row0;
                    row0 -= row0_step;      // (a running value: 2 K - 1 multiples of the step would each take an SGPR)
                    cand = (uint32_t)(j - cand_lo) < cand_n;
                }
                // the last cell's up = lane m + 1's cell 0 of this iteration, shifted in behind cell 0
                const int up = c < C - 1 ? me[c + 1] : lane == 63 ? out_m : up_in;
                uint32_t code = 0;
                const Cell x = cell<!kGlobal, kOge, kTb>(a_row[k], hot[k + c], h[c], up, mf, cost, fold, keep, fixed, code);
                h[c] = x.h;
                me[c] = x.me;
                mf = x.mf;
                if (c == 0) up_in = from_above(x.me);
                if (cand && x.h > best) {
                    best = x.h;
                    best_pos = pos + (uint32_t)c;
                }
                if constexpr (kTb) word[(k * C + c) / 8] |= code << (4 * ((k * C + c) % 8));
                // (the wide global kernels: nothing is scheduled across here, so that few cells' lane masks are live at once)
                if constexpr (kGlobal && K >= 4) if (c % (K == 8 ? 2 : 4) == 1) __builtin_amdgcn_sched_barrier(0);
            }
            mf_last = mf;
            if constexpr (K > 1) __builtin_amdgcn_sched_barrier(0);     // an iteration's 2 K cells are scheduled on their own
        }
        if constexpr (kTb) {
            uint32_t *to = cd + ((size_t)trip * 64 + lane) * K;
            if constexpr (K == 1) {
                *to = word[0];
            } else if constexpr (K == 2) {
                *reinterpret_cast<Dwords2 *>(to) = Dwords2{word[0], word[1]};
            } else {
#pragma unroll
                for (int x = 0; x < K; x += 4) *reinterpret_cast<Dwords4 *>(to + x) = Dwords4{word[x], word[x + 1], word[x + 2], word[x + 3]};
            }
        }
#pragma unroll
        for (int c = 0; c < C - 1; ++c) b_col[c] = hot[c + kBandTrip];
        r += kBandTrip;
        ce += kBandTrip;
    }

    // kLong: iteration t of lane m is row i_lo - m + t, and its cell c is band diagonal C m + c (a lane that took no cell makes
    // a position of no meaning here: it loses below, or no lane took one and no position is used)
    if constexpr (kLong) best_pos = ((uint32_t)(i_lo - lane + (int)(best_pos / C)) << kPosShift) + (uint32_t)(C * lane) + best_pos % C;
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
    if constexpr (kGlobal) {
        if (best < kInfeasible) {           // wave-uniform: no candidate, or every candidate holds -infinity
            nothing();
            return;
        }
    }
    // (kLong, local kind: a best of 0 is no cell, reported as (0, 0) as the other packing's position 0 is)
    const bool no_cell = kLong && !kGlobal && best == 0;
    const int b_hi = (int)(best_pos >> kPosShift), b_lo = (int)(best_pos & ((1u << kPosShift) - 1u));
    const int bi = no_cell ? 0 : b_hi, bj = !kLong ? b_lo : no_cell ? 0 : b_hi + d0 + b_lo - kHalf;
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
        unsigned long long *mv = moves + slot.move_off;
        int i = bi, j = bj, state = 0;      // state: 0 = H, 2 = in a vertical gap (E), 1 = in a horizontal gap (F)
        int w_lo = n_trips, l_lo = 0;       // the window holds trips [w_lo, w_lo + kBandWalkTrips) of lanes [l_lo, l_lo + kWinLanes): nothing yet
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
        // local: a border cell holds 0, the walk stops there in state H; global: E(1, j) and F(i, 1) always open, so the border
        // is reached in state H
        while (i >= 1 && j >= 1) {
            const int dl = j - i - d0 + kHalf;                                  // the band diagonal, 0 .. kBand - 1
            if ((uint32_t)dl > (uint32_t)(kBand - 1)) { lost = true; break; }   // (never: the walk cannot leave the band)
            const int ln = dl / C, cc = dl % C, rel = i - i_lo + ln;            // the lane, its cell and the iteration that hold the cell
            if (rel < 0 || rel >= n_trips * kBandTrip) { lost = true; break; }  // (never: every cell of the table in the band was swept)
            const int q = rel >> 2;
            if (q < w_lo || q >= w_lo + kBandWalkTrips || ln < l_lo || ln >= l_lo + kWinLanes) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();            // every lane is past its reads of the old window
                w_lo = max_i(q - (kBandWalkTrips - 1), 0);
                l_lo = clamp_i(ln - kWinLanes / 2, 0, 64 - kWinLanes);
                const int cnt = n_trips - w_lo < kBandWalkTrips ? n_trips - w_lo : kBandWalkTrips;
                // the window's lanes of a trip are 64 contiguous dwords: the last one read is dword
                // ((n_trips - 1) 64 + 64 - kWinLanes) K + 63 = n_trips 64 K - 1 of the alignment's n_trips 64 K
                for (int x = 0; x < cnt; ++x)
                    win[x * 64 + lane] = __builtin_nontemporal_load(cd + ((size_t)(w_lo + x) * 64 + l_lo) * K + lane);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            const uint32_t byte = win8[(q - w_lo) * 256 + (ln - l_lo) * (4 * K) + (rel & 3) * K + (cc >> 1)];
            const uint32_t c = (byte >> (4 * (cc & 1))) & 15u;
            // arrived in a gap: it ends here if the value this cell handed over opened it
            if (state == 2 && (c & 4u)) state = 0;
            if (state == 1 && (c & 8u)) state = 0;
            int dir = state;
            if (state == 0) dir = (int)(c & 3u);
            if (dir == 0) {                 // local: H = 0, the start cell; global: (never: an interior cell's source is 1, 2 or 3)
                lost = kGlobal;
                break;
            }
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
        // the global border rule: a border that is not free is walked to (0,0) by forced steps
        if constexpr (kGlobal) {
            if (!lost) {
                if (i == 0 && !begin2)
                    for (; j > 0; --j) step(1);
                if (j == 0 && !begin1)
                    for (; i > 0; --i) step(2);
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

template <int K>
hipError_t launch_width(int kind, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n, Rows rows, int gap_open,
                        int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends, uint32_t *codes, unsigned long long *d_moves,
                        uint32_t *d_steps, hipStream_t stream)
{
    return launch_variant(gap_open >= gap_extend, d_moves != nullptr, n, [&](auto oge, auto tb, dim3 grid, dim3 block) {
        if (kind == kRaggedGlobal)
            hipLaunchKernelGGL((BANDED_KERNEL<K, true, decltype(oge)::value, decltype(tb)::value>), grid, block, 0, stream, d_seq1s,
                               d_seq2s, d_slots, (uint32_t)n, rows, gap_open, gap_extend, (uint32_t)free_ends, d_scores, d_ends, codes, d_moves,
                               d_steps);
        else
            hipLaunchKernelGGL((BANDED_KERNEL<K, false, decltype(oge)::value, decltype(tb)::value>), grid, block, 0, stream, d_seq1s,
                               d_seq2s, d_slots, (uint32_t)n, rows, gap_open, gap_extend, 0u, d_scores, d_ends, codes, d_moves, d_steps);
    });
}

}  // namespace

hipError_t BANDED_LAUNCHER(int kind, int band, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t n,
                               const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                               unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (!width_is_legal(band)) return hipErrorInvalidValue;
    const Rows rows = pack_rows(sm);
    uint32_t *codes = reinterpret_cast<uint32_t *>(d_codes);
    auto go = [&](auto k) {
        return launch_width<decltype(k)::value>(kind, d_seq1s, d_seq2s, d_slots, n, rows, gap_open, gap_extend, free_ends, d_scores, d_ends,
                                                codes, d_moves, d_steps, stream);
    };
    switch (band / kBandWidth) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 4: return go(std::integral_constant<int, 4>{});
    default: return go(std::integral_constant<int, 8>{});
    }
}

}  // namespace banded
}  // namespace swmi
