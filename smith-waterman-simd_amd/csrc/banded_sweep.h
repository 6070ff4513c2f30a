// banded_sweep.h -- what the kernels of libswmi_banded.so (banded_align_kernels.hip) and of
// libswmi_banded_global.so (banded_global_kernels.hip, section 34) share: the lane mapping, the cell with its folded gaps and its
// code, the packed matrix and the launch dispatch (section 35).  Each file keeps its own kernel: which rows it sweeps, what a
// cell outside the table holds, which cells compete for the best, and how the walk ends.
//
// MAPPING (section 9's, with the int32 cell).  One wavefront sweeps ONE alignment's anti-diagonals; lane m owns band diagonals
// 2m (its even cell) and 2m + 1 (its odd cell).  From one iteration to the next a lane moves one row down; its even cell is
// column j = i + 2m - 64 + d0 and its odd cell column j + 1.  Neighbours, with t the iteration:
//   even cell: diagonal = own even cell of t - 1, up = own odd cell of t - 1, left = lane m - 1's odd cell of t - 1
//   odd cell:  diagonal = own odd cell of t - 1,  left = own even cell of t,  up = lane m + 1's even cell of t
// Only rows that meet the band are swept, in whole trips of kBandTrip = 4 iterations.  Outside the BAND lie lane 0's left and
// lane 63's upper neighbour; the lane shift delivers nothing there and a select puts the kernel's hand-over value in its place.
//
// SEQUENCES: no LDS stage.  Every lane loads its own row base and column base (the odd cell's: the even cell's is last
// iteration's odd one) one trip ahead, four bytes of each per trip, from indices clamped into the sequence.  A wavefront's
// 64 bytes of one load are consecutive, so they cost one or two cache lines; the LDS a wavefront takes does not depend on the
// lengths (the traceback kernels hold the walk window there, the ends-only kernels nothing).
//
// GAPS are folded as in section 9, on signed int32 without saturation.  A cell hands ONE value down (me) and one to the right
// (mf); with fold = |open - extend| and cost = min(open, extend):
//   open >= extend:  a = H - fold, me = max(a, E), mf = max(a, F)            and the receiver takes  E' = me - extend
//   open <  extend:  a = H,        me = max(a, E - fold), mf = max(a, F - fold)   and                E' = me - open
// E' opened (came from H) iff a >= its partner: the tie goes to the opening.  That bit is known where the value is made, so it
// is stored in the code of the cell that HANDS OVER, and the walk reads it after its up or left move, in the cell it arrives
// at, which it has to read anyway.  A cell that holds H = fixed, E = F = -infinity hands over (open >= extend ? fixed - fold :
// fixed).
//
// CODES: 4 bits per cell: bits 0-1 H's source (0 stop, 3 diagonal, 2 E, 1 F, tested in that order), bit 2 "the E handed down
// opens", bit 3 "the F handed right opens".  A lane's two cells of an iteration are one byte, its four iterations of a trip one
// dword: dword (trip * 64 + lane) of the alignment's codes, a 256-byte store per wavefront and trip.
//
// WALK: all 64 lanes walk the same cell (wave-uniform; lane 0 stores).  The codes of kBandWalkTrips trips ending at the walk's
// trip are loaded into LDS by the whole wavefront; every move goes to iteration t or t - 1, so a window serves at least 64 steps.
#ifndef SWMI_BANDED_SWEEP_H
#define SWMI_BANDED_SWEEP_H

#include "banded_internal.h"

#include <hip/hip_runtime.h>

#include <type_traits>

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
__device__ __forceinline__ int min_i(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

struct Cell {
    int h, me, mf;
};

// One cell from its diagonal H, the values handed to it and its substitution row / column one-hot.  `keep`: the recurrence's
// value stands; else the cell holds H = `fixed` with E = F = -infinity.  kFloor (the local kernels, which pass fixed = 0): H has
// a floor at 0, whose source code is "stop", and a cell that is not kept stores code 12 ("stop", both gaps open); without it a
// cell that is not kept stores a code that the walk never reads.
template <bool kFloor, bool kOge, bool kTb>
__device__ __forceinline__ Cell cell(int arow, int boh, int h_diag, int me_up, int mf_left, int cost, int fold, bool keep, int fixed,
                                     uint32_t &code)
{
    const int e = me_up - cost, f = mf_left - cost;
    const int d = __builtin_amdgcn_sdot4(arow, boh, h_diag, false);
    const int h = kFloor ? max_i(max_i(d, e), max_i(f, 0)) : max_i(d, max_i(e, f));
    const int a = kOge ? h - fold : h;
    const int eb = kOge ? e : e - fold, fb = kOge ? f : f - fold;
    if constexpr (kTb) {
        const uint32_t src = kFloor && h == 0 ? 0u : h == d ? 3u : h == e ? 2u : 1u;
        const uint32_t c = src | (a >= eb ? 4u : 0u) | (a >= fb ? 8u : 0u);
        code = kFloor ? (keep ? c : 12u) : c;
    }
    const int fa = kOge ? fixed - fold : fixed;
    Cell out;
    out.h = keep ? h : fixed;
    out.me = keep ? max_i(a, eb) : fa;
    out.mf = keep ? max_i(a, fb) : fa;
    return out;
}

// the matrix as the kernels take it (host)
inline Rows pack_rows(const int8_t *sm)
{
    Rows rows;
    for (int a = 0; a < 4; ++a) {
        rows.r[a] = 0;
        for (int b = 0; b < 4; ++b) rows.r[a] |= (uint32_t)(uint8_t)sm[4 * a + b] << (8 * b);
    }
    return rows;
}

// The four-way dispatch of a launch of n alignments: calls launch(oge, tb, grid, block) once, with oge and tb as
// std::bool_constant for the kernel's template arguments <kOge, kTb>.
template <class Launch>
inline hipError_t launch_variant(bool oge, bool tb, size_t n, Launch launch)
{
    const dim3 grid((unsigned)((n + kWaves - 1) / kWaves)), block(64 * kWaves);
    if (tb) {
        if (oge) launch(std::true_type{}, std::true_type{}, grid, block);
        else launch(std::false_type{}, std::true_type{}, grid, block);
    } else {
        if (oge) launch(std::true_type{}, std::false_type{}, grid, block);
        else launch(std::false_type{}, std::false_type{}, grid, block);
    }
    return hipGetLastError();
}

}  // namespace
}  // namespace banded
}  // namespace swmi

#endif
