// global_full_variant.h -- the linear-gap variant of the global and free-end-gap aligners (tile_sweep.h: what a variant supplies),
// shared by global_full_kernels.hip and global_long_kernels.hip, whose file comments tell the cell and its key range.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

constexpr int kTag3 = 3 << 4;

// the stored key of -n gap from nn = -n, column bits aside
__device__ __forceinline__ int border_key(int nn, int gap) { return ((nn * gap) << 6) | kTag3; }

struct GlobalLinear {
    static constexpr bool kWalkStops = false;
    static constexpr bool kFreeEnds = true;      // the end rule of tile_sweep.h
    static constexpr int kEnds = 4;
    static constexpr int kStageLanes = 64;
    static constexpr int kRowMin = (int)0x80000000;
    static constexpr int kZeroKey = kTag3;       // the stored key of H = 0, column bits aside

    struct Gaps {
        int gap;
        unsigned free_ends;
    };
    int g_up, g_left, gap_row0, gap_col0;        // gap_row0, gap_col0: what a step along row 0 / column 0 costs

    __device__ __forceinline__ explicit GlobalLinear(Gaps g)
        : g_up(-(g.gap << 6) - (1 << 4)), g_left(-(g.gap << 6) - (2 << 4)), gap_row0(g.free_ends & kFreeBegin2 ? 0 : g.gap),
          gap_col0(g.free_ends & kFreeBegin1 ? 0 : g.gap)
    {
    }

    static __device__ __forceinline__ int row0(int, int nj, Gaps g) { return border_key(nj, g.free_ends & kFreeBegin2 ? 0 : g.gap); }
    __device__ __forceinline__ int border(int nj) const { return border_key(nj, gap_row0); }
    __device__ __forceinline__ int left_border(int nrow) const { return border_key(nrow, gap_col0); }

    template <bool TB>
    __device__ __forceinline__ int cell(int jj, int sc, int &d, int &lft, int &key, uint32_t &code) const
    {
        const int m = max3(d + (sc << 6), key + g_up, lft + g_left);
        const int nk = (m & ~63) | (kTag3 | (kCols - 1 - jj));
        if constexpr (TB) code = ((uint32_t)(m >> 4) & 3u) << (2 * jj);
        d = key;
        key = nk;
        lft = nk;
        return nk;
    }

    static __device__ __forceinline__ uint32_t step(uint32_t wd, int cc) { return (wd >> (2 * cc)) & 3u; }
};

}  // namespace
}  // namespace swmi
