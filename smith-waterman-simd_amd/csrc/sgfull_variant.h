// sgfull_variant.h -- the linear-gap variant of the exact semi-global aligners (tile_sweep.h: what a variant supplies), shared by
// sgfull_kernels.hip and sgfull_long_kernels.hip, whose file comments tell the cell and its key range.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

constexpr int kTag3 = 3 << 4;

// H(0, j) = H(j, 0) as a stored key, from nj = -j
__device__ __forceinline__ int border_key(int nj, int gap) { return ((nj * gap) << 6) | kTag3; }

struct SgLinear {
    static constexpr bool kWalkStops = false;
    static constexpr int kEnds = 2;
    static constexpr int kStageLanes = 64;
    static constexpr int kRowMin = (int)0x80000000;
    static constexpr int kZeroKey = kTag3;       // the stored key of H = 0, column bits aside

    struct Gaps {
        int gap;
    };
    int gap, g_up, g_left;

    __device__ __forceinline__ explicit SgLinear(Gaps g) : gap(g.gap), g_up(-(g.gap << 6) - (1 << 4)), g_left(-(g.gap << 6) - (2 << 4)) {}

    static __device__ __forceinline__ int row0(int, int nj, Gaps g) { return border_key(nj, g.gap); }
    __device__ __forceinline__ int border(int nj) const { return border_key(nj, gap); }
    __device__ __forceinline__ int left_border(int nrow) const { return border(nrow); }

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
