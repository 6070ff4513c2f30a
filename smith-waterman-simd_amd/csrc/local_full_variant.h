// local_full_variant.h -- the linear-gap variant of the any-length local aligners (tile_sweep.h: what a variant supplies), shared by
// local_full_kernels.hip and local_long_kernels.hip, whose file comments tell the cell and its key range.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

constexpr int kFloor = 3 << 4;         // the floor candidate: H = 0, tag 3
constexpr int kStored = 2 << 4;        // tag of a stored key (= the diagonal candidate's)
constexpr uint32_t kStop = 3;          // code of a cell whose floor won

struct LocalLinear {
    static constexpr bool kWalkStops = true;
    static constexpr int kEnds = 4;
    static constexpr int kStageLanes = 64;
    static constexpr int kRowMin = 0;
    static constexpr int kZeroKey = kStored;       // the stored key of H = 0, column bits aside

    struct Gaps {
        int gap;
    };
    int g_up, g_left;

    __device__ __forceinline__ explicit LocalLinear(Gaps g) : g_up(-(g.gap << 6) - (1 << 4)), g_left(-(g.gap << 6) - (2 << 4)) {}

    static __device__ __forceinline__ int row0(int jj, int, Gaps) { return kStored | (kCols - 1 - jj); }
    __device__ __forceinline__ int border(int) const { return kStored; }                    // the borders hold 0
    __device__ __forceinline__ int left_border(int) const { return kStored; }

    template <bool TB>
    __device__ __forceinline__ int cell(int jj, int sc, int &d, int &lft, int &key, uint32_t &code) const
    {
        const int m = imax(max3(d + (sc << 6), key + g_up, lft + g_left), kFloor);
        const int nk = (m & ~63) | (kStored | (kCols - 1 - jj));
        if constexpr (TB) code = ((uint32_t)(m >> 4) & 3u) << (2 * jj);
        d = key;
        key = nk;
        lft = nk;
        return nk;
    }

    // a stop code: the cell holds 0, the start cell; else the move is code + 1
    static __device__ __forceinline__ uint32_t step(uint32_t wd, int cc)
    {
        const uint32_t code = (wd >> (2 * cc)) & 3u;
        return code == kStop ? 0u : code + 1;
    }
};

}  // namespace
}  // namespace swmi
