// sgfull_affine_variant.h -- the affine-gap variant of the exact semi-global aligners (tile_sweep.h: what an affine variant
// supplies), shared by sgfull_affine_kernels.hip and sgfull_long_affine_kernels.hip, whose file comments tell the cell and its
// key range.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

struct SgAffine {
    static constexpr bool kWalkStops = false;
    static constexpr int kEnds = 2;
    static constexpr int kRowMin = (int)0x80000000;
    static constexpr int kTagH = 3 << 4;
    static constexpr int kTagE = 2 << 4;
    static constexpr int kTagF = 1 << 4;
    static constexpr int kOpenBitE = 4;            // kTagH has it, kTagE has not
    static constexpr int kOpenBitF = 5;            // kTagH has it, kTagF has not

    // H(0, j) = H(j, 0) for j >= 1 (and 0 at j = 0) as a stored key
    static __device__ __forceinline__ int border(int j, int gap_open, int gap_extend)
    {
        const int h = j > 0 ? -(gap_open + (j - 1) * gap_extend) : 0;
        return (h << 6) | kTagH;
    }
    static __device__ __forceinline__ int row0(int, int j, int gap_open, int gap_extend) { return border(j, gap_open, gap_extend); }
    static __device__ __forceinline__ int floor(int m) { return m; }
};

}  // namespace
}  // namespace swmi
