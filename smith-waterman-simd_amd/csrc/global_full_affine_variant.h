// global_full_affine_variant.h -- the affine-gap variant of the global and free-end-gap aligners (tile_sweep.h: what an affine variant
// supplies), shared by global_full_affine_kernels.hip and global_long_affine_kernels.hip, whose file comments tell the cell.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

struct GlobalAffine {
    static constexpr bool kWalkStops = false;
    static constexpr bool kFreeEnds = true;        // the end rule of tile_sweep.h
    static constexpr int kEnds = 4;
    static constexpr int kRowMin = (int)0x80000000;
    static constexpr int kTagH = 3 << 4;
    static constexpr int kTagE = 2 << 4;
    static constexpr int kTagF = 1 << 4;
    static constexpr int kOpenBitE = 4;            // kTagH has it, kTagE has not
    static constexpr int kOpenBitF = 5;            // kTagH has it, kTagF has not

    // H(0, j) or H(j, 0) for j >= 1 (and 0 at j = 0) as a stored key, from THAT border's open and extend (0, 0 where it is free)
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
