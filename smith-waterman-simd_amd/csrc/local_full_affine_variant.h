// local_full_affine_variant.h -- the affine-gap variant of the any-length local aligners (tile_sweep.h: what an affine variant
// supplies), shared by local_full_affine_kernels.hip and local_long_affine_kernels.hip, whose file comments tell the cell and its
// key range.
#pragma once
#include "tile_sweep.h"

namespace swmi {
namespace {

using namespace tile;

struct LocalAffine {
    static constexpr bool kWalkStops = true;       // on the floor's code, kTagH's + 1
    static constexpr int kEnds = 4;
    static constexpr int kRowMin = 0;
    static constexpr int kTagH = 2 << 4;           // of a stored H key (= the diagonal's and both open candidates')
    static constexpr int kTagE = 1 << 4;
    static constexpr int kTagF = 0 << 4;
    static constexpr int kFloor = 3 << 4;          // the floor candidate: H = 0, tag 3
    static constexpr int kOpenBitE = 5;            // kTagH has it, kTagE and kTagF have not
    static constexpr int kOpenBitF = 5;

    static __device__ __forceinline__ int border(int, int, int) { return kTagH; }                          // the borders hold 0
    static __device__ __forceinline__ int row0(int jj, int, int, int) { return kTagH | (kCols - 1 - jj); }
    static __device__ __forceinline__ int floor(int m) { return imax(m, kFloor); }
};

}  // namespace
}  // namespace swmi
