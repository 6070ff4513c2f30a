// ref_sgfull_shim.cpp -- fixture tooling only (tests/golden/make_golden_sgfull.py compiles it into a temporary directory).
//
// Exports the reference's own SemiGlobal_111 (source.cpp:1776-1834) and SemiGlobal_AdaptiveBanded_XDrop_111_32_70
// (:1836-1976) through C wrappers, so that the F8 fixture records what those functions returned.  No reference source is
// copied: the translation unit #includes the file where it lies (SWREF_SOURCE, passed by the generator) with its main()
// renamed, the way ref_local_shim.cpp does.
#include <cstddef>
#include <cstdint>

#define main swref_sgfull_reference_main
#include SWREF_SOURCE
#undef main

namespace {

template <class F>
int call(F f, const uint8_t *seq1, const uint8_t *seq2, int32_t *path, size_t cap, size_t *length)
{
    std::array<uint8_t, 16384> a, b;
    for (size_t j = 0; j < 16384; ++j) {
        a[j] = seq1[j];
        b[j] = seq2[j];
    }
    const auto r = f(a, b);
    *length = r.second.size();
    for (size_t k = 0; k < r.second.size() && k < cap; ++k) {
        path[2 * k] = r.second[k].first;
        path[2 * k + 1] = r.second[k].second;
    }
    return r.first;
}

}  // namespace

extern "C" {

// (score, path) of SemiGlobal_111(seq1, seq2) on two 16384-mers; path = (i, j) pairs from (0,0) to the best cell, at most
// `cap` written; *length = the path's full length.
int swref_sgfull_111(const uint8_t *seq1, const uint8_t *seq2, int32_t *path, size_t cap, size_t *length)
{
    return call(SemiGlobal_111, seq1, seq2, path, cap, length);
}

// the same for SemiGlobal_AdaptiveBanded_XDrop_111_32_70
int swref_sgxdrop_111(const uint8_t *seq1, const uint8_t *seq2, int32_t *path, size_t cap, size_t *length)
{
    return call(SemiGlobal_AdaptiveBanded_XDrop_111_32_70, seq1, seq2, path, cap, length);
}

}  // extern "C"
