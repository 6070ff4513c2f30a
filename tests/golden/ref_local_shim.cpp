// ref_local_shim.cpp -- fixture tooling only (tests/golden/make_golden_local.py compiles it into a temporary directory).
//
// Exports the reference's own SmithWaterman_111_long (source.cpp:1526-1576) through a C wrapper, so that the F7 fixture
// records what that function returned.  No reference source is copied: the translation unit #includes the file where it
// lies (SWREF_SOURCE, passed by the generator) with its main() renamed, the way oracle/ref_shim.cpp does.
#include <cstddef>
#include <cstdint>

#define main swref_local_reference_main
#include SWREF_SOURCE
#undef main

extern "C" {

// (score, path) of SmithWaterman_111_long(seq1[0..len1), seq2[0..128)); path = (i, j) pairs from the start cell to the
// end cell, at most `cap` written; *length = the path's full length.
int swref_local_111(const uint8_t *seq1, size_t len1, const uint8_t *seq2, int32_t *path, size_t cap, size_t *length)
{
    const std::vector<uint8_t> a(seq1, seq1 + len1);
    std::array<uint8_t, 128> b;
    for (size_t j = 0; j < 128; ++j) b[j] = seq2[j];
    const auto r = SmithWaterman_111_long(a, b);
    *length = r.second.size();
    for (size_t k = 0; k < r.second.size() && k < cap; ++k) {
        path[2 * k] = r.second[k].first;
        path[2 * k + 1] = r.second[k].second;
    }
    return r.first;
}

}  // extern "C"
