// compat_semiglobal_long.cpp -- the C++ overloads of the long semi-global aligners (include/swmi_compat.hpp): SemiGlobal_long_mi355x,
// SemiGlobal_long_affine_mi355x and their swmi::..._batch forms.  Compiled by tests/test_semiglobal_long_cpu.py (no device needed
// to compile and link), run by tests/test_semiglobal_long_gpu.py and tests/test_semiglobal_long_affine_gpu.py.
//
//   compat_semiglobal_long <file> <piece> [gap_extend]
//
// <file>: int32 n, len1, len2, gap; int8 sm[16]; then n times (seq1[len1], seq2[len2]).  With gap_extend the affine overloads
// run, `gap` the open cost.  Prints one line per alignment of the batch overload, "score positions end_i end_j checksum"
// (checksum over the path's (i, j) from (0, 0) to the best cell), then "single <k>" = how many alignments differ
// between the single and the batch overload.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    std::array<int8_t, 16> sm;
    if (fread(head, 4, 4, f) != 4 || fread(sm.data(), 1, 16, f) != 16) return 2;
    const size_t n = size_t(head[0]), len1 = size_t(head[1]), len2 = size_t(head[2]);
    const int gap = head[3];
    std::vector<std::vector<uint8_t>> seq1s(n, std::vector<uint8_t>(len1)), seq2s(n, std::vector<uint8_t>(len2));
    for (size_t k = 0; k < n; ++k)
        if (fread(seq1s[k].data(), 1, len1, f) != len1 || fread(seq2s[k].data(), 1, len2, f) != len2) return 2;
    fclose(f);
    const size_t piece = size_t(atol(argv[2]));
    const bool affine = argc > 3;
    const int extend = affine ? atoi(argv[3]) : 0;
    if (swmi_init(0) != SWMI_OK) {
        fprintf(stderr, "swmi_init: %s\n", swmi_last_error());
        return 1;
    }
    try {
        const auto batch = affine ? swmi::SemiGlobal_long_affine_mi355x_batch(seq1s, seq2s, sm, gap, extend, piece, 3)
                                  : swmi::SemiGlobal_long_mi355x_batch(seq1s, seq2s, sm, int8_t(gap), piece, 3);
        for (const auto &r : batch) {
            unsigned long long sum = 0;
            for (const auto &p : r.second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
            printf("%d %zu %d %d %llu\n", r.first, r.second.size(), r.second.back().first, r.second.back().second, sum);
        }
        size_t differ = 0;
        for (size_t k = 0; k < n; ++k)
            differ += (affine ? SemiGlobal_long_affine_mi355x(seq1s[k], seq2s[k], sm, gap, extend)
                              : SemiGlobal_long_mi355x(seq1s[k], seq2s[k], sm, int8_t(gap))) != batch[k];
        printf("single %zu\n", differ);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    swmi_shutdown();
    return 0;
}
