// compat_global_long.cpp -- the C++ overloads of the long global / fit / overlap aligners (include/swmi_compat.hpp):
// NeedlemanWunsch_long_mi355x, NeedlemanWunsch_long_affine_mi355x and their swmi::..._batch forms.  Compiled by
// tests/test_global_long_cpu.py (no device needed to compile and link), run by tests/test_global_long_gpu.py.
//
//   compat_global_long <file> <free_ends> <piece> [gap_extend]
//
// <file>: int32 n, len1, len2, gap; int8 sm[16]; then n times (seq1[len1], seq2[len2]).  With gap_extend the affine overloads
// run, `gap` the open cost.  Prints one line per alignment of the batch overload, "score positions end_i end_j checksum"
// (checksum over the path's (i, j) from the start cell to the end cell), then "single <k>" = how many of the first two
// alignments differ between the single and the batch overload, then "ragged <0|1>" = whether a batch of differing lengths
// threw std::invalid_argument.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
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
    const unsigned free_ends = unsigned(atol(argv[2]));
    const size_t piece = size_t(atol(argv[3]));
    const bool affine = argc > 4;
    const int extend = affine ? atoi(argv[4]) : 0;
    if (swmi_init(0) != SWMI_OK) {
        fprintf(stderr, "swmi_init: %s\n", swmi_last_error());
        return 1;
    }
    try {
        auto run = [&](const std::vector<std::vector<uint8_t>> &s2) {
            return affine ? swmi::NeedlemanWunsch_long_affine_mi355x_batch(seq1s, s2, sm, gap, extend, free_ends, piece, 3)
                          : swmi::NeedlemanWunsch_long_mi355x_batch(seq1s, s2, sm, int8_t(gap), free_ends, piece, 3);
        };
        const auto batch = run(seq2s);
        for (const auto &r : batch) {
            unsigned long long sum = 0;
            for (const auto &p : r.second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
            printf("%d %zu %d %d %llu\n", r.first, r.second.size(), r.second.back().first, r.second.back().second, sum);
        }
        size_t differ = 0;
        for (size_t k = 0; k < n && k < 2; ++k)
            differ += (affine ? NeedlemanWunsch_long_affine_mi355x(seq1s[k], seq2s[k], sm, gap, extend, free_ends)
                              : NeedlemanWunsch_long_mi355x(seq1s[k], seq2s[k], sm, int8_t(gap), free_ends)) != batch[k];
        printf("single %zu\n", differ);
        int threw = 0;
        if (n >= 2) {
            auto bad = seq2s;
            bad[1].push_back(0);
            try {
                (void)run(bad);
            } catch (const std::invalid_argument &) {
                threw = 1;
            }
        }
        printf("ragged %d\n", threw);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    swmi_shutdown();
    return 0;
}
