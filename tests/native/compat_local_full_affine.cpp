// compat_local_full_affine.cpp -- the C++ overloads of the any-length affine local aligner (include/swmi_compat.hpp):
// SmithWaterman_long_affine_mi355x and swmi::SmithWaterman_long_affine_mi355x_batch.  Compiled by
// tests/test_table_host_fake.py (no device needed to compile and link), run by tests/test_local_full_affine_gpu.py.
//
//   compat_local_full_affine <file> [piece]
//
// <file>: int32 n, len1, len2, gap_open, gap_extend; int8 sm[16]; then n times (seq1[len1], seq2[len2]).  Prints one line per alignment of the
// batch overload, "score positions end_i end_j checksum" (checksum over the path's (i, j) from the start cell to the end
// cell), then "single <k>" = how many of the first alignments differ between the single and the batch overload, then
// "ragged <0|1>" = whether a batch of differing lengths threw std::invalid_argument, then "linear <k>" = how many of the first
// alignments differ between SmithWaterman_long_affine_mi355x(a, b, 111-matrix, 1, 1) and SmithWaterman_long_mi355x(a, b, 111-matrix, 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    std::array<int8_t, 16> sm;
    if (fread(head, 4, 5, f) != 5 || fread(sm.data(), 1, 16, f) != 16) return 2;
    const size_t n = size_t(head[0]), len1 = size_t(head[1]), len2 = size_t(head[2]);
    const int gap_open = head[3], gap_extend = head[4];
    std::vector<std::vector<uint8_t>> seq1s(n, std::vector<uint8_t>(len1)), seq2s(n, std::vector<uint8_t>(len2));
    for (size_t k = 0; k < n; ++k)
        if (fread(seq1s[k].data(), 1, len1, f) != len1 || fread(seq2s[k].data(), 1, len2, f) != len2) return 2;
    fclose(f);
    const size_t piece = argc > 2 ? size_t(atol(argv[2])) : 0;
    if (swmi_init(0) != SWMI_OK) {
        fprintf(stderr, "swmi_init: %s\n", swmi_last_error());
        return 1;
    }
    try {
        const auto batch = swmi::SmithWaterman_long_affine_mi355x_batch(seq1s, seq2s, sm, gap_open, gap_extend, piece, 3);
        for (const auto &r : batch) {
            unsigned long long sum = 0;
            for (const auto &p : r.second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
            printf("%d %zu %d %d %llu\n", r.first, r.second.size(), r.second.back().first, r.second.back().second, sum);
        }
        size_t differ = 0;
        for (size_t k = 0; k < n && k < 4; ++k) differ += SmithWaterman_long_affine_mi355x(seq1s[k], seq2s[k], sm, gap_open, gap_extend) != batch[k];
        printf("single %zu\n", differ);
        int threw = 0;
        if (n >= 2) {
            auto bad = seq2s;
            bad[1].push_back(0);
            try {
                (void)swmi::SmithWaterman_long_affine_mi355x_batch(seq1s, bad, sm, gap_open, gap_extend);
            } catch (const std::invalid_argument &) {
                threw = 1;
            }
        }
        printf("ragged %d\n", threw);
        size_t linear = 0;
        const auto &m111 = swmi::semiglobal_111_matrix();
        for (size_t k = 0; k < n && k < 4; ++k)
            linear += SmithWaterman_long_affine_mi355x(seq1s[k], seq2s[k], m111, 1, 1) != SmithWaterman_long_mi355x(seq1s[k], seq2s[k], m111, 1);
        printf("linear %zu\n", linear);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    swmi_shutdown();
    return 0;
}
