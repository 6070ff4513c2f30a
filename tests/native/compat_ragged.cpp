// compat_ragged.cpp -- include/swmi_compat.hpp's ragged local-alignment overloads from a plain C++ program (g++, no HIP
// headers).  Input file (that of compat_local.cpp): int32 n, then per alignment int32 len1, len1 bytes of seq1, 128 bytes of
// seq2.  Output, one line per alignment from ONE swmi::SmithWaterman_111_long_mi355x_batch call over the whole mixed-length
// batch: score, path length, first (i, j), last (i, j), a checksum of the whole path.  A final line "mismatches a b c" counts
// the alignments where it differs from SmithWaterman_local_mi355x_ragged_batch at (1, -1, 1) in pieces of 7 (a), from
// SmithWaterman_affine_mi355x_ragged_batch at open = extend = 1 (b), and from SmithWaterman_111_long_mi355x call by call (c).
#include <cstdio>
#include <fstream>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int32_t n = 0;
    in.read(reinterpret_cast<char *>(&n), 4);
    std::vector<std::vector<uint8_t>> s1(n);
    std::vector<std::array<uint8_t, 128>> s2(n);
    for (int k = 0; k < n; ++k) {
        int32_t len1 = 0;
        in.read(reinterpret_cast<char *>(&len1), 4);
        s1[k].resize(len1);
        in.read(reinterpret_cast<char *>(s1[k].data()), len1);
        in.read(reinterpret_cast<char *>(s2[k].data()), 128);
    }
    if (!in) return 3;
    const auto all = swmi::SmithWaterman_111_long_mi355x_batch(s1, s2);
    if ((int)all.size() != n) return 4;
    for (int k = 0; k < n; ++k) {
        unsigned long long sum = 0;
        for (const auto &p : all[k].second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
        const auto &path = all[k].second;
        std::printf("%d %zu %d %d %d %d %llu\n", all[k].first, path.size(), path.front().first, path.front().second,
                    path.back().first, path.back().second, sum);
    }
    const std::array<int8_t, 16> k111 = {1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1};
    const auto pieces = swmi::SmithWaterman_local_mi355x_ragged_batch(s1, s2, k111, 1, 7);
    const auto affine = swmi::SmithWaterman_affine_mi355x_ragged_batch(s1, s2, k111, 1, 1);
    int a = 0, b = 0, c = 0;
    for (int k = 0; k < n; ++k) {
        a += pieces[k] != all[k];
        b += affine[k] != all[k];
        c += SmithWaterman_111_long_mi355x(s1[k], s2[k]) != all[k];
    }
    std::printf("mismatches %d %d %d\n", a, b, c);
    return 0;
}
