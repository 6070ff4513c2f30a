// compat_sgfull.cpp -- include/swmi_compat.hpp's SemiGlobal_111 overloads from a plain C++ program (g++, no HIP headers).
// Input file: int32 n, then per alignment 16384 bytes of seq1 and 16384 bytes of seq2.  Output, one line per alignment:
// score, path length, last (i, j), a checksum of the whole path -- from SemiGlobal_111_mi355x; a final line
// "batch <mismatches>" compares swmi::SemiGlobal_111_mi355x_batch (pieces of 5 alignments) with it.
#include <cstdio>
#include <fstream>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int32_t n = 0;
    in.read(reinterpret_cast<char *>(&n), 4);
    std::vector<std::array<uint8_t, 16384>> s1(n), s2(n);
    for (int k = 0; k < n; ++k) {
        in.read(reinterpret_cast<char *>(s1[k].data()), 16384);
        in.read(reinterpret_cast<char *>(s2[k].data()), 16384);
    }
    if (!in) return 3;
    std::vector<std::pair<int, std::vector<std::pair<int, int>>>> one(n);
    for (int k = 0; k < n; ++k) {
        one[k] = SemiGlobal_111_mi355x(s1[k], s2[k]);
        unsigned long long sum = 0;
        for (const auto &p : one[k].second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
        const auto &path = one[k].second;
        std::printf("%d %zu %d %d %llu\n", one[k].first, path.size(), path.back().first, path.back().second, sum);
    }
    const auto got = swmi::SemiGlobal_111_mi355x_batch(s1, s2, 3, 5);
    int mismatches = 0;
    for (int k = 0; k < n; ++k) mismatches += got[k] != one[k];
    std::printf("batch %d\n", mismatches);
    return 0;
}
