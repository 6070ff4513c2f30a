// compat_sgfull_affine.cpp -- include/swmi_compat.hpp's affine exact semi-global overloads from a plain C++ program (g++, no
// HIP headers).  Input file: 16 int8 of the score matrix, int32 gap_open, int32 gap_extend, int32 n, int32 len1, int32 len2,
// then per alignment len1 bytes of seq1 and len2 bytes of seq2.  Output, one line per alignment: score, path length, last
// (i, j), a checksum of the whole path -- from SemiGlobal_affine_mi355x; a final line "batch <mismatches>" compares
// swmi::SemiGlobal_affine_mi355x_batch (pieces of 5 alignments) with it.
#include <cstdio>
#include <fstream>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::array<int8_t, 16> sm{};
    int32_t go = 0, ge = 0, n = 0, len1 = 0, len2 = 0;
    in.read(reinterpret_cast<char *>(sm.data()), 16);
    in.read(reinterpret_cast<char *>(&go), 4);
    in.read(reinterpret_cast<char *>(&ge), 4);
    in.read(reinterpret_cast<char *>(&n), 4);
    in.read(reinterpret_cast<char *>(&len1), 4);
    in.read(reinterpret_cast<char *>(&len2), 4);
    std::vector<std::vector<uint8_t>> s1(n, std::vector<uint8_t>(len1)), s2(n, std::vector<uint8_t>(len2));
    for (int k = 0; k < n; ++k) {
        in.read(reinterpret_cast<char *>(s1[k].data()), len1);
        in.read(reinterpret_cast<char *>(s2[k].data()), len2);
    }
    if (!in) return 3;
    std::vector<std::pair<int, std::vector<std::pair<int, int>>>> one(n);
    for (int k = 0; k < n; ++k) {
        one[k] = SemiGlobal_affine_mi355x(s1[k], s2[k], sm, go, ge);
        unsigned long long sum = 0;
        for (const auto &p : one[k].second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
        const auto &path = one[k].second;
        std::printf("%d %zu %d %d %llu\n", one[k].first, path.size(), path.back().first, path.back().second, sum);
    }
    const auto got = swmi::SemiGlobal_affine_mi355x_batch(s1, s2, sm, go, ge, 3, 5);
    int mismatches = 0;
    for (int k = 0; k < n; ++k) mismatches += got[k] != one[k];
    std::printf("batch %d\n", mismatches);
    return 0;
}
