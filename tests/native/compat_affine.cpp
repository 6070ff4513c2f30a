// compat_affine.cpp -- include/swmi_compat.hpp's affine local-alignment overloads from a plain C++ program (g++, no HIP
// headers).  Input file: 16 int8 of the score matrix, int32 gap_open, int32 gap_extend, int32 n, then per alignment int32 len1,
// len1 bytes of seq1, 128 bytes of seq2.  Output, one line per alignment: score, path length, first (i, j), last (i, j), a
// checksum of the whole path -- from SmithWaterman_affine_mi355x; a final line "batch <mismatches>" compares
// swmi::SmithWaterman_affine_mi355x_batch (per run of equal lengths, small pieces) with it.
#include <cstdio>
#include <fstream>

#include "swmi_compat.hpp"

int main(int argc, char **argv)
{
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::array<int8_t, 16> sm{};
    int32_t go = 0, ge = 0, n = 0;
    in.read(reinterpret_cast<char *>(sm.data()), 16);
    in.read(reinterpret_cast<char *>(&go), 4);
    in.read(reinterpret_cast<char *>(&ge), 4);
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
    std::vector<std::pair<int, std::vector<std::pair<int, int>>>> one(n);
    for (int k = 0; k < n; ++k) {
        one[k] = SmithWaterman_affine_mi355x(s1[k], s2[k], sm, go, ge);
        unsigned long long sum = 0;
        for (const auto &p : one[k].second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
        const auto &path = one[k].second;
        std::printf("%d %zu %d %d %d %d %llu\n", one[k].first, path.size(), path.front().first, path.front().second,
                    path.back().first, path.back().second, sum);
    }
    int mismatches = 0;
    for (int lo = 0; lo < n;) {
        int hi = lo;
        while (hi < n && s1[hi].size() == s1[lo].size()) ++hi;
        const std::vector<std::vector<uint8_t>> a(s1.begin() + lo, s1.begin() + hi);
        const std::vector<std::array<uint8_t, 128>> b(s2.begin() + lo, s2.begin() + hi);
        const auto got = swmi::SmithWaterman_affine_mi355x_batch(a, b, sm, go, ge, 3);
        for (int k = lo; k < hi; ++k) mismatches += got[k - lo] != one[k];
        lo = hi;
    }
    std::printf("batch %d\n", mismatches);
    return 0;
}
