// compat_wide_long.cpp -- include/swmi_wide_long_compat.hpp's overloads from a plain C++ program (g++, no HIP headers, no swmi_init: the
// long wide library runs on the current device).  Input file: 1024 int8 of matrix, int32 n, then per alignment int32 len1, int32
// len2, len1 bytes of seq1, len2 bytes of seq2: a batch of mixed shapes, some with an empty sequence.  Output, one line per
// alignment -- score, path length, first (i, j), last (i, j), a checksum of the whole path -- for three calls in turn, each
// in pieces of 8 on two threads, at gaps (7, 2): SmithWaterman_wide_long_affine_mi355x_ragged_batch, then
// NeedlemanWunsch_wide_long_affine_mi355x_ragged_batch under SWMI_ENDS_GLOBAL and under SWMI_ENDS_FIT.  A final line "mismatches a"
// counts the alignments where one piece on one thread differs from the pieces of 8, and 1 if a seq2 of 65537 letters does
// not throw with the long wide library's text.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "swmi_wide_long_compat.hpp"

using Batch = std::vector<std::vector<uint8_t>>;
using Results = std::vector<std::pair<int, std::vector<std::pair<int, int>>>>;

static bool read_batch(std::ifstream &in, std::array<int8_t, 1024> &sm, Batch &s1, Batch &s2)
{
    in.read(reinterpret_cast<char *>(sm.data()), 1024);
    int32_t n = 0;
    in.read(reinterpret_cast<char *>(&n), 4);
    s1.resize(n);
    s2.resize(n);
    for (int k = 0; k < n; ++k) {
        int32_t len[2] = {0, 0};
        in.read(reinterpret_cast<char *>(len), 8);
        s1[k].resize(len[0]);
        s2[k].resize(len[1]);
        in.read(reinterpret_cast<char *>(s1[k].data()), len[0]);
        in.read(reinterpret_cast<char *>(s2[k].data()), len[1]);
    }
    return bool(in);
}

static void print(const Results &r)
{
    for (const auto &one : r) {
        unsigned long long sum = 0;
        for (const auto &p : one.second) sum = sum * 1000003ull + (unsigned long long)p.first * 32771ull + (unsigned long long)p.second;
        const auto &path = one.second;
        std::printf("%d %zu %d %d %d %d %llu\n", one.first, path.size(), path.front().first, path.front().second, path.back().first,
                    path.back().second, sum);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::array<int8_t, 1024> sm;
    Batch m1, m2;
    if (!read_batch(in, sm, m1, m2)) return 3;
    int bad = 0;
    for (int call = 0; call < 3; ++call) {
        const unsigned mask = call == 2 ? SWMI_ENDS_FIT : SWMI_ENDS_GLOBAL;
        auto run = [&](size_t piece, unsigned threads) {
            return call == 0 ? swmi::SmithWaterman_wide_long_affine_mi355x_ragged_batch(m1, m2, sm, 7, 2, piece, threads)
                             : swmi::NeedlemanWunsch_wide_long_affine_mi355x_ragged_batch(m1, m2, sm, 7, 2, mask, piece, threads);
        };
        const Results r = run(8, 2);
        if (r.size() != m1.size()) return 4;
        print(r);
        const Results whole = run(m1.size(), 1);
        for (size_t k = 0; k < m1.size(); ++k) bad += whole[k] != r[k];
    }
    try {
        swmi::SmithWaterman_wide_long_affine_mi355x_ragged_batch({std::vector<uint8_t>(3)}, {std::vector<uint8_t>(65537)}, sm, 7, 2);
        ++bad;
    } catch (const std::runtime_error &e) {
        bad += std::strstr(e.what(), "65537 > 65536") == nullptr;
    }
    std::printf("mismatches %d\n", bad);
    return 0;
}
