// compat_wide_profile.cpp -- include/swmi_wide_profile_compat.hpp's overloads from a plain C++ program (g++, no HIP headers,
// no swmi_init: the library runs on the current device).  Input file: int32 len2, 32 len2 int8 of profile (position-major),
// int32 n, then per sequence int32 len1 and len1 bytes: a batch of mixed lengths, some empty.  Output, one line per alignment
// -- score, path length, first (i, j), last (i, j), a checksum of the whole path -- for three calls in turn, each in pieces of
// 16 on two threads, at gaps (7, 2): SmithWaterman_wide_profile_mi355x_batch, then NeedlemanWunsch_wide_profile_mi355x_batch
// under SWMI_ENDS_GLOBAL and under SWMI_ENDS_FIT.  A final line "mismatches a" counts the alignments where one piece on one
// thread differs from the pieces of 16, 1 if a profile of 4097 columns does not throw with the library's text, and 1 if a
// profile of 33 scores does not throw.
#include <cstdio>
#include <cstring>
#include <fstream>

#include "swmi_wide_profile_compat.hpp"

using Batch = std::vector<std::vector<uint8_t>>;
using Results = std::vector<std::pair<int, std::vector<std::pair<int, int>>>>;

static bool read_batch(std::ifstream &in, std::vector<int8_t> &profile, Batch &s1)
{
    int32_t len2 = 0, n = 0;
    in.read(reinterpret_cast<char *>(&len2), 4);
    profile.resize(size_t(len2) * 32);
    in.read(reinterpret_cast<char *>(profile.data()), profile.size());
    in.read(reinterpret_cast<char *>(&n), 4);
    s1.resize(n);
    for (int k = 0; k < n; ++k) {
        int32_t len = 0;
        in.read(reinterpret_cast<char *>(&len), 4);
        s1[k].resize(len);
        in.read(reinterpret_cast<char *>(s1[k].data()), len);
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
    std::vector<int8_t> profile;
    Batch m1;
    if (!read_batch(in, profile, m1)) return 3;
    int bad = 0;
    for (int call = 0; call < 3; ++call) {
        const unsigned mask = call == 2 ? SWMI_ENDS_FIT : SWMI_ENDS_GLOBAL;
        auto run = [&](size_t piece, unsigned threads) {
            return call == 0 ? swmi::SmithWaterman_wide_profile_mi355x_batch(m1, profile, 7, 2, piece, threads)
                             : swmi::NeedlemanWunsch_wide_profile_mi355x_batch(m1, profile, 7, 2, mask, piece, threads);
        };
        const Results r = run(16, 2);
        if (r.size() != m1.size()) return 4;
        print(r);
        const Results whole = run(m1.size(), 1);
        for (size_t k = 0; k < m1.size(); ++k) bad += whole[k] != r[k];
    }
    try {
        swmi::SmithWaterman_wide_profile_mi355x_batch({std::vector<uint8_t>(3)}, std::vector<int8_t>(4097 * 32), 7, 2);
        ++bad;
    } catch (const std::runtime_error &e) {
        bad += std::strstr(e.what(), "4097 > 4096") == nullptr;
    }
    try {
        swmi::NeedlemanWunsch_wide_profile_mi355x_batch({std::vector<uint8_t>(3)}, std::vector<int8_t>(33), 7, 2);
        ++bad;
    } catch (const std::invalid_argument &) {
    }
    std::printf("mismatches %d\n", bad);
    return 0;
}
