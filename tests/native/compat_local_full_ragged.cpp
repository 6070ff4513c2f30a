// compat_local_full_ragged.cpp -- include/swmi_compat.hpp's ragged any-length overloads from a plain C++ program (g++, no HIP
// headers).  Input file: two batches, each int32 n, then per alignment int32 len1, int32 len2, len1 bytes of seq1, len2 bytes
// of seq2: fixture F7 and a batch of mixed shapes.  Output, one line per alignment -- score, path length, first (i, j), last
// (i, j), a checksum of the whole path -- for four calls in turn: F7 through SmithWaterman_long_mi355x_ragged_batch at
// (1, -1, 1) in ONE piece, F7 through SmithWaterman_long_affine_mi355x_ragged_batch at open = extend = 1, the mixed batch
// through the linear overload at (2, -3, 2) in pieces of 16, and through the affine one at (2, -3, 5, 1).  A final line
// "mismatches a" counts: F7 alignments where pieces of 7 on one thread differ from the one piece; mixed alignments where the
// one-call overloads SmithWaterman_long_mi355x / SmithWaterman_long_affine_mi355x (neither length 0) differ from the batch;
// and 1 each if a fixed-shape _batch overload no longer throws on differing lengths.
#include <cstdio>
#include <fstream>

#include "swmi_compat.hpp"

using Batch = std::vector<std::vector<uint8_t>>;
using Results = std::vector<std::pair<int, std::vector<std::pair<int, int>>>>;

static bool read_batch(std::ifstream &in, Batch &s1, Batch &s2)
{
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
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    Batch f1, f2, m1, m2;
    if (!read_batch(in, f1, f2) || !read_batch(in, m1, m2)) return 3;
    const std::array<int8_t, 16> k111 = {1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1};
    const std::array<int8_t, 16> k23 = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};
    const Results f_lin = swmi::SmithWaterman_long_mi355x_ragged_batch(f1, f2, k111, 1, f1.size());
    const Results f_aff = swmi::SmithWaterman_long_affine_mi355x_ragged_batch(f1, f2, k111, 1, 1, f1.size());
    const Results m_lin = swmi::SmithWaterman_long_mi355x_ragged_batch(m1, m2, k23, 2, 16, 2);
    const Results m_aff = swmi::SmithWaterman_long_affine_mi355x_ragged_batch(m1, m2, k23, 5, 1, 16, 2);
    if (f_lin.size() != f1.size() || f_aff.size() != f1.size() || m_lin.size() != m1.size() || m_aff.size() != m1.size()) return 4;
    print(f_lin);
    print(f_aff);
    print(m_lin);
    print(m_aff);
    int bad = 0;
    const Results f_pieces = swmi::SmithWaterman_long_mi355x_ragged_batch(f1, f2, k111, 1, 7, 1);
    for (size_t k = 0; k < f1.size(); ++k) bad += f_pieces[k] != f_lin[k];
    for (size_t k = 0; k < m1.size(); ++k) {
        if (m1[k].empty() || m2[k].empty()) {
            bad += m_lin[k] != m_aff[k] || m_lin[k].first != 0 || m_lin[k].second.size() != 1;
            continue;
        }
        bad += SmithWaterman_long_mi355x(m1[k], m2[k], k23, 2) != m_lin[k];
        bad += SmithWaterman_long_affine_mi355x(m1[k], m2[k], k23, 5, 1) != m_aff[k];
    }
    try {
        swmi::SmithWaterman_long_mi355x_batch(m1, m2, k23, 2);
        ++bad;
    } catch (const std::invalid_argument &) {
    }
    try {
        swmi::SmithWaterman_long_affine_mi355x_batch(m1, m2, k23, 5, 1);
        ++bad;
    } catch (const std::invalid_argument &) {
    }
    std::printf("mismatches %d\n", bad);
    return 0;
}
