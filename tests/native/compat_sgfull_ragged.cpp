// compat_sgfull_ragged.cpp -- include/swmi_compat.hpp's ragged semi-global overloads from a plain C++ program (g++, no HIP
// headers).  Input file: int32 n, then per alignment int32 len1, int32 len2, len1 bytes of seq1, len2 bytes of seq2: a batch
// of mixed shapes, some with an empty sequence.  Output, one line per alignment -- score, path length, end cell (i, j), a
// checksum of the whole path -- for two calls in turn, each in pieces of 16 on two threads:
// SemiGlobal_111_mi355x_ragged_batch at (2, -3, 2), then SemiGlobal_affine_mi355x_ragged_batch at (2, -3, 5, 1).  A final line
// "mismatches a" counts: alignments where one piece on one thread differs from the pieces of 16; non-empty alignments where the
// per-pair overloads SemiGlobal_long_mi355x / SemiGlobal_affine_mi355x differ from the batch; alignments with an empty sequence
// whose result is not (0, {(0, 0)}); paths that do not start at (0, 0); and 1 if SemiGlobal_affine_mi355x_batch no longer throws
// on differing lengths.
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
        std::printf("%d %zu %d %d %llu\n", one.first, path.size(), path.back().first, path.back().second, sum);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2 || swmi_init(0) != SWMI_OK) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    Batch m1, m2;
    if (!read_batch(in, m1, m2)) return 3;
    const std::array<int8_t, 16> k23 = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};
    const Results::value_type empty{0, {{0, 0}}};
    int bad = 0;
    for (int affine = 0; affine < 2; ++affine) {
        const Results r = affine ? swmi::SemiGlobal_affine_mi355x_ragged_batch(m1, m2, k23, 5, 1, 16, 2)
                                 : swmi::SemiGlobal_111_mi355x_ragged_batch(m1, m2, k23, 2, 16, 2);
        if (r.size() != m1.size()) return 4;
        print(r);
        const Results whole = affine ? swmi::SemiGlobal_affine_mi355x_ragged_batch(m1, m2, k23, 5, 1, m1.size(), 1)
                                     : swmi::SemiGlobal_111_mi355x_ragged_batch(m1, m2, k23, 2, m1.size(), 1);
        for (size_t k = 0; k < m1.size(); ++k) {
            bad += whole[k] != r[k];
            bad += r[k].second.empty() || r[k].second.front() != std::pair<int, int>(0, 0);
            if (m1[k].empty() || m2[k].empty())
                bad += r[k] != empty;
            else
                bad += (affine ? SemiGlobal_affine_mi355x(m1[k], m2[k], k23, 5, 1) : SemiGlobal_long_mi355x(m1[k], m2[k], k23, 2)) != r[k];
        }
    }
    try {
        swmi::SemiGlobal_affine_mi355x_batch(m1, m2, k23, 5, 1);
        ++bad;
    } catch (const std::invalid_argument &) {
    }
    std::printf("mismatches %d\n", bad);
    return 0;
}
