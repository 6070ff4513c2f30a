// compat_banded_long.cpp -- TEST ONLY: swmi::SmithWaterman_banded_long_affine_mi355x_ragged_batch and
// swmi::NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch (include/swmi_banded_long_compat.hpp) on the inputs a test
// wrote: <dir>/a.bin and b.bin (the sequences back to back), o1.bin and o2.bin (n + 1 uint64 offsets each), d.bin (n int32).
// Arguments: dir n kind band match mismatch open extend free_ends (kind 0 = local, 1 = global).  Prints one line per alignment:
// score end_i end_j start_i start_j positions i0 j0 i1 j1 ... (the ends are the path's last and first position); pieces of 3
// alignments, so that more than one piece runs.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "swmi_banded_long_compat.hpp"

template <class T> static std::vector<T> slurp(const std::string &path, size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), std::streamsize(count * sizeof(T)));
    if (!f && count) {
        std::fprintf(stderr, "cannot read %s\n", path.c_str());
        std::exit(2);
    }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    const std::string dir = argv[1];
    const size_t n = std::strtoul(argv[2], nullptr, 10);
    const int kind = std::atoi(argv[3]), band = std::atoi(argv[4]), match = std::atoi(argv[5]), mismatch = std::atoi(argv[6]),
              open = std::atoi(argv[7]), extend = std::atoi(argv[8]);
    const unsigned free_ends = unsigned(std::strtoul(argv[9], nullptr, 10));
    const auto o1 = slurp<uint64_t>(dir + "/o1.bin", n + 1), o2 = slurp<uint64_t>(dir + "/o2.bin", n + 1);
    const auto a = slurp<uint8_t>(dir + "/a.bin", o1[n]), b = slurp<uint8_t>(dir + "/b.bin", o2[n]);
    const auto d = slurp<int32_t>(dir + "/d.bin", n);
    std::vector<std::vector<uint8_t>> s1(n), s2(n);
    for (size_t k = 0; k < n; ++k) {
        s1[k].assign(a.begin() + o1[k], a.begin() + o1[k + 1]);
        s2[k].assign(b.begin() + o2[k], b.begin() + o2[k + 1]);
    }
    std::array<int8_t, 16> sm;
    for (int x = 0; x < 16; ++x) sm[x] = int8_t(x / 4 == x % 4 ? match : mismatch);
    auto run = [&](const std::vector<int32_t> &diag, int width, int go, unsigned fe) {
        return kind ? swmi::NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch(s1, s2, diag, width, sm, go, extend, fe, 3, 2)
                    : swmi::SmithWaterman_banded_long_affine_mi355x_ragged_batch(s1, s2, diag, width, sm, go, extend, 3, 2);
    };
    try {
        const auto res = run(d, band, open, free_ends);
        for (const auto &r : res) {
            std::printf("%d %d %d %d %d %zu", r.first, r.second.back().first, r.second.back().second, r.second.front().first,
                        r.second.front().second, r.second.size());
            for (const auto &p : r.second) std::printf(" %d %d", p.first, p.second);
            std::printf("\n");
        }
        // the refusals reach the caller as exceptions with the library's text: the band before the gaps
        try {
            (void)run(d, 192, 200, free_ends);
            return 3;
        } catch (const std::runtime_error &e) {
            if (std::string(e.what()).find("band 192") == std::string::npos) return 4;
        }
        try {
            (void)run(d, band, 200, free_ends);
            return 5;
        } catch (const std::runtime_error &e) {
            if (std::string(e.what()).find("outside [0,127]") == std::string::npos) return 6;
        }
        try {
            (void)run(std::vector<int32_t>(n + 1), band, open, free_ends);
            return 7;
        } catch (const std::invalid_argument &) {
        }
        return run(std::vector<int32_t>(), band, open, free_ends).size() == n ? 0 : 8;        // no diagonals: the main one for all
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
