// compat_banded_global.cpp -- TEST ONLY: swmi::NeedlemanWunsch_banded_affine_mi355x_batch (include/swmi_banded_global_compat.hpp)
// on the inputs a test wrote: <dir>/a.bin (n x len1 bytes), b.bin (n x len2), d.bin (n int32).  Arguments: dir n len1 len2
// match mismatch open extend free_ends.  Prints one line per alignment: score end_i end_j start_i start_j positions i0 j0 i1 j1
// ... (the ends are the path's last and first position); pieces of 2 alignments, so that more than one piece runs.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "swmi_banded_global_compat.hpp"

template <class T> static std::vector<T> slurp(const std::string &path, size_t count)
{
    std::vector<T> v(count);
    std::ifstream f(path, std::ios::binary);
    f.read(reinterpret_cast<char *>(v.data()), std::streamsize(count * sizeof(T)));
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path.c_str());
        std::exit(2);
    }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    const std::string dir = argv[1];
    const size_t n = std::strtoul(argv[2], nullptr, 10), len1 = std::strtoul(argv[3], nullptr, 10), len2 = std::strtoul(argv[4], nullptr, 10);
    const int match = std::atoi(argv[5]), mismatch = std::atoi(argv[6]), open = std::atoi(argv[7]), extend = std::atoi(argv[8]);
    const unsigned free_ends = unsigned(std::strtoul(argv[9], nullptr, 10));
    const auto a = slurp<uint8_t>(dir + "/a.bin", n * len1), b = slurp<uint8_t>(dir + "/b.bin", n * len2);
    const auto d = slurp<int32_t>(dir + "/d.bin", n);
    std::vector<std::vector<uint8_t>> s1(n), s2(n);
    for (size_t k = 0; k < n; ++k) {
        s1[k].assign(a.begin() + k * len1, a.begin() + (k + 1) * len1);
        s2[k].assign(b.begin() + k * len2, b.begin() + (k + 1) * len2);
    }
    std::array<int8_t, 16> sm;
    for (int x = 0; x < 16; ++x) sm[x] = int8_t(x / 4 == x % 4 ? match : mismatch);
    try {
        const auto res = swmi::NeedlemanWunsch_banded_affine_mi355x_batch(s1, s2, d, sm, open, extend, free_ends, 2, 2);
        for (const auto &r : res) {
            std::printf("%d %d %d %d %d %zu", r.first, r.second.back().first, r.second.back().second, r.second.front().first,
                        r.second.front().second, r.second.size());
            for (const auto &p : r.second) std::printf(" %d %d", p.first, p.second);
            std::printf("\n");
        }
        // the refusals reach the caller as exceptions with the library's text
        try {
            (void)swmi::NeedlemanWunsch_banded_affine_mi355x_batch(s1, s2, d, sm, 200, extend, free_ends);
            return 3;
        } catch (const std::runtime_error &e) {
            if (std::string(e.what()).find("outside [0,127]") == std::string::npos) return 4;
        }
        try {
            (void)swmi::NeedlemanWunsch_banded_affine_mi355x_batch(s1, s2, d, sm, open, extend, SWMI_BANDED_END_ANYWHERE | SWMI_FREE_END1);
            return 5;
        } catch (const std::runtime_error &e) {
            if (std::string(e.what()).find("free_ends 20") == std::string::npos) return 6;
        }
        try {
            (void)swmi::NeedlemanWunsch_banded_affine_mi355x_batch(s1, s2, std::vector<int32_t>(n + 1), sm, open, extend);
            return 7;
        } catch (const std::invalid_argument &) {
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
