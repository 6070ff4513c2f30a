// compat_banded_long_fake.cpp -- TEST ONLY: include/swmi_banded_long_compat.hpp run without a device, as a stand-alone program
// under ASan + UBSan: the two overloads over the real host source (csrc/banded_ragged_api.cpp with -DSWMI_BANDED_LONG_LIBRARY)
// on the fake GPU of fake_hip.cpp.  This file holds the stand-in for the launcher, hipGetDevice, and plain stand-ins for the two
// functions the header takes from libswmi.so (swmi_last_error, swmi_local_long_expand_moves: the expander as swmi.h states it);
// the move layout is the library's own export.  The launcher's stand-in gives every slot a result made from the slot and the
// first byte of its seq1, which the driver sets to the alignment's index in the batch: score = 100000 tag + len1 + len2 + d0 +
// band + 7 free_ends + 50000000 kind, the end cell (len1, len2), min(len1, len2) diagonal steps.  So a result in the wrong place,
// a piece staged wrongly, a wrong move offset or a path expanded from the wrong row shows.  The batch holds lengths on both
// sides of 16384 and one of 65536.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "swmi_banded_long_compat.hpp"
#include "../../smith-waterman-simd_amd/csrc/banded_internal.h"

using swmi::banded::RaggedSlot;

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

// ---- the two functions of libswmi.so that the header calls ----
extern "C" const char *swmi_last_error(void) { return "stand-in"; }

// positions: steps + 1 pairs (i, j) from the start cell to the end cell; step t at bits 2 (t % 32) of word t / 32, in walking
// order from the end cell: 3 = diagonal, 2 = up, 1 = left
extern "C" int swmi_local_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                                            size_t cap)
{
    if (cap < size_t(steps) + 1) return SWMI_ERR_INVALID_ARGUMENT;
    int32_t i = end_i, j = end_j;
    for (uint32_t t = 0;; ++t) {
        positions[2 * (steps - t)] = i;
        positions[2 * (steps - t) + 1] = j;
        if (t == steps) break;
        const unsigned dir = unsigned(moves[t / 32] >> (2 * (t % 32))) & 3u;
        if (dir == 0) return SWMI_ERR_INVALID_ARGUMENT;
        i -= dir != 1;
        j -= dir != 2;
    }
    return SWMI_OK;
}

namespace {

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

int g_failed = 0;
int g_band = 0;                       // the band of the overload call that is running
size_t g_launches = 0, g_largest = 0;

int expected_score(size_t tag, size_t len1, size_t len2, int d0, int band, unsigned free_ends, int kind)
{
    return int(100000 * tag + len1 + len2) + d0 + band + 7 * int(free_ends) + 50000000 * kind;
}

}  // namespace

hipError_t swmi::banded::launch_banded_long(int kind, int band, const uint8_t *s1, const uint8_t *, const RaggedSlot *slots, size_t n,
                                            const int8_t *, int, int, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes,
                                            unsigned long long *moves, uint32_t *steps, hipStream_t)
{
    EXPECT(band == g_band && moves && steps && codes);                           // the overloads always ask for a traceback
    ++g_launches;
    g_largest = std::max(g_largest, n);
    for (size_t x = 0; x < n; ++x) {
        const RaggedSlot &q = slots[x];
        const size_t tag = q.len1 ? s1[q.off1] : 0;
        const uint32_t st = uint32_t(std::min(q.len1, q.len2));
        scores[q.index] = expected_score(tag, size_t(q.len1), size_t(q.len2), q.d0, band, free_ends, kind);
        ends[4 * q.index] = q.len1, ends[4 * q.index + 1] = q.len2;
        ends[4 * q.index + 2] = q.len1 - int32_t(st), ends[4 * q.index + 3] = q.len2 - int32_t(st);
        steps[q.index] = st;
        for (uint32_t t = 0; t < st; ++t) {
            if (t % 32 == 0) moves[q.move_off + t / 32] = 0;
            moves[q.move_off + t / 32] |= 3ull << (2 * (t % 32));
        }
    }
    return hipSuccess;
}

namespace {

using Seqs = std::vector<std::vector<uint8_t>>;
const std::array<int8_t, 16> kSm = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};

std::vector<std::pair<int, std::vector<std::pair<int, int>>>> run(int kind, const Seqs &a, const Seqs &b, const std::vector<int32_t> &d, int band,
                                                                 int open, unsigned fe, size_t piece)
{
    g_band = band;
    return kind ? swmi::NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch(a, b, d, band, kSm, open, 1, fe, piece, 2)
                : swmi::SmithWaterman_banded_long_affine_mi355x_ragged_batch(a, b, d, band, kSm, open, 1, piece, 2);
}

void check(const char *name, int kind, const Seqs &a, const Seqs &b, const std::vector<int32_t> &d, int band, unsigned fe, size_t piece)
{
    g_launches = g_largest = 0;
    const auto res = run(kind, a, b, d, band, 5, fe, piece);
    EXPECT(res.size() == a.size());
    const size_t per = piece ? piece : 4096;                                         // (piece 0 counts as 4096)
    EXPECT(g_launches == (a.size() + per - 1) / per && g_largest <= per);            // one C call, one slice, a piece
    for (size_t k = 0; k < res.size(); ++k) {
        const size_t len1 = a[k].size(), len2 = b[k].size(), st = std::min(len1, len2);
        const int d0 = d.empty() ? 0 : std::max(-131072, std::min(131072, d[k]));
        EXPECT(res[k].first == expected_score(len1 ? k : 0, len1, len2, d0, band, kind ? fe : 0u, kind));
        const auto &path = res[k].second;
        EXPECT(path.size() == st + 1);
        if (path.size() != st + 1) break;
        EXPECT(path.back() == std::make_pair(int(len1), int(len2)) && path.front() == std::make_pair(int(len1 - st), int(len2 - st)));
        for (size_t t = 1; t < path.size(); ++t) EXPECT(path[t].first == path[t - 1].first + 1 && path[t].second == path[t - 1].second + 1);
    }
    std::printf("%s: %s\n", name, g_failed ? "FAILED" : "ok");
}

template <class E, class F> bool throws(F f, const char *needle)
{
    try {
        f();
    } catch (const E &e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    } catch (...) {
    }
    return false;
}

}  // namespace

int main()
{
    // nine alignments, seq1's first byte the index: lengths on both sides of 16384, the longest, an empty side, both empty
    const size_t lens[9][2] = {{40, 50}, {16385, 16384}, {0, 7}, {65536, 65536}, {33, 33}, {9, 0}, {0, 0}, {17000, 300}, {64, 40000}};
    Seqs a, b;
    std::vector<int32_t> d;
    for (size_t k = 0; k < 9; ++k) {
        a.emplace_back(lens[k][0], uint8_t(3));
        b.emplace_back(lens[k][1], uint8_t(1));
        if (!a[k].empty()) a[k][0] = uint8_t(k);
        d.push_back(int32_t(k) * 37 - 150);
    }
    d[7] = 65536 + 300;                                  // reaches the launcher as it is
    d[8] = 2147483647;                                   // ... as 131072
    check("local, three pieces of 3", 0, a, b, d, 256, 0u, 3);
    check("global, three pieces of 4", 1, a, b, d, 1024, 10u, 4);
    check("global, no diagonals, one piece", 1, a, b, {}, 512, 19u, 0);
    {
        Seqs e(5), f;
        for (size_t k = 0; k < 5; ++k) f.emplace_back(3 + k, uint8_t(2));
        check("every seq1 empty", 1, e, f, {}, 128, 3u, 2);
        EXPECT(run(0, {}, {}, {}, 256, 5, 0u, 3).empty());
    }
    // the refusals reach the caller as exceptions: the library's with its text (the band before the gaps), the header's own and
    // the layout's as std::invalid_argument
    g_launches = 0;
    EXPECT(throws<std::runtime_error>([&] { run(0, a, b, d, 192, 200, 0u, 3); }, "band 192 is not one of"));
    EXPECT(throws<std::runtime_error>([&] { run(0, a, b, d, 256, 200, 0u, 3); }, "outside [0,127]"));
    EXPECT(throws<std::runtime_error>([&] { run(1, a, b, d, 256, 5, 20u, 3); }, "NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch: "));
    EXPECT(throws<std::invalid_argument>([&] { run(0, a, b, std::vector<int32_t>(10), 256, 5, 0u, 3); }, "diagonals"));
    EXPECT(throws<std::invalid_argument>([&] { run(0, a, Seqs(8), d, 256, 5, 0u, 3); }, "differ in length"));
    {
        Seqs big(1, std::vector<uint8_t>(65537, 1)), one(1, std::vector<uint8_t>(4, 1));
        EXPECT(throws<std::invalid_argument>([&] { run(0, big, one, {}, 256, 5, 0u, 3); }, "a length above 65536"));
    }
    EXPECT(g_launches == 0);
    std::printf("refusals: %s\n", g_failed ? "FAILED" : "ok");
    EXPECT(swmi_banded_long_release_workspaces() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("banded long compat fake ok\n");
    return 0;
}
