// wide_host_fake.cpp -- the host side of the wide-alphabet aligners (csrc/wide_api.cpp, the whole host code of libswmi_wide.so
// and, with -DSWMI_WIDE_LONG_LIBRARY on both files, of libswmi_wide_long.so) on a fake GPU (fake_hip.cpp), plus the stand-ins
// for what that file takes from elsewhere: the launchers, code sizes and wave count (wide_affine_kernels.hip,
// wide_long_affine_kernels.hip) and hipGetDevice.  The code workspaces take a constant 512 qwords per alignment, so a
// traceback slice is a few thousand short alignments or a handful of long ones.  Built and run once per library by
// tests/test_wide_host_fake.py (g++, ASan + UBSan, no GPU).
//
// A stand-in launch checks that the matrix in "device" memory, the gaps and the mask are the call's, and computes every slot's
// results from ALL bytes of the sequences the slot names (so ASan sees a slot that points outside the buffers): score = 3 len1
// + 5 len2 + sum(seq1) + 7 sum(seq2) + 1000 mask, ends[e] = score + e + 1, and with a traceback (sum(seq1) + sum(seq2)) %
// (32 move_words + 1) moves and move word w = 0xC0DE << 48 | score << 16 | w in every word of its row; it writes the first and
// last qword of the slot's codes (none for a slot with a zero length).  The UNSTRIPED stand-in insists that no slot is one the
// striped kernels take (len1 > 16384 or len2 > 4096, no zero length), on the wave count and on the library's limits.  The
// STRIPED stand-in, which only the long library's build has, insists on the opposite, that the width is the process's (the
// rule: 4 below 1024 slots, else 1; or what swmi_wide_long_set_stripe_waves set), that the stride is the unit of 2, and it
// writes the first and last int2 of the carry block of every slot of more than 1024 columns (ASan: inside the workspace) and
// checks that the blocks of one launch are disjoint.  In a slice (one score buffer) the striped launch comes first, then the
// wave counts in descending order; len1 never grows inside a launch.  After a call the driver checks every result at its
// caller position, that every alignment was launched once, and the sentinels behind ends and moves.
//
// Cases: refusals before any device is touched; the host entry, both kinds, with a traceback split by the byte budget into at
// least 3 slices and ends-only split by the count cap into 2; in the long build a forced stripe width; the device entry on two
// streams with a growing workspace; the timer; the release, then the host entry again.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../smith-waterman-simd_amd/csrc/wide_long_internal.h"

// ---- what the two builds differ in: the header, the prefix of the entries, the limits, the closing line ----
#ifdef SWMI_WIDE_LONG_LIBRARY
#include "../../include/swmi_wide_long.h"
#define W(name) swmi_wide_long_##name
constexpr bool kLong = true;
constexpr uint32_t kMaxLen1 = swmi::kWideLongMaxLen, kMaxLen2 = swmi::kWideLongMaxLen;
constexpr const char *kDone = "wide long host fake ok";
#else
#include "../../include/swmi_wide.h"
#define W(name) swmi_wide_##name
constexpr bool kLong = false;
constexpr uint32_t kMaxLen1 = swmi::kWideMaxLen1, kMaxLen2 = swmi::kWideMaxLen2;
constexpr const char *kDone = "wide host fake ok";
#endif

#define CHECK(cond)                                                                                                     \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, W(last_error)());      \
            exit(1);                                                                                                    \
        }                                                                                                               \
    } while (0)

constexpr uint64_t kSentinel = 0x5E5E5E5E5E5E5E5Eull;
constexpr int32_t kEndSentinel = 0x5E5E5E5E;
constexpr size_t kCodeQwords = 512;

// ---- what the call under test was given, for the stand-ins to insist on ----
static int8_t g_sm[1024];
static int g_open = 5, g_extend = 2;
static unsigned g_mask = 0;
static swmi::WideKind g_kind = swmi::kWideLocal;

struct Launch {
    const void *scores;
    int waves;
    size_t n;
};
static std::mutex g_mu;
static std::vector<Launch> g_launches;
static size_t g_slots = 0;
static bool g_check_order = true;      // off under the timer, whose calls in turn reuse one score buffer

static size_t move_words(size_t a, size_t b) { return SWMI_LOCAL_LONG_MOVE_WORDS(a, b); }
#ifdef SWMI_WIDE_LONG_LIBRARY
static int g_width = 0;                // what swmi_wide_long_set_stripe_waves was given
static size_t g_striped = 0, g_carried = 0;
#endif

struct Expected {
    int32_t score, ends[4];
    uint32_t steps;
};
static Expected expected(const uint8_t *s1, size_t len1, const uint8_t *s2, size_t len2, unsigned mask)
{
    long sum1 = 0, sum2 = 0;
    for (size_t x = 0; x < len1; ++x) sum1 += s1[x];
    for (size_t x = 0; x < len2; ++x) sum2 += s2[x];
    Expected e;
    e.score = int32_t(3 * len1 + 5 * len2 + sum1 + 7 * sum2 + 1000 * mask);
    for (int x = 0; x < 4; ++x) e.ends[x] = e.score + x + 1;
    e.steps = uint32_t((sum1 + sum2) % long(32 * move_words(len1, len2) + 1));
    return e;
}

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

namespace swmi {
size_t wide_affine_code_qwords(int, int) { return kCodeQwords; }
int wide_ragged_waves(int len1, int len2) { return len1 == 0 || len2 == 0 ? 1 : (len2 + 1023) / 1024; }

// both stand-ins: `waves` = kWideMaxWaves + 1 names the striped launch
static hipError_t fake_launch(WideKind kind, const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves,
                              const int8_t *d_sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                              unsigned long long *codes, unsigned long long *moves, uint32_t *steps)
{
    const bool striped = waves == kWideMaxWaves + 1;
    CHECK(kind == g_kind && open == g_open && extend == g_extend && free_ends == (g_kind == kWideGlobal ? g_mask : 0u));
    CHECK(memcmp(d_sm, g_sm, sizeof g_sm) == 0);
    CHECK(n >= 1 && n <= (size_t(1) << 20) && waves >= 1 && waves <= kWideMaxWaves + 1);
    CHECK((moves != nullptr) == (codes != nullptr) && (moves != nullptr) == (steps != nullptr));
    {
        std::lock_guard<std::mutex> l(g_mu);
        // the launches of one slice (one score buffer) come in descending wave count
        if (g_check_order && !g_launches.empty() && g_launches.back().scores == scores) CHECK(g_launches.back().waves > waves);
        g_launches.push_back({scores, waves, n});
        g_slots += n;
    }
    uint32_t last_len1 = ~0u;
    for (size_t x = 0; x < n; ++x) {
        const TileWork w = work[x];
        CHECK(wide_long_striped(w.len1, w.len2) == striped);
        CHECK(striped || (wide_ragged_waves(int(w.len1), int(w.len2)) == waves && w.pad == 0));
        CHECK(w.len1 <= last_len1 && w.len1 <= kMaxLen1 && w.len2 <= kMaxLen2);
        last_len1 = w.len1;
        const bool empty = w.len1 == 0 || w.len2 == 0;
        // (a slot with a zero length reads neither sequence, as the kernel does)
        const Expected e = expected(s1 + w.s1_off, empty ? 0 : w.len1, s2 + w.s2_off, empty ? 0 : w.len2, free_ends);
        scores[w.k] = e.score;
        for (int y = 0; y < 4; ++y) ends[4 * size_t(w.k) + y] = e.ends[y];
        if (!moves) continue;
        steps[w.k] = e.steps;
        for (size_t y = 0; y < move_words(w.len1, w.len2); ++y) moves[w.move_base + y] = 0xC0DEull << 48 | uint64_t(uint32_t(e.score)) << 16 | y;
        if (!empty) codes[w.code_base] = codes[w.code_base + kCodeQwords - 1] = 1;
    }
    return hipSuccess;
}

hipError_t launch_wide_affine_ragged(WideKind kind, const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves,
                                     const int8_t *d_sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                     unsigned long long *codes, unsigned long long *moves, uint32_t *steps, hipStream_t)
{
    CHECK(waves <= kWideMaxWaves);
    return fake_launch(kind, s1, s2, work, n, waves, d_sm, open, extend, free_ends, scores, ends, codes, moves, steps);
}

#ifdef SWMI_WIDE_LONG_LIBRARY
size_t wide_long_code_qwords(int, int) { return kCodeQwords; }

hipError_t launch_wide_long_affine_ragged(WideKind kind, const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int width,
                                          const int8_t *d_sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                          unsigned long long *codes, unsigned long long *moves, uint32_t *steps, void *d_carry,
                                          uint32_t stride, hipStream_t)
{
    CHECK(width == (g_width ? g_width : n >= 1024 ? 1 : 4) && stride == 2);
    // the carry blocks of the slots of more than 1024 columns: inside the workspace (ASan), disjoint inside the launch
    std::vector<std::pair<size_t, size_t>> blocks;
    int2 *carry = static_cast<int2 *>(d_carry);
    for (size_t x = 0; x < n; ++x) {
        const TileWork w = work[x];
        if (w.len2 <= 1024) {
            CHECK(w.pad == 0);
            continue;
        }
        CHECK(carry != nullptr);
        const size_t at = size_t(w.pad) * stride;
        carry[at] = carry[at + w.len1 - 1] = int2{int(w.k), int(w.len1)};
        blocks.push_back({at, at + w.len1});
    }
    std::sort(blocks.begin(), blocks.end());
    for (size_t x = 1; x < blocks.size(); ++x) CHECK(blocks[x - 1].second <= blocks[x].first);
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_striped += n;
        g_carried += blocks.size();
    }
    return fake_launch(kind, s1, s2, work, n, kWideMaxWaves + 1, d_sm, open, extend, free_ends, scores, ends, codes, moves, steps);
}
#endif
}  // namespace swmi

// ---- the driver ----
struct Batch {
    std::vector<uint8_t> s1, s2;
    std::vector<uint64_t> o1{0}, o2{0}, mo{0};
    size_t n() const { return o1.size() - 1; }
    void add(size_t len1, size_t len2, unsigned &seed)
    {
        for (size_t x = 0; x < len1; ++x) s1.push_back(uint8_t((seed = seed * 1664525u + 1013904223u) >> 24));
        for (size_t x = 0; x < len2; ++x) s2.push_back(uint8_t((seed = seed * 1664525u + 1013904223u) >> 24));
        o1.push_back(s1.size());
        o2.push_back(s2.size());
        mo.push_back(mo.back() + move_words(len1, len2));
    }
};

static void check_results(const Batch &b, bool tb, const int32_t *sc, const int32_t *en, const uint64_t *mv, const uint32_t *st)
{
    for (size_t k = 0; k < b.n(); ++k) {
        const size_t len1 = b.o1[k + 1] - b.o1[k], len2 = b.o2[k + 1] - b.o2[k];
        const bool empty = len1 == 0 || len2 == 0;
        const Expected e = expected(b.s1.data() + b.o1[k], empty ? 0 : len1, b.s2.data() + b.o2[k], empty ? 0 : len2,
                                    g_kind == swmi::kWideGlobal ? g_mask : 0u);
        CHECK(sc[k] == e.score);
        for (int y = 0; y < 4; ++y) CHECK(en[4 * k + y] == e.ends[y]);
        if (!tb) continue;
        CHECK(st[k] == e.steps);
        for (size_t y = 0; y < move_words(len1, len2); ++y) CHECK(mv[b.mo[k] + y] == (0xC0DEull << 48 | uint64_t(uint32_t(e.score)) << 16 | y));
    }
    CHECK(en[4 * b.n()] == kEndSentinel && en[4 * b.n() + 1] == kEndSentinel);
    if (tb) CHECK(mv[b.mo.back()] == kSentinel);
}

static int call_host(const Batch &b, bool tb, int32_t *sc, int32_t *en, uint64_t *mv, uint32_t *st)
{
    const uint8_t *s1 = b.s1.empty() ? reinterpret_cast<const uint8_t *>("") : b.s1.data();
    const uint8_t *s2 = b.s2.empty() ? reinterpret_cast<const uint8_t *>("") : b.s2.data();
    return g_kind == swmi::kWideLocal
               ? W(local)(s1, b.o1.data(), s2, b.o2.data(), b.n(), g_sm, g_open, g_extend, sc, en, tb ? mv : nullptr, tb ? st : nullptr)
               : W(global)(s1, b.o1.data(), s2, b.o2.data(), b.n(), g_sm, g_open, g_extend, g_mask, sc, en, tb ? mv : nullptr,
                                  tb ? st : nullptr);
}

static void host_case(const char *name, const Batch &b, bool tb, size_t min_slices)
{
    std::vector<int32_t> sc(b.n()), en(4 * b.n() + 2, kEndSentinel);
    std::vector<uint64_t> mv(b.mo.back() + 1, kSentinel);
    std::vector<uint32_t> st(b.n());
    std::vector<size_t> sizes(64);
    const size_t slices = W(slices_for)(b.o1.data(), b.o2.data(), b.n(), tb, sizes.data(), sizes.size());
    CHECK(slices >= min_slices);
    g_launches.clear();
    g_slots = 0;
    CHECK(call_host(b, tb, sc.data(), en.data(), mv.data(), st.data()) == SWMI_OK);
    CHECK(g_slots == b.n());
    // as many groups of launches (one score buffer each, the two sets in turn) as slices
    size_t groups = 0;
    for (size_t x = 0; x < g_launches.size(); ++x) groups += x == 0 || g_launches[x].scores != g_launches[x - 1].scores;
    CHECK(groups == slices);
    check_results(b, tb, sc.data(), en.data(), mv.data(), st.data());
    printf("%s (%zu alignments, %zu slices, %zu launches): ok\n", name, b.n(), slices, g_launches.size());
}

static void device_case(const char *name, const Batch &b, bool tb, hipStream_t stream)
{
    uint8_t *d1 = nullptr, *d2 = nullptr;
    int32_t *sc = nullptr, *en = nullptr;
    uint64_t *mv = nullptr;
    uint32_t *st = nullptr;
    CHECK(hipMalloc(reinterpret_cast<void **>(&d1), b.s1.size() + 16) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&d2), b.s2.size() + 16) == hipSuccess);
    CHECK(hipMalloc(reinterpret_cast<void **>(&sc), 4 * b.n()) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&en), 4 * (4 * b.n() + 2)) == hipSuccess);
    CHECK(hipMalloc(reinterpret_cast<void **>(&mv), 8 * (b.mo.back() + 1)) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&st), 4 * b.n()) == hipSuccess);
    if (!b.s1.empty()) memcpy(d1, b.s1.data(), b.s1.size());
    if (!b.s2.empty()) memcpy(d2, b.s2.data(), b.s2.size());
    en[4 * b.n()] = en[4 * b.n() + 1] = kEndSentinel;
    mv[b.mo.back()] = kSentinel;
    g_launches.clear();
    g_slots = 0;
    const int rc = g_kind == swmi::kWideLocal
                       ? W(local_device)(d1, b.o1.data(), d2, b.o2.data(), b.n(), g_sm, g_open, g_extend, sc, en, tb ? mv : nullptr,
                                                tb ? st : nullptr, stream)
                       : W(global_device)(d1, b.o1.data(), d2, b.o2.data(), b.n(), g_sm, g_open, g_extend, g_mask, sc, en,
                                                 tb ? mv : nullptr, tb ? st : nullptr, stream);
    CHECK(rc == SWMI_OK && g_slots == b.n());
    check_results(b, tb, sc, en, mv, st);
    float ms = 0.f;
    g_check_order = false;
    CHECK(W(time_device)(g_kind == swmi::kWideLocal ? SWMI_WIDE_LOCAL : SWMI_WIDE_GLOBAL, d1, b.o1.data(), d2, b.o2.data(), b.n(), g_sm,
                                g_open, g_extend, g_mask, sc, en, tb ? mv : nullptr, tb ? st : nullptr, stream, 2, &ms) == SWMI_OK);
    CHECK(ms == 0.5f && g_slots == 4 * b.n());      // the fake's 1 ms over 2 calls; one untimed call before them
    g_check_order = true;
    for (void *p : {(void *)d1, (void *)d2, (void *)sc, (void *)en, (void *)mv, (void *)st}) CHECK(hipFree(p) == hipSuccess);
    printf("%s (%zu alignments): ok\n", name, b.n());
}

int main()
{
    unsigned seed = 12345;
    // (the long build: |entries| <= 60, so that with the gaps below P = 60 and the global kind's domain rule takes the batch's
    // 65536 x 65536; the short build: every int8, which the rule takes at every shape within its limits)
    for (int x = 0; x < 1024; ++x) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 24;
        g_sm[x] = kLong ? int8_t(int(r % 121) - 60) : int8_t(r);
    }
    // ---- refusals, before any device is touched ----
    {
        const uint64_t good[3] = {0, 3, 8}, dec[3] = {0, 5, 3}, long2[3] = {0, kMaxLen2 + 1, kMaxLen2 + 4}, long1[3] = {0, kMaxLen1 + 1, kMaxLen1 + 6};
        uint8_t s[16] = {0};
        int32_t out[16];
        uint64_t mv[8];
        uint32_t st[2];
        CHECK(W(local)(s, dec, s, good, 2, g_sm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(local)(s, good, s, long2, 2, g_sm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(global)(s, long1, s, good, 2, g_sm, 1, 1, 0, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(global)(s, good, s, good, 2, g_sm, 1, 1, 16, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(local)(s, good, s, good, 2, g_sm, 1, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
#ifdef SWMI_WIDE_LONG_LIBRARY
        // the global kind's domain rule, P = 128: (3, 65534) is outside it -- and the local kind has none (checked below, where it runs)
        const uint64_t edge_out[3] = {0, 65534, 65540};
        int8_t low[1024];
        memset(low, -128, sizeof low);
        CHECK(W(global)(s, good, s, edge_out, 2, low, 1, 1, 0, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(strstr(W(last_error)(), "alignment 0 is outside the domain") != nullptr);
        CHECK(swmi_wide_long_set_stripe_waves(3) == SWMI_ERR_INVALID_ARGUMENT && swmi_wide_long_set_stripe_waves(2) == SWMI_ERR_INVALID_ARGUMENT && swmi_wide_long_set_stripe_waves(0) == SWMI_OK);
#endif
        CHECK(W(local)(s, good, s, good, 2, g_sm, 128, 1, out, out, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(W(local)(nullptr, nullptr, nullptr, nullptr, 0, g_sm, 1, 1, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(g_launches.empty());
        printf("refusals: ok\n");
    }
    // ---- batches: per library the recipe it always had ----
    Batch mixed;        // every wave count, zero lengths, the limits; the long build: striped slots with and without a carry
    for (int k = 0; k < (kLong ? 9000 : 5200); ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        size_t len1 = r % 301, len2 = (r >> 10) % 301;
        if (k % 97 == 0) len2 = 1025 + r % 3072;        // 2 .. 4 wavefronts
        if (kLong && k % 101 == 0) len2 = 4097 + r % 3000;       // striped, with a carry
        if (k % 211 == 0) len1 = 0;
        if (k % 223 == 0) len2 = 0;
        if (k == 1000) len1 = 16384, len2 = 3;
        if (k == 2000) len1 = 7, len2 = 4096;
        if (kLong) {
            if (k == 2500) len1 = 16385, len2 = 3;          // striped because of len1: one stripe, no carry
            if (k == 3000) len1 = 20000, len2 = 1025;       // ... and with one
            if (k == 3500) len1 = 65536, len2 = 0;
            if (k == 4000) len1 = 65536, len2 = 65536;
            if (k == 4500) len1 = 3, len2 = 65536;
        }
        mixed.add(len1, len2, seed);
    }
    Batch tiny;         // the count cap
    for (size_t k = 0; k < (size_t(1) << 20) + 5; ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        tiny.add(r % 5, (r >> 8) % 5, seed);
    }
    Batch small;
    for (int k = 0; k < 700; ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        small.add(r % 200, k % 50 == 0 ? 2048 + r % 2049 : kLong && k % 7 == 0 ? 4097 + r % 2000 : (r >> 10) % 200, seed);
    }
    for (int kind = 0; kind < 2; ++kind) {
        g_kind = kind ? swmi::kWideGlobal : swmi::kWideLocal;
        g_mask = kind ? 10u : 0u;
        g_open = 5 + kind;
#ifdef SWMI_WIDE_LONG_LIBRARY
        g_striped = g_carried = 0;
#endif
        host_case(kind ? "global host traceback" : "local host traceback", mixed, true, 3);
        host_case(kind ? "global host ends-only" : "local host ends-only", mixed, false, 1);
#ifdef SWMI_WIDE_LONG_LIBRARY
        // two calls: every striped alignment went to the striped launcher, every one of more than 1024 columns with a carry block
        size_t striped = 0, carried = 0;
        for (size_t k = 0; k < mixed.n(); ++k) {
            const size_t len1 = mixed.o1[k + 1] - mixed.o1[k], len2 = mixed.o2[k + 1] - mixed.o2[k];
            striped += swmi::wide_long_striped(len1, len2);
            carried += swmi::wide_long_striped(len1, len2) && len2 > 1024;
        }
        CHECK(striped >= 90 && carried >= 88 && carried < striped && g_striped == 2 * striped && g_carried == 2 * carried);
#endif
    }
#ifdef SWMI_WIDE_LONG_LIBRARY
    // a forced width: the striped launches of the 700 of `small` would take the rule's 4 (100 striped slots)
    g_kind = swmi::kWideLocal;
    g_mask = 0;
    g_open = 5;
    for (int w : {1, 4}) {
        CHECK(swmi_wide_long_set_stripe_waves(w) == SWMI_OK);
        g_width = w;
        host_case("local host traceback, forced width", small, true, 1);
    }
    CHECK(swmi_wide_long_set_stripe_waves(0) == SWMI_OK);
    g_width = 0;
#endif
    g_kind = swmi::kWideGlobal;
    g_mask = 15;
    host_case("global host count cap", tiny, false, 2);
    // ---- the device entry on two streams: the second stream's workspace is its own, the first one's grows ----
    hipStream_t a = nullptr, b = nullptr;
    CHECK(hipStreamCreateWithFlags(&a, 0) == hipSuccess && hipStreamCreateWithFlags(&b, 0) == hipSuccess);
    device_case("device small traceback, stream a", small, true, a);
    device_case("device mixed traceback, stream b", mixed, true, b);
    device_case("device mixed traceback, stream a (grown)", mixed, true, a);
    g_kind = swmi::kWideLocal;
    device_case("device mixed ends-only, stream b", mixed, false, b);
    CHECK(W(release_workspaces)() == SWMI_OK);
    host_case("local host traceback after the release", small, true, 1);
    CHECK(W(release_workspaces)() == SWMI_OK);
    CHECK(hipStreamDestroy(a) == hipSuccess && hipStreamDestroy(b) == hipSuccess);
    printf("%s\n", kDone);
    return 0;
}
