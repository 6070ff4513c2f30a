// wide_profile_host_fake.cpp -- the host side of the profile aligners (csrc/wide_api.cpp compiled with
// -DSWMI_WIDE_PROFILE_LIBRARY, the whole host code of libswmi_wide_profile.so) on a fake GPU (fake_hip.cpp), plus the stand-ins
// for what that file takes from wide_profile_kernels.hip -- the launcher, the code size and the wave count -- and hipGetDevice.
// The code workspaces take a constant 512 qwords per alignment, so a traceback slice is a few thousand short alignments.  Built
// and run by tests/test_wide_profile_host_fake.py (g++, ASan + UBSan, a stand-alone program, no GPU).  wide_host_fake.cpp is
// the pattern.
//
// The stand-in launch insists that the profile in "device" memory is the call's in the kernels' layout -- letter-major, 32
// rows of 64 x waves(len2) entries of 16 bytes, byte jj of entry G of row a = profile[(16 G + jj) * 32 + a], and -128 at
// exactly the columns past len2 -- and on the gaps, the mask and the wave count: every slot of two non-zero lengths in a launch
// of waves(len2) wavefronts, every slot with a zero length in a launch of one, which is a launch of its own when waves(len2) >
// 1.  It computes every slot's results from ALL bytes of the sequence the slot names (so ASan sees a slot that points outside
// the buffer): score = 3 len1 + 5 len2 + sum(seq1) + 1000 mask + (sum of the profile's bytes as read from "device" memory) %
// 997, ends[e] = score + e + 1, and with a traceback sum(seq1) % (32 move_words + 1) moves and move word w = 0xC0DE << 48 |
// score << 16 | w in every word of its row; it writes the first and last qword of the slot's codes (none for a slot with a
// zero length).  In a slice (one score buffer) the wave counts come in descending order; len1 never grows inside a launch;
// s2_off is 0.  After a call the driver checks every result at its caller position, that every alignment was launched once,
// and the sentinels behind ends and moves.
//
// Cases: refusals before any device is touched; the host entry, both kinds, at len2 = 1, 17, 1025 and 4096 and at 0 with a
// NULL profile, with a traceback split by the byte budget into at least 3 slices and ends-only split by the count cap into 2;
// the device entry on two streams with DIFFERENT profiles and a growing workspace; the timer; the release, then the host entry
// again.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/swmi_wide_profile.h"
#include "../../smith-waterman-simd_amd/csrc/wide_profile_internal.h"

#define W(name) swmi_wide_profile_##name

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

// ---- what the call under test was given, for the stand-in to insist on ----
static std::vector<int8_t> g_profile;      // len2 * 32
static size_t g_len2 = 0;
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
static size_t g_slots = 0, g_zero_launches = 0;
static bool g_check_order = true;      // off under the timer, whose calls in turn reuse one score buffer

static size_t move_words(size_t a, size_t b) { return SWMI_LOCAL_FULL_MOVE_WORDS(a, b); }
static int waves_of(size_t len2) { return len2 == 0 ? 1 : int((len2 + 1023) / 1024); }

static long profile_sum(const std::vector<int8_t> &p)
{
    long s = 0;
    for (int8_t v : p) s += v;
    return ((s % 997) + 997) % 997;
}

struct Expected {
    int32_t score, ends[4];
    uint32_t steps;
};
static Expected expected(const uint8_t *s1, size_t len1, size_t len2, unsigned mask, long psum)
{
    long sum1 = 0;
    for (size_t x = 0; x < len1; ++x) sum1 += s1[x];
    Expected e;
    e.score = int32_t(3 * len1 + 5 * len2 + sum1 + 1000 * mask + psum);
    for (int x = 0; x < 4; ++x) e.ends[x] = e.score + x + 1;
    e.steps = uint32_t(sum1 % long(32 * move_words(len1, len2) + 1));
    return e;
}

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

namespace swmi {
size_t wide_profile_code_qwords(int, int) { return kCodeQwords; }
int wide_profile_ragged_waves(int len1, int len2) { return len1 == 0 || len2 == 0 ? 1 : (len2 + 1023) / 1024; }

hipError_t launch_wide_profile_ragged(WideKind kind, const uint8_t *s1, const TileWork *work, size_t n, int waves, const void *d_pssm,
                                      int pssm_waves, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                      unsigned long long *codes, unsigned long long *moves, uint32_t *steps, hipStream_t)
{
    CHECK(kind == g_kind && open == g_open && extend == g_extend && free_ends == (g_kind == kWideGlobal ? g_mask : 0u));
    CHECK(n >= 1 && n <= (size_t(1) << 20) && waves >= 1 && waves <= kWideMaxWaves);
    CHECK(pssm_waves == waves_of(g_len2) && d_pssm != nullptr && (reinterpret_cast<uintptr_t>(d_pssm) & 15) == 0);
    CHECK((moves != nullptr) == (codes != nullptr) && (moves != nullptr) == (steps != nullptr));
    // the profile in "device" memory: the call's, transposed, -128 at exactly the columns past len2
    const uint8_t *dp = static_cast<const uint8_t *>(d_pssm);
    const size_t row = size_t(64) * pssm_waves * 16;
    CHECK(wide_profile_device_bytes(g_len2) == 32 * row);
    long psum = 0;
    for (size_t a = 0; a < 32; ++a)
        for (size_t col = 0; col < row; ++col) {
            const uint8_t want = col < g_len2 ? uint8_t(g_profile[col * 32 + a]) : uint8_t(0x80);
            CHECK(dp[a * row + col] == want);
            if (col < g_len2) psum += int8_t(dp[a * row + col]);
        }
    psum = ((psum % 997) + 997) % 997;
    {
        std::lock_guard<std::mutex> l(g_mu);
        // the launches of one slice (one score buffer) come in descending wave count
        if (g_check_order && !g_launches.empty() && g_launches.back().scores == scores) CHECK(g_launches.back().waves > waves);
        g_launches.push_back({scores, waves, n});
        g_slots += n;
        g_zero_launches += waves != pssm_waves;
    }
    uint32_t last_len1 = ~0u;
    for (size_t x = 0; x < n; ++x) {
        const TileWork w = work[x];
        const bool empty = w.len1 == 0 || w.len2 == 0;
        CHECK(w.len2 == g_len2 && w.s2_off == 0 && w.pad == 0);
        CHECK(waves == (empty ? 1 : pssm_waves));                   // W for two non-zero lengths, one wavefront else
        CHECK(w.len1 <= last_len1 && w.len1 <= uint32_t(kWideMaxLen1));
        last_len1 = w.len1;
        // (a slot with a zero length reads no sequence, as the kernel does)
        const Expected e = expected(s1 + w.s1_off, empty ? 0 : w.len1, empty ? 0 : w.len2, free_ends, psum);
        scores[w.k] = e.score;
        for (int y = 0; y < 4; ++y) ends[4 * size_t(w.k) + y] = e.ends[y];
        if (!moves) continue;
        steps[w.k] = e.steps;
        for (size_t y = 0; y < move_words(w.len1, w.len2); ++y) moves[w.move_base + y] = 0xC0DEull << 48 | uint64_t(uint32_t(e.score)) << 16 | y;
        if (!empty) codes[w.code_base] = codes[w.code_base + kCodeQwords - 1] = 1;
    }
    return hipSuccess;
}
}  // namespace swmi

// ---- the driver ----
struct Batch {
    std::vector<uint8_t> s1;
    std::vector<uint64_t> o1{0};
    size_t n() const { return o1.size() - 1; }
    void add(size_t len1, unsigned &seed)
    {
        for (size_t x = 0; x < len1; ++x) s1.push_back(uint8_t((seed = seed * 1664525u + 1013904223u) >> 24));
        o1.push_back(s1.size());
    }
    std::vector<uint64_t> move_offsets(size_t len2) const
    {
        std::vector<uint64_t> mo(n() + 1);
        CHECK(W(move_offsets)(o1.data(), n(), len2, mo.data()) == SWMI_OK);
        for (size_t k = 0; k < n(); ++k) CHECK(mo[k + 1] - mo[k] == move_words(o1[k + 1] - o1[k], len2));
        return mo;
    }
};

static void set_profile(size_t len2, unsigned &seed)
{
    g_len2 = len2;
    g_profile.resize(len2 * 32);
    for (auto &v : g_profile) v = int8_t((seed = seed * 1664525u + 1013904223u) >> 24);
}
static const int8_t *profile_ptr() { return g_len2 ? g_profile.data() : nullptr; }

static void check_results(const Batch &b, const std::vector<uint64_t> &mo, bool tb, const int32_t *sc, const int32_t *en, const uint64_t *mv,
                          const uint32_t *st)
{
    const long psum = profile_sum(g_profile);
    for (size_t k = 0; k < b.n(); ++k) {
        const size_t len1 = b.o1[k + 1] - b.o1[k];
        const bool empty = len1 == 0 || g_len2 == 0;
        const Expected e = expected(b.s1.data() + b.o1[k], empty ? 0 : len1, empty ? 0 : g_len2, g_kind == swmi::kWideGlobal ? g_mask : 0u, psum);
        CHECK(sc[k] == e.score);
        for (int y = 0; y < 4; ++y) CHECK(en[4 * k + y] == e.ends[y]);
        if (!tb) continue;
        CHECK(st[k] == e.steps);
        for (size_t y = 0; y < move_words(len1, g_len2); ++y) CHECK(mv[mo[k] + y] == (0xC0DEull << 48 | uint64_t(uint32_t(e.score)) << 16 | y));
    }
    CHECK(en[4 * b.n()] == kEndSentinel && en[4 * b.n() + 1] == kEndSentinel);
    if (tb) CHECK(mv[mo.back()] == kSentinel);
}

static void host_case(const char *name, const Batch &b, bool tb, size_t min_slices)
{
    const std::vector<uint64_t> mo = b.move_offsets(g_len2);
    std::vector<int32_t> sc(b.n()), en(4 * b.n() + 2, kEndSentinel);
    std::vector<uint64_t> mv(mo.back() + 1, kSentinel);
    std::vector<uint32_t> st(b.n());
    std::vector<size_t> sizes(64);
    const size_t slices = W(slices_for)(b.o1.data(), b.n(), g_len2, tb, sizes.data(), sizes.size());
    CHECK(slices >= min_slices);
    g_launches.clear();
    g_slots = g_zero_launches = 0;
    const uint8_t *s1 = b.s1.empty() ? reinterpret_cast<const uint8_t *>("") : b.s1.data();
    const int rc = g_kind == swmi::kWideLocal
                       ? W(local)(s1, b.o1.data(), b.n(), profile_ptr(), g_len2, g_open, g_extend, sc.data(), en.data(), tb ? mv.data() : nullptr,
                                  tb ? st.data() : nullptr)
                       : W(global)(s1, b.o1.data(), b.n(), profile_ptr(), g_len2, g_open, g_extend, g_mask, sc.data(), en.data(),
                                   tb ? mv.data() : nullptr, tb ? st.data() : nullptr);
    CHECK(rc == SWMI_OK);
    CHECK(g_slots == b.n());
    // as many groups of launches (one score buffer each, the two sets in turn) as slices
    size_t groups = 0, with_zero = 0;
    for (size_t x = 0; x < g_launches.size(); ++x) groups += x == 0 || g_launches[x].scores != g_launches[x - 1].scores;
    CHECK(groups == slices);
    // zero-length slots: a launch of their own per slice that has some, when the others run wider than one wavefront
    for (size_t s = 0, at = 0; s < slices && s < sizes.size(); at += sizes[s], ++s) {
        bool any = false;
        for (size_t k = at; k < at + sizes[s]; ++k) any = any || b.o1[k + 1] == b.o1[k];
        with_zero += any;
    }
    if (waves_of(g_len2) > 1 && slices <= sizes.size()) CHECK(g_zero_launches == with_zero && with_zero >= 1);
    if (waves_of(g_len2) == 1) CHECK(g_zero_launches == 0 && g_launches.size() == slices);
    check_results(b, mo, tb, sc.data(), en.data(), mv.data(), st.data());
    printf("%s, len2 %zu (%zu alignments, %zu slices, %zu launches): ok\n", name, g_len2, b.n(), slices, g_launches.size());
}

struct DeviceBuffers {
    uint8_t *d1 = nullptr;
    int32_t *sc = nullptr, *en = nullptr;
    uint64_t *mv = nullptr;
    uint32_t *st = nullptr;
    void make(const Batch &b, const std::vector<uint64_t> &mo)
    {
        CHECK(hipMalloc(reinterpret_cast<void **>(&d1), b.s1.size() + 16) == hipSuccess);
        CHECK(hipMalloc(reinterpret_cast<void **>(&sc), 4 * b.n()) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&en), 4 * (4 * b.n() + 2)) == hipSuccess);
        CHECK(hipMalloc(reinterpret_cast<void **>(&mv), 8 * (mo.back() + 1)) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&st), 4 * b.n()) == hipSuccess);
        if (!b.s1.empty()) memcpy(d1, b.s1.data(), b.s1.size());
        en[4 * b.n()] = en[4 * b.n() + 1] = kEndSentinel;
        mv[mo.back()] = kSentinel;
    }
    void free_all()
    {
        for (void *p : {(void *)d1, (void *)sc, (void *)en, (void *)mv, (void *)st}) CHECK(hipFree(p) == hipSuccess);
    }
};

static void device_case(const char *name, const Batch &b, bool tb, hipStream_t stream)
{
    const std::vector<uint64_t> mo = b.move_offsets(g_len2);
    DeviceBuffers d;
    d.make(b, mo);
    g_launches.clear();
    g_slots = 0;
    const int rc = g_kind == swmi::kWideLocal
                       ? W(local_device)(d.d1, b.o1.data(), b.n(), profile_ptr(), g_len2, g_open, g_extend, d.sc, d.en, tb ? d.mv : nullptr,
                                         tb ? d.st : nullptr, stream)
                       : W(global_device)(d.d1, b.o1.data(), b.n(), profile_ptr(), g_len2, g_open, g_extend, g_mask, d.sc, d.en,
                                          tb ? d.mv : nullptr, tb ? d.st : nullptr, stream);
    CHECK(rc == SWMI_OK && g_slots == b.n());
    check_results(b, mo, tb, d.sc, d.en, d.mv, d.st);
    float ms = 0.f;
    g_check_order = false;
    CHECK(W(time_device)(g_kind == swmi::kWideLocal ? SWMI_WIDE_PROFILE_LOCAL : SWMI_WIDE_PROFILE_GLOBAL, d.d1, b.o1.data(), b.n(), profile_ptr(),
                         g_len2, g_open, g_extend, g_mask, d.sc, d.en, tb ? d.mv : nullptr, tb ? d.st : nullptr, stream, 2, &ms) == SWMI_OK);
    CHECK(ms == 0.5f && g_slots == 4 * b.n());      // the fake's 1 ms over 2 calls; one untimed call before them
    g_check_order = true;
    check_results(b, mo, tb, d.sc, d.en, d.mv, d.st);
    d.free_all();
    printf("%s, len2 %zu (%zu alignments): ok\n", name, g_len2, b.n());
}

int main()
{
    unsigned seed = 12345;
    // ---- refusals, before any device is touched ----
    {
        set_profile(8, seed);
        const uint64_t good[3] = {0, 3, 8}, dec[3] = {0, 5, 3}, long1[3] = {0, swmi::kWideMaxLen1 + 1, swmi::kWideMaxLen1 + 6};
        uint8_t s[16] = {0};
        int32_t out[16];
        uint64_t mv[8];
        uint32_t st[2];
        const int8_t *p = g_profile.data();
        CHECK(W(local)(s, dec, 2, p, 8, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(global)(s, long1, 2, p, 8, 1, 1, 0, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(local)(s, good, 2, p, SWMI_WIDE_PROFILE_MAX_LEN2 + 1, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(strstr(W(last_error)(), "len2 4097 > 4096") != nullptr);
        CHECK(W(local)(s, good, 2, nullptr, 8, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(strstr(W(last_error)(), "profile is NULL") != nullptr);
        CHECK(W(global)(s, good, 2, p, 8, 1, 1, 16, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(local)(s, good, 2, p, 8, 1, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(W(local)(s, good, 2, p, 8, 128, 1, out, out, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(W(local)(nullptr, nullptr, 0, nullptr, 0, 1, 1, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(g_launches.empty());
        printf("refusals: ok\n");
    }
    Batch mixed;        // zero lengths, the limit, everything between
    for (int k = 0; k < 5200; ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        size_t len1 = r % 301;
        if (k % 211 == 0) len1 = 0;
        if (k == 1000) len1 = 16384;
        mixed.add(len1, seed);
    }
    Batch tiny;         // the count cap
    for (size_t k = 0; k < (size_t(1) << 20) + 5; ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        tiny.add(r % 5, seed);
    }
    Batch small;
    for (int k = 0; k < 700; ++k) {
        const unsigned r = (seed = seed * 1664525u + 1013904223u) >> 8;
        small.add(k % 50 == 7 ? 0 : r % 200, seed);
    }
    // ---- the host entry: the layout's edges (inside one lane, one lane and a column, one wave and a column, everything) ----
    int turn = 0;
    for (size_t len2 : {size_t(1), size_t(17), size_t(1025), size_t(4096)}) {
        for (int kind = 0; kind < 2; ++kind, ++turn) {
            g_kind = kind ? swmi::kWideGlobal : swmi::kWideLocal;
            g_mask = kind ? 10u : 0u;
            g_open = 5 + kind;
            set_profile(len2, seed);
            host_case(kind ? "global host traceback" : "local host traceback", mixed, true, 3);
            if (turn % 3 == 0) host_case(kind ? "global host ends-only" : "local host ends-only", mixed, false, 1);
        }
    }
    // len2 = 0 with a NULL profile: every slot a zero-length one
    g_kind = swmi::kWideGlobal;
    g_mask = 15;
    set_profile(0, seed);
    host_case("global host traceback, no columns", small, true, 1);
    set_profile(3, seed);
    host_case("global host count cap", tiny, false, 2);
    // ---- the device entry on two streams with different profiles: the second stream's workspace is its own, the first
    // ---- one's grows (a wider profile and more slots); every call's launches see that call's profile ----
    hipStream_t a = nullptr, b = nullptr;
    CHECK(hipStreamCreateWithFlags(&a, 0) == hipSuccess && hipStreamCreateWithFlags(&b, 0) == hipSuccess);
    set_profile(17, seed);
    device_case("device small traceback, stream a", small, true, a);
    set_profile(1025, seed);
    device_case("device mixed traceback, stream b", mixed, true, b);
    set_profile(4096, seed);
    device_case("device mixed traceback, stream a (grown)", mixed, true, a);
    set_profile(17, seed);                   // the same length as stream a's first call, other scores
    device_case("device small traceback, stream a (another profile)", small, true, a);
    g_kind = swmi::kWideLocal;
    set_profile(1, seed);
    device_case("device mixed ends-only, stream b", mixed, false, b);
    CHECK(W(release_workspaces)() == SWMI_OK);
    set_profile(1025, seed);
    host_case("local host traceback after the release", small, true, 1);
    CHECK(W(release_workspaces)() == SWMI_OK);
    CHECK(hipStreamDestroy(a) == hipSuccess && hipStreamDestroy(b) == hipSuccess);
    printf("wide profile host fake ok\n");
    return 0;
}
