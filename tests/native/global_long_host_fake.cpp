// global_long_host_fake.cpp -- the host side of the long global / fit / overlap aligners (swmi_global_long*,
// swmi_global_long_affine*: global_long_api.cpp and global_long_affine_api.cpp through the slice pipeline of swmi_table.cpp) on
// a fake GPU (fake_hip.cpp), plus stand-ins for the four launchers they name, which record every launch: its size, stream,
// shape, mask, gaps and CARRY pointer.  A stand-in writes score 2 id + 1, ends[e] = 8 id + e + 3 and, with a traceback, id % 97
// steps and move word 0xC0DE << 48 | id << 16 | w, where id is the alignment's index from the first four bytes of its seq1;
// it touches the first and last byte of every buffer it is handed, the codes and the carry (len1 dwords per alignment, 2 len1
// with affine gaps) included, so that ASan sees a buffer that is too small.  Code workspaces take a constant 1024 dwords
// (512 qwords) per alignment whatever the shape, so the slices are short and the buffers small.
// Built and run by tests/test_global_long_host_fake.py (g++, ASan + UBSan, no GPU).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/swmi.h"
#include "../../smith-waterman-simd_amd/csrc/swmi_internal.h"

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t);
extern "C" void fake_hip_log_clear();

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, swmi_last_error()); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

constexpr uint64_t kSentinel = 0x5E5E5E5E5E5E5E5Eull;
constexpr size_t kCodeWords = 1024;
static int8_t g_sm[16];
static bool g_any_params = false;

struct Launch { size_t n; hipStream_t stream; int len1, len2; bool traceback, affine, striped; unsigned mask; const int32_t *carry; };
static std::mutex g_launch_mu;
static std::vector<Launch> g_launches;

static hipError_t stand_in(bool affine, bool striped, const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm,
                           int gap_a, int gap_b, unsigned mask, int32_t *scores, int32_t *ends, uint32_t *codes,
                           unsigned long long *moves, uint32_t *steps, size_t move_words, int32_t *carry, hipStream_t st)
{
    {
        std::lock_guard<std::mutex> l(g_launch_mu);
        g_launches.push_back({n, st, len1, len2, moves != nullptr, affine, striped, mask, carry});
    }
    if (n == 0) return hipSuccess;
    CHECK(sm && (g_any_params || (memcmp(sm, g_sm, 16) == 0 && gap_a == (affine ? 3 : 1) && gap_b == (affine ? 2 : 0))));
    CHECK(move_words == SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2));
    volatile uint8_t touch = uint8_t(s1[0] + s1[n * size_t(len1) - 1] + s2[0] + s2[n * size_t(len2) - 1]);
    (void)touch;
    if (striped && len2 > SWMI_GLOBAL_FULL_MAX_LEN) {
        CHECK(carry && (reinterpret_cast<uintptr_t>(carry) & 7) == 0);
        carry[0] = 1;
        carry[n * size_t(len1) * (affine ? 2 : 1) - 1] = 1;
    }
    if (moves) {
        CHECK(codes && steps);
        codes[0] = 1;
        codes[n * kCodeWords - 1] = 1;
    }
    for (size_t k = 0; k < n; ++k) {
        uint32_t id = 0;
        memcpy(&id, s1 + k * size_t(len1), 4);
        scores[k] = int32_t(2 * id + 1);
        for (size_t e = 0; e < 4; ++e) ends[4 * k + e] = int32_t(8 * id + e + 3);
        if (!moves) continue;
        steps[k] = id % 97;
        for (size_t w = 0; w < move_words; ++w) moves[k * move_words + w] = 0xC0DEull << 48 | uint64_t(id) << 16 | w;
    }
    return hipSuccess;
}

namespace swmi {
size_t global_full_code_words(int, int) { return kCodeWords; }
size_t global_long_code_words(int, int) { return kCodeWords; }
size_t global_full_affine_code_qwords(int, int) { return kCodeWords / 2; }
size_t global_long_affine_code_qwords(int, int) { return kCodeWords / 2; }
hipError_t launch_global_full(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, unsigned fe,
                              int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw,
                              hipStream_t st)
{
    return stand_in(false, false, s1, s2, len1, len2, n, sm, gap, 0, fe, scores, ends, codes, moves, steps, mw, nullptr, st);
}
hipError_t launch_global_long(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, unsigned fe,
                              int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw,
                              int32_t *carry, hipStream_t st)
{
    return stand_in(false, true, s1, s2, len1, len2, n, sm, gap, 0, fe, scores, ends, codes, moves, steps, mw, carry, st);
}
hipError_t launch_global_full_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                     unsigned fe, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                                     uint32_t *steps, size_t mw, hipStream_t st)
{
    return stand_in(true, false, s1, s2, len1, len2, n, sm, go, ge, fe, scores, ends, reinterpret_cast<uint32_t *>(codes), moves, steps, mw,
                    nullptr, st);
}
hipError_t launch_global_long_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                     unsigned fe, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                                     uint32_t *steps, size_t mw, int32_t *carry, hipStream_t st)
{
    return stand_in(true, true, s1, s2, len1, len2, n, sm, go, ge, fe, scores, ends, reinterpret_cast<uint32_t *>(codes), moves, steps, mw,
                    carry, st);
}
}  // namespace swmi

static std::vector<Launch> take_launches()
{
    std::lock_guard<std::mutex> l(g_launch_mu);
    std::vector<Launch> out;
    out.swap(g_launches);
    return out;
}

struct Shape { size_t len1, len2, mw; };
static Shape shape(size_t len1, size_t len2) { return {len1, len2, SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2)}; }

static std::vector<size_t> slices(bool affine, const Shape &a, size_t n, bool tb)
{
    auto f = affine ? swmi_global_long_affine_slices_for : swmi_global_long_slices_for;
    std::vector<size_t> s(f(n, a.len1, a.len2, tb, nullptr, 0));
    f(n, a.len1, a.len2, tb, s.data(), s.size());
    return s;
}

static int call_host(bool affine, const Shape &a, const uint8_t *s1, const uint8_t *s2, size_t n, unsigned mask, int32_t *sc, int32_t *ends,
                     uint64_t *mv, uint32_t *st)
{
    return affine ? swmi_global_long_affine(s1, a.len1, s2, a.len2, n, g_sm, 3, 2, mask, sc, ends, mv, st)
                  : swmi_global_long(s1, a.len1, s2, a.len2, n, g_sm, 1, mask, sc, ends, mv, st);
}

static int call_device(bool affine, const Shape &a, const void *s1, const void *s2, size_t n, unsigned mask, void *sc, void *ends, void *mv,
                       void *st, hipStream_t stream)
{
    return affine ? swmi_global_long_affine_device(s1, a.len1, s2, a.len2, n, g_sm, 3, 2, mask, sc, ends, mv, st, stream)
                  : swmi_global_long_device(s1, a.len1, s2, a.len2, n, g_sm, 1, mask, sc, ends, mv, st, stream);
}

static void check_results(const Shape &a, size_t n, const int32_t *scores, const int32_t *ends, const uint64_t *moves, const uint32_t *counts)
{
    for (size_t k = 0; k < n; ++k) {
        const uint32_t id = uint32_t(k + 5);
        bool ok = scores[k] == int32_t(2 * id + 1);
        for (size_t e = 0; e < 4; ++e) ok = ok && ends[4 * k + e] == int32_t(8 * id + e + 3);
        if (moves) {
            ok = ok && counts[k] == id % 97;
            for (size_t w = 0; w < (counts[k] + 31) / 32; ++w) ok = ok && moves[k * a.mw + w] == (0xC0DEull << 48 | uint64_t(id) << 16 | w);
        }
        if (!ok) {
            fprintf(stderr, "len %zu x %zu: alignment %zu has wrong results\n", a.len1, a.len2, k);
            exit(1);
        }
    }
}

static void fill(const Shape &a, size_t n, uint8_t *s1)
{
    memset(s1, 0, n * a.len1);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t id = uint32_t(k + 5);
        memcpy(s1 + k * a.len1, &id, 4);
    }
}

// what every launch of a call must show: the slice's size, the call's shape, mask and family, the striped launcher exactly
// where a length exceeds 16384, and a carry exactly where len2 does
static void check_launches(const std::vector<Launch> &l, const std::vector<size_t> &sizes, bool affine, const Shape &a, bool tb, unsigned mask)
{
    CHECK(l.size() == sizes.size());
    const bool striped = a.len1 > SWMI_GLOBAL_FULL_MAX_LEN || a.len2 > SWMI_GLOBAL_FULL_MAX_LEN;
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].n == sizes[i] && l[i].traceback == tb && l[i].affine == affine && l[i].mask == mask);
        CHECK(l[i].len1 == int(a.len1) && l[i].len2 == int(a.len2) && l[i].striped == striped);
        CHECK((l[i].carry != nullptr) == (a.len2 > SWMI_GLOBAL_FULL_MAX_LEN));
    }
}

static void host_case(bool affine, const Shape &a, size_t n, bool tb, unsigned mask)
{
    const std::vector<size_t> sizes = slices(affine, a, n, tb);
    std::vector<uint8_t> s1(n * a.len1), s2(n * a.len2, 0);
    fill(a, n, s1.data());
    std::vector<int32_t> scores(n, -1), ends(n * 4, -1);
    std::vector<uint64_t> moves(tb ? n * a.mw : 0, kSentinel);
    std::vector<uint32_t> counts(tb ? n : 0, 0);
    take_launches();
    CHECK(call_host(affine, a, s1.data(), s2.data(), n, mask, scores.data(), ends.data(), tb ? moves.data() : nullptr,
                    tb ? counts.data() : nullptr) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    check_launches(l, sizes, affine, a, tb, mask);
    for (size_t i = 1; i < l.size(); ++i) CHECK(l[i].stream != l[i - 1].stream);       // two sets of buffers, alternating
    check_results(a, n, scores.data(), ends.data(), tb ? moves.data() : nullptr, counts.data());
    printf("  %s host   %5zu x %5zu n %3zu %-10s mask %2u: %zu slices: ok\n", affine ? "affine" : "linear", a.len1, a.len2, n,
           tb ? "traceback" : "ends-only", mask, sizes.size());
}

static bool has(const std::vector<std::string> &log, const std::string &line)
{
    for (const std::string &l : log)
        if (l == line) return true;
    return false;
}

// one device-entry call on a fresh stream: the workspace holds one slice's codes (with a traceback) and one slice's carry
static void device_case(bool affine, const Shape &a, size_t n, bool tb, unsigned mask)
{
    const std::vector<size_t> sizes = slices(affine, a, n, tb);
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, 0) == hipSuccess);
    void *s1, *s2, *scores, *ends, *moves = nullptr, *counts = nullptr;
    CHECK(hipMalloc(&s1, n * a.len1) == hipSuccess && hipMalloc(&s2, n * a.len2) == hipSuccess);
    CHECK(hipMalloc(&scores, n * 4) == hipSuccess && hipMalloc(&ends, n * 16) == hipSuccess);
    if (tb) CHECK(hipMalloc(&moves, n * a.mw * 8) == hipSuccess && hipMalloc(&counts, n * 4) == hipSuccess);
    fill(a, n, static_cast<uint8_t *>(s1));
    memset(s2, 0, n * a.len2);
    fake_hip_log_clear();
    take_launches();
    CHECK(call_device(affine, a, s1, s2, n, mask, scores, ends, moves, counts, st) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    check_launches(l, sizes, affine, a, tb, mask);
    for (const Launch &x : l) CHECK(x.stream == st && x.carry == l[0].carry);
    check_results(a, n, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                  static_cast<uint32_t *>(counts));
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) log.push_back(fake_hip_log_at(k));
    const size_t carry_words = a.len2 > SWMI_GLOBAL_FULL_MAX_LEN ? a.len1 * (affine ? 2 : 1) : 0;
    const size_t want = (tb ? sizes[0] * kCodeWords * 4 : 0) + ((sizes[0] * carry_words * 4 + 15) & ~size_t(15));
    if (want) CHECK(has(log, "dev0 malloc bytes" + std::to_string(want)));
    else CHECK(log.empty());
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    CHECK(hipStreamDestroy(st) == hipSuccess);
    printf("  %s device %5zu x %5zu n %3zu %-10s mask %2u: %zu slices, workspace %zu bytes: ok\n", affine ? "affine" : "linear", a.len1,
           a.len2, n, tb ? "traceback" : "ends-only", mask, sizes.size(), want);
}

int main()
{
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 1 : -1);
    int8_t sm64[16], sm65[16], sm128[16];
    for (int i = 0; i < 16; ++i) {
        sm64[i] = int8_t(i % 5 == 0 ? 64 : -64);
        sm65[i] = int8_t(i % 5 == 0 ? 64 : -65);
        sm128[i] = int8_t(i % 5 == 0 ? 1 : -128);
    }
    // every argument error and n = 0 come back before any device is touched and before anything is launched, also with
    // buffers that a launch could use
    std::vector<uint8_t> seq(65538, 0);
    int32_t sc1 = 0, e4[4] = {0, 0, 0, 0};
    uint64_t mv1[4200];
    uint32_t st1 = 0;
    const int bad = SWMI_ERR_INVALID_ARGUMENT;
    for (int pass = 0; pass < 2; ++pass) {
        // (pass 0: no device bound; pass 1: after swmi_init)
        const uint8_t *s = seq.data();
        CHECK(swmi_global_long(s, 0, s, 5, 1, g_sm, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 0, 1, g_sm, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 65537, s, 5, 1, g_sm, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 65537, 1, g_sm, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 5, 1, g_sm, 1, 16, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 5, 1, nullptr, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 5, 1, g_sm, -1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(swmi_global_long(s, 5, s, 5, 1, g_sm, 1, 0, &sc1, e4, mv1, nullptr) == bad);
        CHECK(swmi_global_long(s, 5, s, 5, 1, g_sm, 1, 0, &sc1, e4, nullptr, &st1) == bad);
        CHECK(swmi_global_long(s, 5, s, 5, 1, g_sm, 1, 0, nullptr, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(nullptr, 5, s, 5, 1, g_sm, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        // the domain rule, P (len1 + len2) <= 2^23, on both sides of its edge
        CHECK(swmi_global_long(s, 32769, s, 32768, 1, sm128, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 65536, s, 65536, 1, sm65, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long(s, 65536, s, 65536, 1, sm64, 65, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine(s, 65536, s, 65536, 1, sm64, 64, 65, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine(s, 65536, s, 65536, 1, sm64, 65, 1, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine(s, 65537, s, 5, 1, g_sm, 3, 2, 0, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine(s, 5, s, 5, 1, g_sm, 3, 2, 16, &sc1, e4, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine(s, 5, s, 5, 1, g_sm, 128, 2, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(swmi_global_long_device(s, 5, s, 5, 1, g_sm, 1, 16, &sc1, e4, nullptr, nullptr, nullptr) == bad);
        CHECK(swmi_global_long_affine_device(s, 65537, s, 5, 1, g_sm, 3, 2, 0, &sc1, e4, nullptr, nullptr, nullptr) == bad);
        float t_ms = 0.f;
        CHECK(swmi_global_long_time_device(s, 5, s, 5, 1, g_sm, 1, 16, &sc1, e4, nullptr, nullptr, nullptr, 2, &t_ms) == bad);
        CHECK(swmi_global_long_affine_time_device(s, 5, s, 65537, 1, g_sm, 3, 2, 0, &sc1, e4, nullptr, nullptr, nullptr, 2, &t_ms) == bad);
        CHECK(swmi_global_long(nullptr, 5, nullptr, 5, 0, g_sm, 1, 0, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(swmi_global_long_affine(nullptr, 5, nullptr, 5, 0, g_sm, 3, 2, 0, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(fake_hip_log_size() == 0 && take_launches().empty());
        if (pass == 0) {
            CHECK(swmi_init(0) == SWMI_OK);
            fake_hip_log_clear();
        }
    }
    printf("  lengths of 0 and 65537, a mask of 16, NULLs, one of moves / steps, calls outside the domain rule: refused, nothing launched\n");

    // the edge of the domain rule from inside: accepted, and launched (the stand-in is told to expect other parameters)
    {
        std::vector<uint8_t> big(2 * 65536 + 1, 0);
        g_any_params = true;
        take_launches();
        CHECK(swmi_global_long(big.data(), 65536, big.data() + 65536, 65536, 1, sm64, 64, 0, &sc1, e4, nullptr, nullptr) == SWMI_OK);
        CHECK(swmi_global_long_affine(big.data(), 65536, big.data() + 65536, 65536, 1, sm64, 64, 64, 0, &sc1, e4, nullptr, nullptr) == SWMI_OK);
        CHECK(swmi_global_long(big.data(), 32768, big.data() + 65536, 32768, 1, sm128, 127, 0, &sc1, e4, nullptr, nullptr) == SWMI_OK);
        CHECK(take_launches().size() == 3);
        g_any_params = false;
        printf("  (65536, 65536) with P = 64 and (32768, 32768) with P = 128: accepted\n");
    }

    const Shape full = shape(65536, 65536), wide = shape(40, 16385), tall = shape(16385, 40), small = shape(300, 16384);
    unsigned mask = 0;
    for (int affine = 0; affine < 2; ++affine) {
        const size_t s = slices(affine, full, 1000, true)[0];
        CHECK(s >= 2 && s < 100);
        // n across a slice boundary: one slice, one more, two and a half
        for (size_t n : {s, s + 1, 2 * s + s / 2}) host_case(affine, full, n, true, mask++ & 15);
        host_case(affine, full, 3, false, mask++ & 15);
        host_case(affine, wide, 7, true, mask++ & 15);
        host_case(affine, wide, 7, false, mask++ & 15);
        host_case(affine, tall, 7, true, mask++ & 15);          // the striped launcher, no carry
        host_case(affine, small, 7, true, mask++ & 15);         // the fixed-length launcher
        device_case(affine, full, s + 1, true, mask++ & 15);
        device_case(affine, wide, 9, false, mask++ & 15);       // ends-only with a carry: a workspace of the carry alone
        device_case(affine, tall, 9, false, mask++ & 15);       // ends-only without: nothing but the launch
        device_case(affine, small, 9, true, mask++ & 15);
    }
    CHECK(swmi_global_long_release_workspaces() == SWMI_OK && swmi_global_long_affine_release_workspaces() == SWMI_OK);
    host_case(0, wide, 3, true, SWMI_ENDS_OVERLAP);
    host_case(1, wide, 3, true, SWMI_ENDS_FIT);
    printf("  release_workspaces, then both host entries again: ok\n");
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("global_long host fake ok\n");
    return 0;
}
