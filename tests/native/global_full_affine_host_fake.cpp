// global_full_affine_host_fake.cpp -- the host side of the affine global / free-end-gap aligner (swmi_global_full_affine*,
// global_full_affine_api.cpp through the slice pipeline of swmi_table.cpp) on a fake GPU (fake_hip.cpp), plus the stand-in for
// its launcher, which fake_hip.cpp does not know, and which records gap_open, gap_extend and the free_ends mask of every
// launch.  The stand-in follows fake_hip.cpp's table stand-ins: alignment k of a launch reads its index `id` from the first
// (up to) four bytes of its seq1 and writes score 2 id + 1, ends[e] = 8 id + e + 3 (four of them), and with a traceback
// (id >> 20) % (32 move_words + 1) steps and move word w = 0xC0DE << 48 | id << 16 | w in every word of its row; it touches
// the first and last byte of every buffer it is handed, codes included, so that ASan sees a buffer that is too small.  Code
// workspaces take a constant 512 qwords (1024 dwords) per alignment whatever the shape, so at 16384 x 16384 a traceback slice is the
// real 256 alignments while its buffers stay small.
// Built and run by tests/test_global_full_affine_host_fake.py (g++, ASan + UBSan, no GPU).
//
// Host entry, traceback (16384 x 16384: slices of 256) and ends-only, at n = 1, 256, 257 and 640: every score, end and
// count, every move word up to the slice's longest walk and the sentinel past it, one launch per slice alternating between
// two streams, each with the call's open, extend and mask, one 2-D move copy per slice that has a walk, as wide as its longest walk.  Device
// entry on two streams, growing a stream's workspace.  The timer's warm-up call.  The release of the workspaces, and calls
// after it.  A mask of 16, lengths of 0 and 16385, an open of -1 or 128, an extend of 128, NULL buffers and only one of moves /
// steps are refused before anything is launched.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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

// ---- the launcher stand-in ------------------------------------------------------------------------------------------------
struct Launch { size_t n; hipStream_t stream; int len1, len2; bool traceback; unsigned mask; int open, extend; };
static std::mutex g_launch_mu;
static std::vector<Launch> g_launches;

namespace swmi {
size_t global_full_affine_code_qwords(int, int) { return kCodeWords / 2; }
hipError_t launch_global_full_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                     unsigned long long *codes, unsigned long long *moves, uint32_t *steps, size_t move_words,
                                     hipStream_t st)
{
    {
        std::lock_guard<std::mutex> l(g_launch_mu);
        g_launches.push_back({n, st, len1, len2, moves != nullptr, free_ends, gap_open, gap_extend});
    }
    if (n == 0) return hipSuccess;
    CHECK(sm && memcmp(sm, g_sm, 16) == 0);
    volatile uint8_t touch = uint8_t(s1[0] + s1[n * size_t(len1) - 1] + s2[0] + s2[n * size_t(len2) - 1]);
    (void)touch;
    if (moves) {
        CHECK(codes && steps);
        codes[0] = 1;
        codes[n * (kCodeWords / 2) - 1] = 1;
    }
    for (size_t k = 0; k < n; ++k) {
        uint32_t id = 0;
        memcpy(&id, s1 + k * size_t(len1), len1 < 4 ? size_t(len1) : 4);
        scores[k] = int32_t(2 * id + 1);
        for (size_t e = 0; e < 4; ++e) ends[4 * k + e] = int32_t(8 * id + e + 3);
        if (!moves) continue;
        steps[k] = uint32_t((id >> 20) % (32 * move_words + 1));
        for (size_t w = 0; w < move_words; ++w) moves[k * move_words + w] = 0xC0DEull << 48 | uint64_t(id) << 16 | w;
    }
    return hipSuccess;
}
}  // namespace swmi

// ---- the driver -----------------------------------------------------------------------------------------------------------
struct Shape { size_t len1, len2, mw; };
static Shape shape(size_t len1, size_t len2) { return {len1, len2, SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2)}; }

static std::vector<size_t> slices(const Shape &a, size_t n, bool tb)
{
    std::vector<size_t> s(swmi_global_full_affine_slices_for(n, a.len1, a.len2, tb, nullptr, 0));
    swmi_global_full_affine_slices_for(n, a.len1, a.len2, tb, s.data(), s.size());
    return s;
}

static uint32_t walk_of(const Shape &a, uint32_t id) { return uint32_t((id >> 20) % (32 * a.mw + 1)); }
static uint64_t move_word(uint32_t id, size_t w) { return 0xC0DEull << 48 | uint64_t(id) << 16 | w; }

// alignment k of a batch whose slices are `sizes`: index k | walk << 20, the walk bounded per slice by 70 moves, none, and
// the full row in turn (k < 2^20 whenever there is a walk)
static std::vector<uint32_t> indices(const Shape &a, const std::vector<size_t> &sizes, bool tb)
{
    std::vector<uint32_t> id;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bound = i % 3 == 0 ? 70 : i % 3 == 1 ? 0 : 32 * a.mw;
        for (size_t j = 0; j < sizes[i]; ++j) {
            const size_t k = id.size();
            CHECK(!tb || k < (size_t(1) << 20));
            id.push_back(uint32_t(k | (tb ? (k * 7) % (bound + 1) : 0) << 20));
        }
    }
    return id;
}

static void fill_seq1(const Shape &a, const std::vector<uint32_t> &id, uint8_t *s1)
{
    memset(s1, 0, id.size() * a.len1);
    for (size_t k = 0; k < id.size(); ++k) memcpy(s1 + k * a.len1, &id[k], a.len1 < 4 ? a.len1 : 4);
}

// every result of alignment k; move words from `words` on must hold the sentinel (SIZE_MAX: the whole row was written)
static void check_results(const Shape &a, const std::vector<uint32_t> &id, size_t k, const int32_t *scores, const int32_t *ends,
                          const uint64_t *moves, const uint32_t *counts, size_t words)
{
    uint32_t i = 0;
    memcpy(&i, &id[k], a.len1 < 4 ? a.len1 : 4);
    bool ok = scores[k] == int32_t(2 * i + 1);
    for (size_t e = 0; e < 4; ++e) ok = ok && ends[4 * k + e] == int32_t(8 * i + e + 3);
    if (moves) {
        ok = ok && counts[k] == walk_of(a, i);
        for (size_t w = 0; w < a.mw; ++w) ok = ok && moves[k * a.mw + w] == (w < words ? move_word(i, w) : kSentinel);
    }
    if (!ok) {
        fprintf(stderr, "len %zu x %zu: alignment %zu (index %#x, %zu move words copied) has wrong results\n", a.len1, a.len2, k, i, words);
        exit(1);
    }
}

static std::vector<Launch> take_launches()
{
    std::lock_guard<std::mutex> l(g_launch_mu);
    std::vector<Launch> out;
    out.swap(g_launches);
    return out;
}

// the call's gaps, another pair for every mask: open 0 .. 127 and extend 127 .. 7, in either order
static int open_of(unsigned mask) { return int(mask * 8 + (mask == 15 ? 7 : 0)); }
static int extend_of(unsigned mask) { return int(127 - mask * 8); }

static void host_case(const Shape &a, size_t n, bool tb, unsigned mask)
{
    const std::vector<size_t> sizes = slices(a, n, tb);
    const std::vector<uint32_t> id = indices(a, sizes, tb);
    std::vector<uint8_t> s1(n * a.len1), s2(n * a.len2, 0);
    fill_seq1(a, id, s1.data());
    std::vector<int32_t> scores(n, -1), ends(n * 4, -1);
    std::vector<uint64_t> moves(tb ? n * a.mw : 0, kSentinel);
    std::vector<uint32_t> counts(tb ? n : 0, 0);          // (a pipeline that read them before the copy-back saw no walk)
    fake_hip_log_clear();
    take_launches();
    CHECK(swmi_global_full_affine(s1.data(), a.len1, s2.data(), a.len2, n, g_sm, open_of(mask), extend_of(mask), mask, scores.data(),
                                  ends.data(), tb ? moves.data() : nullptr, tb ? counts.data() : nullptr) == SWMI_OK);

    // one launch per slice, alternating between two streams
    const std::vector<Launch> l = take_launches();
    CHECK(l.size() == sizes.size());
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].n == sizes[i] && l[i].traceback == tb && l[i].len1 == int(a.len1) && l[i].len2 == int(a.len2));
        // open, extend and the mask reach the launcher unchanged in every slice
        CHECK(l[i].mask == mask && l[i].open == open_of(mask) && l[i].extend == extend_of(mask));
        if (i >= 1) CHECK(l[i].stream != l[i - 1].stream);
        if (i >= 2) CHECK(l[i].stream == l[i - 2].stream);
    }
    // per slice: the move words its longest walk needs, copied as one 2-D copy of that width (none for no walk), in order
    std::vector<std::string> want_2d, got_2d;
    std::vector<size_t> words(sizes.size(), 0);
    for (size_t i = 0, off = 0; i < sizes.size(); off += sizes[i++]) {
        uint32_t longest = 0;
        for (size_t k = off; k < off + sizes[i]; ++k) longest = walk_of(a, id[k]) > longest ? walk_of(a, id[k]) : longest;
        words[i] = tb ? (longest + 31) / 32 : 0;
        if (words[i]) want_2d.push_back("width" + std::to_string(words[i] * 8) + " height" + std::to_string(sizes[i]));
    }
    for (size_t k = 0; k < fake_hip_log_size(); ++k) {
        const char *m = strstr(fake_hip_log_at(k), "memcpy2d kind2 ");
        if (m) got_2d.push_back(std::string(m + 15).substr(0, std::string(m + 15).find(" stream")));
    }
    CHECK(got_2d == want_2d);
    for (size_t i = 0, off = 0; i < sizes.size(); off += sizes[i++])
        for (size_t k = off; k < off + sizes[i]; ++k)
            check_results(a, id, k, scores.data(), ends.data(), tb ? moves.data() : nullptr, counts.data(), words[i]);
    printf("  host n %7zu %-10s mask %2u: %zu slices, move words per slice", n, tb ? "traceback" : "ends-only", mask, sizes.size());
    for (size_t w : words) printf(" %zu", w);
    printf(": ok\n");
}

// one device-entry call on `st` with buffers of exactly n alignments; returns the log of the call
static std::vector<std::string> device_case(const Shape &a, size_t n, bool tb, hipStream_t st, unsigned mask)
{
    const std::vector<size_t> sizes = slices(a, n, tb);
    const std::vector<uint32_t> id = indices(a, sizes, tb);
    void *s1, *s2, *scores, *ends, *moves = nullptr, *counts = nullptr;
    CHECK(hipMalloc(&s1, n * a.len1) == hipSuccess && hipMalloc(&s2, n * a.len2) == hipSuccess);
    CHECK(hipMalloc(&scores, n * 4) == hipSuccess && hipMalloc(&ends, n * 16) == hipSuccess);
    if (tb) CHECK(hipMalloc(&moves, n * a.mw * 8) == hipSuccess && hipMalloc(&counts, n * 4) == hipSuccess);
    fill_seq1(a, id, static_cast<uint8_t *>(s1));
    memset(s2, 0, n * a.len2);
    fake_hip_log_clear();
    take_launches();
    CHECK(swmi_global_full_affine_device(s1, a.len1, s2, a.len2, n, g_sm, open_of(mask), extend_of(mask), mask, scores, ends, moves,
                                         counts, st) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    CHECK(l.size() == sizes.size());
    for (size_t i = 0; i < l.size(); ++i)
        CHECK(l[i].n == sizes[i] && l[i].stream == st && l[i].traceback == tb && l[i].mask == mask && l[i].open == open_of(mask) &&
              l[i].extend == extend_of(mask));
    for (size_t k = 0; k < n; ++k)      // (the fake's launches write at once; the device entry copies nothing)
        check_results(a, id, k, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(counts), SIZE_MAX);
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) log.push_back(fake_hip_log_at(k));
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    printf("  device n %7zu %-10s mask %2u: %zu slices: ok\n", n, tb ? "traceback" : "ends-only", mask, sizes.size());
    return log;
}

static bool has(const std::vector<std::string> &log, const std::string &line)
{
    for (const std::string &l : log)
        if (l == line) return true;
    return false;
}

static size_t full_slice(const Shape &a, bool tb) { return slices(a, size_t(1) << 24, tb)[0]; }

// the workspace a traceback call of n alignments on a stream needs: one slice's codes
static std::string workspace_malloc(const Shape &a, size_t n)
{
    return "dev0 malloc bytes" + std::to_string(slices(a, n, true)[0] * kCodeWords * 4);
}

int main()
{
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 1 : -1);
    // every argument error and n = 0 come back before any device is touched and before anything is launched, also with
    // buffers that a launch could use
    std::vector<uint8_t> seq(16386, 0);
    int32_t sc1 = 0, e4[4] = {0, 0, 0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        // (pass 0: no device bound; pass 1: after swmi_init)
        uint64_t mv1[2] = {0, 0};
        uint32_t st1 = 0;
        auto host = [&](const uint8_t *s1, size_t len1, const uint8_t *s2, size_t len2, const int8_t *sm, int go, int ge, unsigned mask,
                        int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps) {
            return swmi_global_full_affine(s1, len1, s2, len2, 1, sm, go, ge, mask, scores, ends, moves, steps);
        };
        const uint8_t *q = seq.data();
        CHECK(host(q, 0, q, 5, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 0, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 16385, q, 5, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 16385, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, g_sm, 3, 1, 16, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, g_sm, -1, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(host(q, 5, q, 5, g_sm, 128, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(host(q, 5, q, 5, g_sm, 3, 128, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(host(nullptr, 5, q, 5, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, nullptr, 5, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, nullptr, 3, 1, 0, &sc1, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, g_sm, 3, 1, 0, nullptr, e4, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, g_sm, 3, 1, 0, &sc1, nullptr, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(host(q, 5, q, 5, g_sm, 3, 1, 0, &sc1, e4, mv1, nullptr) == SWMI_ERR_INVALID_ARGUMENT);     // moves without steps
        CHECK(host(q, 5, q, 5, g_sm, 3, 1, 0, &sc1, e4, nullptr, &st1) == SWMI_ERR_INVALID_ARGUMENT);    // steps without moves
        CHECK(swmi_global_full_affine_device(q, 5, q, 5, 1, g_sm, 3, 1, 16, &sc1, e4, nullptr, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(swmi_global_full_affine_device(q, 16385, q, 5, 1, g_sm, 3, 1, 0, &sc1, e4, nullptr, nullptr, nullptr) ==
              SWMI_ERR_INVALID_ARGUMENT);
        CHECK(swmi_global_full_affine_device(q, 5, q, 5, 1, g_sm, 3, 128, 0, &sc1, e4, nullptr, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(swmi_global_full_affine_device(q, 5, q, 5, 1, g_sm, 3, 1, 0, &sc1, e4, mv1, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        float t_ms = 0.f;
        CHECK(swmi_global_full_affine_time_device(q, 5, q, 5, 1, g_sm, 3, 1, 16, &sc1, e4, nullptr, nullptr, nullptr, 2, &t_ms) ==
              SWMI_ERR_INVALID_ARGUMENT);
        CHECK(swmi_global_full_affine_time_device(q, 5, q, 5, 1, g_sm, 128, 1, 0, &sc1, e4, nullptr, nullptr, nullptr, 2, &t_ms) ==
              SWMI_ERR_DOMAIN);
        CHECK(swmi_global_full_affine(nullptr, 5, nullptr, 5, 0, g_sm, 3, 1, 0, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(fake_hip_log_size() == 0 && take_launches().empty());
        if (pass == 0) {
            CHECK(swmi_init(0) == SWMI_OK);
            fake_hip_log_clear();
        }
    }
    printf("  a mask of 16, lengths of 0 and 16385, gaps of -1 and 128, NULL buffers, one of moves / steps: refused, nothing launched\n");
    const Shape tb_a = shape(16384, 16384), eo_a = shape(4, 1);
    CHECK(full_slice(tb_a, true) == 256);
    CHECK(slices(tb_a, 1, true) == std::vector<size_t>({1}) && slices(tb_a, 256, true) == std::vector<size_t>({256}));
    CHECK(slices(tb_a, 257, true) == std::vector<size_t>({256, 1}) && slices(tb_a, 640, true) == std::vector<size_t>({256, 256, 128}));
    CHECK(slices(eo_a, 640, false) == std::vector<size_t>({640}));

    // host entry: n = 1, 256, 257 and 640 (with a traceback: one slice, one slice + 1, two and a half slices), every mask once
    unsigned mask = 0;
    for (const Shape *a : {&tb_a, &eo_a}) {
        const bool tb = a == &tb_a;
        for (size_t n : {size_t(1), size_t(256), size_t(257), size_t(640)}) {
            host_case(*a, n, tb, mask);
            host_case(*a, n, tb, mask + 1);
            mask = (mask + 2) & 15;
        }
    }

    // device entry on two streams; the second call on stream A grows its workspace (after synchronising that stream)
    hipStream_t sa, sb;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    fake_hip_log_clear();
    CHECK(hipStreamSynchronize(sa) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess);
    int ida = 0, idb = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &ida) == 1 && sscanf(fake_hip_log_at(1), "dev0 stream_sync stream%d", &idb) == 1);
    const size_t s = full_slice(tb_a, true), big = 2 * s + s / 2;
    CHECK(big == 640);
    CHECK(has(device_case(tb_a, 3, true, sa, SWMI_ENDS_FIT), workspace_malloc(tb_a, 3)));
    CHECK(has(device_case(tb_a, big, true, sb, SWMI_ENDS_OVERLAP), workspace_malloc(tb_a, big)));
    std::vector<std::string> log = device_case(tb_a, big, true, sa, SWMI_FREE_END1);
    CHECK(log.size() >= 2 && log[0] == "dev0 stream_sync stream" + std::to_string(ida) && log[1] == workspace_malloc(tb_a, big));
    log = device_case(tb_a, 5, true, sb, SWMI_ENDS_GLOBAL);                       // fits: no synchronisation, no allocation
    CHECK(!has(log, "dev0 stream_sync stream" + std::to_string(idb)) && !has(log, workspace_malloc(tb_a, big)));
    log = device_case(eo_a, 7, false, sa, SWMI_FREE_BEGIN1 | SWMI_FREE_END1);                      // ends-only: no workspace, nothing but the launch
    CHECK(log.empty());

    // the timer: one untimed call, then `iters` timed ones (the fake's events are 1 ms apart)
    void *d[6];
    const size_t n = 5;
    const size_t bytes[6] = {n * tb_a.len1, n * tb_a.len2, n * 4, n * 16, n * tb_a.mw * 8, n * 4};
    for (int k = 0; k < 6; ++k) {
        CHECK(hipMalloc(&d[k], bytes[k]) == hipSuccess);
        memset(d[k], 0, bytes[k]);
    }
    float ms = 0.f;
    take_launches();
    CHECK(swmi_global_full_affine_time_device(d[0], tb_a.len1, d[1], tb_a.len2, n, g_sm, 11, 2, SWMI_ENDS_FIT, d[2], d[3], d[4], d[5], sb,
                                              4, &ms) == SWMI_OK);
    const std::vector<Launch> timed = take_launches();
    CHECK(ms == 0.25f && timed.size() == 5);
    for (const Launch &x : timed) CHECK(x.mask == SWMI_ENDS_FIT && x.stream == sb && x.open == 11 && x.extend == 2);
    printf("  timer: 1 + 4 launches, %.2f ms each: ok\n", ms);

    // the release frees the workspaces and the host sets; the next calls allocate them again
    CHECK(swmi_global_full_affine_release_workspaces() == SWMI_OK);
    CHECK(has(device_case(tb_a, 5, true, sb, SWMI_ENDS_OVERLAP), workspace_malloc(tb_a, 5)));
    host_case(tb_a, s + 1, true, SWMI_ENDS_OVERLAP);
    CHECK(swmi_global_full_affine_release_workspaces() == SWMI_OK);
    printf("  release_workspaces, then both entries again: ok\n");

    for (void *p : d) CHECK(hipFree(p) == hipSuccess);
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("global_full_affine host fake ok\n");
    return 0;
}
