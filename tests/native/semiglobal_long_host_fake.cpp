// semiglobal_long_host_fake.cpp -- the host side of the two long semi-global aligners (csrc/semiglobal_long_api.cpp over
// table_api.cpp's bodies and the slice pipeline of swmi_table.cpp) on a fake GPU: fake_hip.cpp, unchanged, for the runtime and the
// fixed-length launchers, fake_semiglobal_long.cpp for the two striped launchers.  The stand-ins write results derived from an
// index in each seq1's first four bytes (k | walk << 20 for alignment k: `walk` is its number of moves, reported as lengths =
// walk + 1), touch the first and last element of every operand and log what each launch was handed.  `linear` or `affine` on the
// command line; built once and run per family by tests/test_semiglobal_long_host_fake.py (g++, ASan + UBSan, no GPU).  Each group
// prints one ": ok" line per case:
//   refusals     lengths of 0 and 65537 on either axis, a NULL matrix, gaps outside their domain, only one of moves / lengths, and
//                the domain rule ((127, -127, 127) and (64, -64, 65) at 65536 x 65536), through the host entry, the device entry
//                and the timer, with code and text, before a device is bound and after; nothing launched
//   domain edge  (64, -64, 64) at 65536 x 65536 is accepted, and launched through the striped launcher with a carry
//   routing      the fixed launcher for (300, 16384) and (16384, 300); the striped one for (16385, 17), carry NULL allowed, and
//                for (64, 16385) with a carry that is non-NULL, 8-byte aligned and sized (the stand-in touches its ends)
//   host entry   traceback at (64, 16385) and ends-only at n = 1, S, S + 1 and 2.5 S: every score, best cell and length, every
//                move word up to the slice's longest walk and the sentinel past it, one launch per slice on two alternating streams
//   device entry two streams, a workspace (codes and carry) that grows only after synchronising its stream
//   timer        1 + iters launches on the caller's stream
//   release      then both entries again, which allocate again
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/swmi.h"

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t);
extern "C" void fake_hip_log_clear();
extern "C" unsigned fake_hip_matrix_sum(const int8_t *sm);
extern "C" size_t fake_semiglobal_long_log_size();
extern "C" const char *fake_semiglobal_long_log_at(size_t);
extern "C" void fake_semiglobal_long_log_clear();

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, swmi_last_error()); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

constexpr uint64_t kSentinel = 0x5E5E5E5E5E5E5E5Eull;
constexpr size_t kCodeWords = 1024;     // the fakes' dwords of codes per alignment
constexpr size_t kStripe = 16384, kMax = SWMI_SEMIGLOBAL_LONG_MAX_LEN;
static int8_t g_sm[16];
static bool g_affine;

struct Shape { size_t len1, len2; };
struct Call { size_t len1, len2; const int8_t *sm; int gap, extend; };
struct Bufs { const void *s1, *s2; size_t n; void *scores, *ends, *moves, *counts; void *stream; int iters; float *ms; };

static int host(const Call &c, const Bufs &b)
{
    const uint8_t *s1 = static_cast<const uint8_t *>(b.s1), *s2 = static_cast<const uint8_t *>(b.s2);
    int32_t *sc = static_cast<int32_t *>(b.scores), *en = static_cast<int32_t *>(b.ends);
    uint64_t *mv = static_cast<uint64_t *>(b.moves);
    uint32_t *ct = static_cast<uint32_t *>(b.counts);
    return g_affine ? swmi_semiglobal_long_affine(s1, c.len1, s2, c.len2, b.n, c.sm, c.gap, c.extend, sc, en, mv, ct)
                    : swmi_semiglobal_long(s1, c.len1, s2, c.len2, b.n, c.sm, int8_t(c.gap), sc, en, mv, ct);
}
static int device(const Call &c, const Bufs &b)
{
    return g_affine ? swmi_semiglobal_long_affine_device(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, b.scores, b.ends, b.moves, b.counts,
                                                    b.stream)
                    : swmi_semiglobal_long_device(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), b.scores, b.ends, b.moves, b.counts, b.stream);
}
static int timer(const Call &c, const Bufs &b)
{
    return g_affine ? swmi_semiglobal_long_affine_time_device(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, b.scores, b.ends, b.moves,
                                                         b.counts, b.stream, b.iters, b.ms)
                    : swmi_semiglobal_long_time_device(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), b.scores, b.ends, b.moves, b.counts,
                                                  b.stream, b.iters, b.ms);
}
static int release() { return g_affine ? swmi_semiglobal_long_affine_release_workspaces() : swmi_semiglobal_long_release_workspaces(); }
static size_t slices_for(size_t n, size_t len1, size_t len2, int tb, size_t *sizes, size_t cap)
{
    return g_affine ? swmi_semiglobal_long_affine_slices_for(n, len1, len2, tb, sizes, cap) : swmi_semiglobal_long_slices_for(n, len1, len2, tb, sizes, cap);
}

static size_t mw_of(const Shape &a) { return SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(a.len1, a.len2); }
static size_t carry_words(const Shape &a) { return a.len2 > kStripe ? a.len1 * (g_affine ? 2 : 1) : 0; }
static Call call_of(const Shape &a, unsigned c)
{
    c &= 15;
    return {a.len1, a.len2, g_sm, int(c) * 8 + (c == 15 ? 7 : 0), g_affine ? 127 - int(c) * 8 : 0};
}
static std::vector<size_t> slices(const Shape &a, size_t n, bool tb)
{
    std::vector<size_t> s(slices_for(n, a.len1, a.len2, tb, nullptr, 0));
    CHECK(slices_for(n, a.len1, a.len2, tb, s.data(), s.size()) == s.size());
    return s;
}
static size_t full_slice(const Shape &a, bool tb) { return slices(a, size_t(1) << 24, tb)[0]; }

static void clear_logs()
{
    fake_hip_log_clear();
    fake_semiglobal_long_log_clear();
}

// ---- the launch logs: fake_hip.cpp's (the fixed-length launchers) and fake_semiglobal_long.cpp's (the striped ones) ----
struct Launch { std::string name; size_t n; int stream, len1, len2, tb; unsigned mask; int gap, extend; unsigned sm; size_t mw; void *carry; };
static void parse(const char *line, std::vector<Launch> *out)
{
    const char *l = strstr(line, " launch_");
    if (!l) return;
    char name[64];
    Launch x{};
    CHECK(sscanf(l, " %63s n%zu stream%d len%dx%d tb%d mask%u gap%d extend%d sm%u mw%zu carry%p", name, &x.n, &x.stream, &x.len1, &x.len2, &x.tb,
                 &x.mask, &x.gap, &x.extend, &x.sm, &x.mw, &x.carry) == 12);
    x.name = name;
    out->push_back(x);
}
static std::vector<Launch> launches()
{
    std::vector<Launch> out;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) parse(fake_hip_log_at(k), &out);
    for (size_t k = 0; k < fake_semiglobal_long_log_size(); ++k) parse(fake_semiglobal_long_log_at(k), &out);
    return out;
}

// what every launch of a call must show: the slice's size, the call's shape, gaps and matrix unchanged, the striped launcher
// exactly where a length exceeds 16384, and a carry exactly where len2 does (NULL or not is free where it is not needed)
static void check_launches(const std::vector<Launch> &l, const std::vector<size_t> &sizes, const Call &c, bool tb)
{
    CHECK(l.size() == sizes.size());
    const bool striped = c.len1 > kStripe || c.len2 > kStripe;
    const std::string want = std::string(striped ? "launch_sgfull_long" : "launch_sgfull") + (g_affine ? "_affine" : "");
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].name == want && l[i].n == sizes[i] && l[i].tb == tb);
        CHECK(l[i].len1 == int(c.len1) && l[i].len2 == int(c.len2) && l[i].mw == SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(c.len1, c.len2));
        CHECK(l[i].mask == 0 && l[i].gap == c.gap && l[i].extend == c.extend && l[i].sm == fake_hip_matrix_sum(c.sm));
        if (c.len2 > kStripe) CHECK(l[i].carry != nullptr && (reinterpret_cast<uintptr_t>(l[i].carry) & 7) == 0);
        if (!striped) CHECK(l[i].carry == nullptr);
    }
}

static uint32_t walk_of(const Shape &a, uint32_t id) { return uint32_t((id >> 20) % (32 * mw_of(a) + 1)); }
static uint64_t move_word(uint32_t id, size_t w) { return 0xC0DEull << 48 | uint64_t(id) << 16 | w; }

static std::vector<uint32_t> indices(const Shape &a, const std::vector<size_t> &sizes, bool tb)
{
    std::vector<uint32_t> id;
    for (size_t i = 0; i < sizes.size(); ++i) {
        const size_t bound = i % 3 == 0 ? 70 : i % 3 == 1 ? 0 : 32 * mw_of(a);
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
static void check_results(const Shape &a, const std::vector<uint32_t> &id, size_t k, const int32_t *scores, const int32_t *ends,
                          const uint64_t *moves, const uint32_t *counts, size_t words)
{
    uint32_t i = 0;
    memcpy(&i, &id[k], a.len1 < 4 ? a.len1 : 4);
    const size_t mw = mw_of(a);
    bool ok = scores[k] == int32_t(2 * i + 1);
    for (size_t e = 0; e < 2; ++e) ok = ok && ends[k * 2 + e] == int32_t(8 * i + e + 3);
    if (moves) {
        ok = ok && counts[k] == walk_of(a, i) + 1;           // lengths = the moves + 1
        for (size_t w = 0; w < mw; ++w) ok = ok && moves[k * mw + w] == (w < words ? move_word(i, w) : kSentinel);
    }
    if (!ok) {
        fprintf(stderr, "len %zu x %zu: alignment %zu (index %#x, %zu move words copied) has wrong results\n", a.len1, a.len2, k, i, words);
        exit(1);
    }
}

static void host_case(const Shape &a, size_t n, bool tb, unsigned c)
{
    const Call call = call_of(a, c);
    const std::vector<size_t> sizes = slices(a, n, tb);
    const std::vector<uint32_t> id = indices(a, sizes, tb);
    const size_t mw = mw_of(a);
    std::vector<uint8_t> s1(n * a.len1), s2(n * a.len2, 0);
    fill_seq1(a, id, s1.data());
    std::vector<int32_t> scores(n, -1), ends(n * 2, -1);
    std::vector<uint64_t> moves(tb ? n * mw : 0, kSentinel);
    std::vector<uint32_t> counts(tb ? n : 0, 0);
    clear_logs();
    CHECK(host(call, {s1.data(), s2.data(), n, scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? counts.data() : nullptr, nullptr, 0,
                      nullptr}) == SWMI_OK);
    const std::vector<Launch> l = launches();
    check_launches(l, sizes, call, tb);
    for (size_t i = 0; i < l.size(); ++i) {
        if (i >= 1) CHECK(l[i].stream != l[i - 1].stream);
        if (i >= 2) CHECK(l[i].stream == l[i - 2].stream);
    }
    // per slice: the move words its longest walk needs, copied back as one 2-D copy of that width (none for no walk), in order
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
    printf("  host   %5zu x %5zu n %7zu %-10s gaps %3d %3d: %zu slices: ok\n", a.len1, a.len2, n, tb ? "traceback" : "ends-only", call.gap,
           call.extend, sizes.size());
}

static size_t workspace_bytes(const Shape &a, size_t n, bool tb)
{
    const size_t m = slices(a, n, tb)[0];
    return (tb ? m * kCodeWords * 4 : 0) + ((m * carry_words(a) * 4 + 15) & ~size_t(15));
}
static std::string workspace_malloc(const Shape &a, size_t n, bool tb) { return "dev0 malloc bytes" + std::to_string(workspace_bytes(a, n, tb)); }
static bool has(const std::vector<std::string> &log, const std::string &line)
{
    for (const std::string &l : log)
        if (l == line) return true;
    return false;
}

// one device-entry call on `st` with buffers of exactly n alignments; returns fake_hip.cpp's log of the call less its launches
static std::vector<std::string> device_case(const Shape &a, size_t n, bool tb, hipStream_t st, int stream_id, unsigned c)
{
    const Call call = call_of(a, c);
    const std::vector<size_t> sizes = slices(a, n, tb);
    const std::vector<uint32_t> id = indices(a, sizes, tb);
    const size_t mw = mw_of(a);
    void *s1, *s2, *scores, *ends, *moves = nullptr, *counts = nullptr;
    CHECK(hipMalloc(&s1, n * a.len1) == hipSuccess && hipMalloc(&s2, n * a.len2) == hipSuccess);
    CHECK(hipMalloc(&scores, n * 4) == hipSuccess && hipMalloc(&ends, n * 8) == hipSuccess);
    if (tb) CHECK(hipMalloc(&moves, n * mw * 8) == hipSuccess && hipMalloc(&counts, n * 4) == hipSuccess);
    fill_seq1(a, id, static_cast<uint8_t *>(s1));
    memset(s2, 0, n * a.len2);
    clear_logs();
    CHECK(device(call, {s1, s2, n, scores, ends, moves, counts, st, 0, nullptr}) == SWMI_OK);
    const std::vector<Launch> l = launches();
    check_launches(l, sizes, call, tb);
    for (const Launch &x : l) CHECK(x.stream == stream_id && x.carry == l[0].carry);
    for (size_t k = 0; k < n; ++k)
        check_results(a, id, k, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(counts), SIZE_MAX);
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k)
        if (!strstr(fake_hip_log_at(k), " launch_")) log.push_back(fake_hip_log_at(k));
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    printf("  device %5zu x %5zu n %7zu %-10s gaps %3d %3d on stream %d: %zu slices: ok\n", a.len1, a.len2, n, tb ? "traceback" : "ends-only",
           call.gap, call.extend, stream_id, sizes.size());
    return log;
}

// ---- refusals ----
static int g_pass;      // 0: no device bound; 1: after swmi_init
static const char *const kNotInit = "swmi_init() has not been called (or failed)";
static void refused(int rc, int code, const std::string &text, int line)
{
    if (rc == code && text == swmi_last_error()) return;
    fprintf(stderr, "line %d, pass %d: got %d \"%s\", expected %d \"%s\"\n", line, g_pass, rc, swmi_last_error(), code, text.c_str());
    exit(1);
}
static std::string lengths_text(size_t len1, size_t len2)
{
    return "lengths (" + std::to_string(len1) + ", " + std::to_string(len2) + ") outside [1, " + std::to_string(kMax) + "]";
}
static std::string gaps_text(int gap, int extend)
{
    if (!g_affine) return "gap_penalty " + std::to_string(gap) + " < 0 is outside the supported domain [0,127]";
    return "gap_open " + std::to_string(gap) + " / gap_extend " + std::to_string(extend) + " outside [0,127]";
}

static void refusals()
{
    std::vector<uint8_t> seq(2 * kMax + 64, 0);
    const uint8_t *s = seq.data() + (16 - (reinterpret_cast<uintptr_t>(seq.data()) & 15)) % 16;     // (the device entries want 16-byte alignment)
    alignas(16) int32_t sc1[4] = {0, 0, 0, 0};
    alignas(16) int32_t e4[4] = {0, 0, 0, 0};         // (two are written)
    float ms = 0.f;
    const Call good{5, 5, g_sm, 3, g_affine ? 2 : 0};
    const Bufs bufs{s, s + kMax + 16, 1, sc1, e4, nullptr, nullptr, nullptr, 2, &ms};
    const int bad = SWMI_ERR_INVALID_ARGUMENT;
    int (*const entries[3])(const Call &, const Bufs &) = {host, device, timer};
    for (int e = 0; e < 3; ++e) {
        const auto args = [&](Call c, int code, const std::string &text, int line) { refused(entries[e](c, bufs), code, text, line); };
        for (const Shape &a : {Shape{0, 5}, Shape{kMax + 1, 5}, Shape{5, 0}, Shape{5, kMax + 1}})
            args({a.len1, a.len2, g_sm, good.gap, good.extend}, bad, lengths_text(a.len1, a.len2), __LINE__);
        Call c = good;
        c.sm = nullptr;
        args(c, bad, "score_matrix is NULL", __LINE__);
        c = good;
        c.gap = -1;
        args(c, SWMI_ERR_DOMAIN, gaps_text(-1, c.extend), __LINE__);
        if (g_affine) {
            c.gap = 128;
            args(c, SWMI_ERR_DOMAIN, gaps_text(128, c.extend), __LINE__);
            c = good;
            c.extend = 128;
            args(c, SWMI_ERR_DOMAIN, gaps_text(c.gap, 128), __LINE__);
        }
        // only one of moves / lengths
        alignas(16) static uint64_t half[8];
        Bufs one = bufs;
        one.moves = half;
        refused(entries[e](good, one), bad, "moves and lengths must both be given (traceback) or both be NULL (ends-only)", __LINE__);
        one.moves = nullptr;
        one.counts = half;
        refused(entries[e](good, one), bad, "moves and lengths must both be given (traceback) or both be NULL (ends-only)", __LINE__);
        // the domain rule: P (len1 + len2) <= 2^23; 64 * 131072 is the edge, and in pass 0 that call then finds no device
        const std::string above = std::string("max(1, |score|, ") + (g_affine ? "gap_open, gap_extend" : "gap") +
                                  ") * (len1 + len2) = P * 131072 above 2^23";
        int8_t sm127[16], sm64[16];
        for (int i = 0; i < 16; ++i) sm127[i] = int8_t(i % 5 == 0 ? 127 : -127), sm64[i] = int8_t(i % 5 == 0 ? 64 : -64);
        args({kMax, kMax, sm127, 127, g_affine ? 127 : 0}, bad, above, __LINE__);
        args({kMax, kMax, sm64, 65, g_affine ? 64 : 0}, bad, above, __LINE__);
        if (g_affine) args({kMax, kMax, sm64, 64, 65}, bad, above, __LINE__);
        sm64[0] = 65;
        args({kMax, kMax, sm64, 64, g_affine ? 64 : 0}, bad, above, __LINE__);
        sm64[0] = 64;
        const Call edge{kMax, kMax, sm64, 64, g_affine ? 64 : 0};
        if (g_pass == 0) refused(entries[e](edge, bufs), SWMI_ERR_NOT_INITIALIZED, kNotInit, __LINE__);
    }
    CHECK(fake_hip_log_size() == 0 && fake_semiglobal_long_log_size() == 0);
}

int main(int argc, char **argv)
{
    CHECK(argc == 2 && (argv[1] == std::string("linear") || argv[1] == std::string("affine")));
    g_affine = argv[1] == std::string("affine");
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 1 : -1);

    for (g_pass = 0; g_pass < 2; ++g_pass) {
        refusals();
        if (g_pass == 0) {
            // slices need no device and know no parameters
            CHECK(slices({kMax, kMax}, 3, true).size() >= 1 && slices_for(3, 0, 5, 1, nullptr, 0) == 0 && slices_for(3, 5, kMax + 1, 1, nullptr, 0) == 0);
            CHECK(swmi_init(0) == SWMI_OK);
            clear_logs();
        }
    }
    printf("  refusals through the host entry, the device entry and the timer, without a device and with one, nothing launched: ok\n");

    // the edge of the domain at 65536 x 65536 is launched (ends-only, one alignment), through the striped launcher with a carry
    {
        std::vector<uint8_t> big(2 * kMax, 0);
        int32_t sc1 = 0, e2[2] = {0, 0};
        int8_t sm64[16];
        for (int i = 0; i < 16; ++i) sm64[i] = int8_t(i % 5 == 0 ? 64 : -64);
        const Call edge{kMax, kMax, sm64, 64, g_affine ? 64 : 0};
        clear_logs();
        CHECK(host(edge, {big.data(), big.data() + kMax, 1, &sc1, e2, nullptr, nullptr, nullptr, 0, nullptr}) == SWMI_OK);
        check_launches(launches(), {1}, edge, false);
        printf("  domain rule: (64, -64, 64) at 65536 x 65536, 64 * 131072 = 2^23, accepted and launched: ok\n");
    }

    // launcher routing, and the carry (check_launches; the striped stand-in touches the carry's first and last dword)
    unsigned c = 0;
    const Shape wide{64, 16385}, tall{16385, 17}, small1{300, 16384}, small2{16384, 300};
    for (const Shape *a : {&small1, &small2, &tall, &wide})
        for (int tb = 1; tb >= 0; --tb) host_case(*a, 7, tb != 0, c++);

    // host entry: n = 1, one slice, one slice + 1, two and a half slices
    const Shape eo{4, 1};
    for (int tb = 1; tb >= 0; --tb) {
        const Shape &a = tb ? wide : eo;
        const size_t s = full_slice(a, tb != 0);
        CHECK(s > 1);
        for (size_t n : {size_t(1), s, s + 1, 2 * s + s / 2}) host_case(a, n, tb != 0, c++);
    }

    // device entry on two streams; the second call on stream A grows its workspace (after synchronising that stream)
    hipStream_t sa, sb;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    clear_logs();
    CHECK(hipStreamSynchronize(sa) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess);
    int ida = 0, idb = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &ida) == 1 && sscanf(fake_hip_log_at(1), "dev0 stream_sync stream%d", &idb) == 1);
    const size_t s = full_slice(wide, true), big = 2 * s + s / 2;
    CHECK(has(device_case(wide, 3, true, sa, ida, c++), workspace_malloc(wide, 3, true)));
    CHECK(has(device_case(wide, big, true, sb, idb, c++), workspace_malloc(wide, big, true)));
    std::vector<std::string> log = device_case(wide, big, true, sa, ida, c++);
    CHECK(log.size() == 2 && log[0] == "dev0 stream_sync stream" + std::to_string(ida) && log[1] == workspace_malloc(wide, big, true));
    CHECK(device_case(wide, 5, true, sb, idb, c++).empty());            // fits: no synchronisation, no allocation
    CHECK(device_case(wide, 7, false, sa, ida, c++).empty());           // ends-only: the carry alone, which fits
    CHECK(device_case(tall, 9, false, sa, ida, c++).empty());           // the striped launcher without a carry: no workspace
    // an ends-only call with a carry on a fresh stream takes a workspace of the carry alone
    hipStream_t sc;
    CHECK(hipStreamCreateWithFlags(&sc, 0) == hipSuccess);
    clear_logs();
    CHECK(hipStreamSynchronize(sc) == hipSuccess);
    int idc = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &idc) == 1);
    log = device_case(wide, 9, false, sc, idc, c++);
    CHECK(workspace_bytes(wide, 9, false) == ((9 * carry_words(wide) * 4 + 15) & ~size_t(15)) && has(log, workspace_malloc(wide, 9, false)));
    CHECK(hipStreamDestroy(sc) == hipSuccess);

    // the timer: one untimed call, then `iters` timed ones (the fake's events are 1 ms apart)
    void *d[6];
    const size_t n = 5, mw = mw_of(wide);
    const size_t bytes[6] = {n * wide.len1, n * wide.len2, n * 4, n * 8, n * mw * 8, n * 4};
    for (int k = 0; k < 6; ++k) {
        CHECK(hipMalloc(&d[k], bytes[k]) == hipSuccess);
        memset(d[k], 0, bytes[k]);
    }
    float ms = 0.f;
    clear_logs();
    const Call timed = call_of(wide, c++);
    CHECK(timer(timed, {d[0], d[1], n, d[2], d[3], d[4], d[5], sb, 4, &ms}) == SWMI_OK);
    const std::vector<Launch> l = launches();
    CHECK(ms == 0.25f && l.size() == 5);
    check_launches(l, std::vector<size_t>(5, n), timed, true);
    for (const Launch &x : l) CHECK(x.stream == idb);
    printf("  timer: 1 + 4 launches on the caller's stream, %.2f ms each: ok\n", ms);

    // the release frees the workspaces and the host sets; the next calls allocate them again
    CHECK(release() == SWMI_OK);
    CHECK(has(device_case(wide, 5, true, sb, idb, c++), workspace_malloc(wide, 5, true)));
    host_case(wide, s + 1, true, c++);
    size_t mallocs = 0;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) mallocs += strstr(fake_hip_log_at(k), " malloc ") != nullptr;
    CHECK(mallocs >= 2 * 7);            // two sets of seq1, seq2, scores, ends, counts, codes (with the carry), moves
    CHECK(release() == SWMI_OK);
    printf("  release_workspaces, then both entries again: ok\n");

    for (void *p : d) CHECK(hipFree(p) == hipSuccess);
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("semiglobal long host fake ok: %s\n", argv[1]);
    return 0;
}
