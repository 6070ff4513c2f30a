// table_host_fake.cpp -- the host side of the fourteen fixed-shape table aligners (table_api.cpp through the slice pipeline of
// swmi_table.cpp) on a fake GPU (fake_hip.cpp), whose launcher stand-ins write results derived from an index in each seq1's
// first four bytes, abort on any copy or launch that leaves its device block, and log what each launch was handed.  The index
// is k | walk << 20 for alignment k: the fake makes `walk` its number of moves, so every slice of a batch gets a longest walk of
// its own (the full row, none, a few words).  One driver, one row of data per family (kFamilies), the family's name on the
// command line.  Built once and run per family by tests/test_table_host_fake.py (g++, ASan + UBSan, no GPU).
//
// Per family, each group printing one ": ok" line per case:
//   refusals     before any device is bound and again after swmi_init, through the host entry, the device entry and the timer,
//                each with its code and its swmi_last_error() text -- one of moves / counts among them, which the long
//                semi-global pair's timers refuse without a device too; n = 0; nothing logged or launched
//   timer order  which of the timer's own arguments and the call's is checked first
//   domain rule  (the striped families that have one) P (len1 + len2) just over 2^23 refused, by the matrix and by each gap, at
//                (32769, 32768) and at 65536 x 65536 -- there (127, -127, 127), gap 65, extend 65, one matrix entry of 65 -- each
//                with its code and text; the boundary (64, -64, 64) at 65536 x 65536 and 128 at 32768 x 32768 accepted: without
//                a device the call then finds none, with one it is launched through the striped launcher with a carry
//   no rule      (the long local pair) (127, -127, 127) at 65536 x 65536 passes the check in the same two ways
//   slices_for   hand-computed sizes with the kernels' real code sizes, the full-slice value, the splits, 0 out of range
//   host entry   traceback and ends-only at n = 1, S, S + 1 and 2.5 S: every score, end and count, every move word up to the
//                slice's longest walk and the sentinel past it, one launch per slice alternating between two streams with the
//                call's shape, gaps, mask and matrix, one 2-D move copy per slice that has a walk, as wide as its longest walk
//   device entry two streams, a workspace that grows only after synchronising its stream; every result over the full rows
//   timer        1 + iters launches on the caller's stream with the call's parameters
//   release      (where there is one) then both entries again, which allocate again; the entries after swmi_shutdown
//   striped      which launcher a shape reaches -- the fixed one for (300, 16384) and (16384, 300), the striped one for
//                (16385, 17) and (64, 16385) -- and the carry: NULL, or 8-byte aligned and of the stated size (fake_table checks
//                it against the device blocks); the workspace of the device entry with and without a carry
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
extern "C" void fake_hip_real_code_sizes(int on);
extern "C" unsigned fake_hip_matrix_sum(const int8_t *sm);

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, swmi_last_error()); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

constexpr uint64_t kSentinel = 0x5E5E5E5E5E5E5E5Eull;
constexpr size_t kCodeWords = 1024;     // fake_hip.cpp kFakeCodeWords (dwords; 512 qwords with affine gaps)
constexpr size_t kStripe = SWMI_GLOBAL_FULL_MAX_LEN;
static int8_t g_sm[16];

// ---- the six signatures of include/swmi.h behind one ----
struct Call { size_t len1, len2; const int8_t *sm; int gap, extend; unsigned mask; };
struct Bufs { const void *s1, *s2; size_t n; void *scores, *ends, *moves, *counts; void *stream; int iters; float *ms; };
#define HOST_BUFS static_cast<const uint8_t *>(b.s1), c.len1, static_cast<const uint8_t *>(b.s2)
#define HOST_OUT static_cast<int32_t *>(b.scores), static_cast<int32_t *>(b.ends), static_cast<uint64_t *>(b.moves), static_cast<uint32_t *>(b.counts)
#define DEV_OUT b.scores, b.ends, b.moves, b.counts, b.stream
// 1: len1 only; 2: both lengths; l / a: linear / affine gaps; m: with a mask
template <auto F> int host_1l(const Call &c, const Bufs &b) { return F(HOST_BUFS, b.n, c.sm, int8_t(c.gap), HOST_OUT); }
template <auto F> int host_1a(const Call &c, const Bufs &b) { return F(HOST_BUFS, b.n, c.sm, c.gap, c.extend, HOST_OUT); }
template <auto F> int host_2l(const Call &c, const Bufs &b) { return F(HOST_BUFS, c.len2, b.n, c.sm, int8_t(c.gap), HOST_OUT); }
template <auto F> int host_2a(const Call &c, const Bufs &b) { return F(HOST_BUFS, c.len2, b.n, c.sm, c.gap, c.extend, HOST_OUT); }
template <auto F> int host_2lm(const Call &c, const Bufs &b) { return F(HOST_BUFS, c.len2, b.n, c.sm, int8_t(c.gap), c.mask, HOST_OUT); }
template <auto F> int host_2am(const Call &c, const Bufs &b) { return F(HOST_BUFS, c.len2, b.n, c.sm, c.gap, c.extend, c.mask, HOST_OUT); }
template <auto F> int dev_1l(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, b.n, c.sm, int8_t(c.gap), DEV_OUT); }
template <auto F> int dev_1a(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, b.n, c.sm, c.gap, c.extend, DEV_OUT); }
template <auto F> int dev_2l(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), DEV_OUT); }
template <auto F> int dev_2a(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, DEV_OUT); }
template <auto F> int dev_2lm(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), c.mask, DEV_OUT); }
template <auto F> int dev_2am(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, c.mask, DEV_OUT); }
template <auto F> int time_1l(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, b.n, c.sm, int8_t(c.gap), DEV_OUT, b.iters, b.ms); }
template <auto F> int time_1a(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, b.n, c.sm, c.gap, c.extend, DEV_OUT, b.iters, b.ms); }
template <auto F> int time_2l(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), DEV_OUT, b.iters, b.ms); }
template <auto F> int time_2a(const Call &c, const Bufs &b) { return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, DEV_OUT, b.iters, b.ms); }
template <auto F> int time_2lm(const Call &c, const Bufs &b)
{
    return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, int8_t(c.gap), c.mask, DEV_OUT, b.iters, b.ms);
}
template <auto F> int time_2am(const Call &c, const Bufs &b)
{
    return F(b.s1, c.len1, b.s2, c.len2, b.n, c.sm, c.gap, c.extend, c.mask, DEV_OUT, b.iters, b.ms);
}
template <auto F> size_t slices_1(size_t n, size_t len1, size_t, int tb, size_t *sizes, size_t cap) { return F(n, len1, tb, sizes, cap); }
template <auto F> size_t slices_2(size_t n, size_t len1, size_t len2, int tb, size_t *sizes, size_t cap) { return F(n, len1, len2, tb, sizes, cap); }

static size_t mw_local(size_t len1, size_t) { return SWMI_LOCAL_MOVE_WORDS(len1); }
static size_t mw_sgfull(size_t len1, size_t len2) { return SWMI_SGFULL_MOVE_WORDS(len1, len2); }
static size_t mw_local_full(size_t len1, size_t len2) { return SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2); }
static size_t mw_global_full(size_t len1, size_t len2) { return SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2); }
static size_t mw_global_long(size_t len1, size_t len2) { return SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2); }
static size_t mw_local_long(size_t len1, size_t len2) { return SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2); }
static size_t mw_semiglobal_long(size_t len1, size_t len2) { return SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(len1, len2); }

// ---- the families ----
struct Shape { size_t len1, len2; };
struct Family {
    const char *name;               // on the command line
    const char *launcher;           // the stand-in's log name
    const char *striped;            // the striped launcher's, for a length above 16384 (else NULL)
    size_t max_len;
    bool fixed_len2;                // len2 is SWMI_LOCAL_SEQ2_LEN
    size_t n_ends;
    const char *count;              // the count array's name in the error text
    uint32_t count_offset;          // count = moves + count_offset
    size_t budget;                  // a traceback slice: alignments of the maximum shape (0: 256 MiB)
    bool affine, mask, timer_first;
    bool domain;                    // a striped family with the domain rule P (len1 + len2) <= 2^23
    bool timer_pair;                // the timer refuses one of moves / counts itself, before it looks for a device
    Shape tb, eo;                   // the shapes of the traceback and the ends-only cases
    size_t (*move_words)(size_t, size_t);
    size_t (*slices_for)(size_t, size_t, size_t, int, size_t *, size_t);
    int (*host)(const Call &, const Bufs &);
    int (*device)(const Call &, const Bufs &);
    int (*timer)(const Call &, const Bufs &);
    int (*release)(void);           // NULL: the family has no release entry
};

static const Family kFamilies[] = {
    {"local", "launch_local", nullptr, SWMI_LOCAL_MAX_LEN, true, 4, "steps", 0, 0, false, false, true, false, false, {200, 128}, {4, 128}, mw_local,
     slices_1<swmi_local_slices_for>, host_1l<swmi_local_align>, dev_1l<swmi_local_align_device>, time_1l<swmi_local_time_device>, nullptr},
    {"sgfull", "launch_sgfull", nullptr, SWMI_SGFULL_MAX_LEN, false, 2, "lengths", 1, 256, false, false, true, false, false, {300, 77}, {4, 1}, mw_sgfull,
     slices_2<swmi_semiglobal_full_slices_for>, host_2l<swmi_semiglobal_full>, dev_2l<swmi_semiglobal_full_device>,
     time_2l<swmi_semiglobal_full_time_device>, swmi_semiglobal_full_release_workspaces},
    {"local_affine", "launch_local_affine", nullptr, SWMI_LOCAL_MAX_LEN, true, 4, "steps", 0, 4096, true, false, true, false, false, {200, 128}, {4, 128},
     mw_local, slices_1<swmi_local_affine_slices_for>, host_1a<swmi_local_align_affine>, dev_1a<swmi_local_align_affine_device>,
     time_1a<swmi_local_affine_time_device>, nullptr},
    {"sgfull_affine", "launch_sgfull_affine", nullptr, SWMI_SGFULL_MAX_LEN, false, 2, "lengths", 1, 256, true, false, false, false, false, {300, 77},
     {4, 1}, mw_sgfull, slices_2<swmi_semiglobal_full_affine_slices_for>, host_2a<swmi_semiglobal_full_affine>,
     dev_2a<swmi_semiglobal_full_affine_device>, time_2a<swmi_semiglobal_full_affine_time_device>,
     swmi_semiglobal_full_affine_release_workspaces},
    {"local_full", "launch_local_full", nullptr, SWMI_LOCAL_FULL_MAX_LEN, false, 4, "steps", 0, 256, false, false, false, false, false, {300, 777}, {4, 1},
     mw_local_full, slices_2<swmi_local_full_slices_for>, host_2l<swmi_local_full>, dev_2l<swmi_local_full_device>,
     time_2l<swmi_local_full_time_device>, swmi_local_full_release_workspaces},
    {"local_full_affine", "launch_local_full_affine", nullptr, SWMI_LOCAL_FULL_MAX_LEN, false, 4, "steps", 0, 256, true, false, false, false, false,
     {300, 777}, {4, 1}, mw_local_full, slices_2<swmi_local_full_affine_slices_for>, host_2a<swmi_local_full_affine>,
     dev_2a<swmi_local_full_affine_device>, time_2a<swmi_local_full_affine_time_device>, swmi_local_full_affine_release_workspaces},
    {"global_full", "launch_global_full", nullptr, SWMI_GLOBAL_FULL_MAX_LEN, false, 4, "steps", 0, 256, false, true, false, false, false, {16384, 16384},
     {4, 1}, mw_global_full, slices_2<swmi_global_full_slices_for>, host_2lm<swmi_global_full>, dev_2lm<swmi_global_full_device>,
     time_2lm<swmi_global_full_time_device>, swmi_global_full_release_workspaces},
    {"global_full_affine", "launch_global_full_affine", nullptr, SWMI_GLOBAL_FULL_MAX_LEN, false, 4, "steps", 0, 256, true, true, false, false, false,
     {16384, 16384}, {4, 1}, mw_global_full, slices_2<swmi_global_full_affine_slices_for>, host_2am<swmi_global_full_affine>,
     dev_2am<swmi_global_full_affine_device>, time_2am<swmi_global_full_affine_time_device>, swmi_global_full_affine_release_workspaces},
    {"global_long", "launch_global_full", "launch_global_long", SWMI_GLOBAL_LONG_MAX_LEN, false, 4, "steps", 0, 256, false, true, false, true, false,
     {65536, 65536}, {4, 1}, mw_global_long, slices_2<swmi_global_long_slices_for>, host_2lm<swmi_global_long>,
     dev_2lm<swmi_global_long_device>, time_2lm<swmi_global_long_time_device>, swmi_global_long_release_workspaces},
    {"global_long_affine", "launch_global_full_affine", "launch_global_long_affine", SWMI_GLOBAL_LONG_MAX_LEN, false, 4, "steps", 0, 256,
     true, true, false, true, false, {65536, 65536}, {4, 1}, mw_global_long, slices_2<swmi_global_long_affine_slices_for>,
     host_2am<swmi_global_long_affine>, dev_2am<swmi_global_long_affine_device>, time_2am<swmi_global_long_affine_time_device>,
     swmi_global_long_affine_release_workspaces},
    {"local_long", "launch_local_full", "launch_local_long", SWMI_LOCAL_LONG_MAX_LEN, false, 4, "steps", 0, 256, false, false, false,
     false, false, {64, 16385}, {4, 1}, mw_local_long, slices_2<swmi_local_long_slices_for>, host_2l<swmi_local_long>,
     dev_2l<swmi_local_long_device>, time_2l<swmi_local_long_time_device>, swmi_local_long_release_workspaces},
    {"local_long_affine", "launch_local_full_affine", "launch_local_long_affine", SWMI_LOCAL_LONG_MAX_LEN, false, 4, "steps", 0, 256, true,
     false, false, false, false, {64, 16385}, {4, 1}, mw_local_long, slices_2<swmi_local_long_affine_slices_for>,
     host_2a<swmi_local_long_affine>, dev_2a<swmi_local_long_affine_device>, time_2a<swmi_local_long_affine_time_device>,
     swmi_local_long_affine_release_workspaces},
    {"semiglobal_long", "launch_sgfull", "launch_sgfull_long", SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, 2, "lengths", 1, 256, false, false,
     false, true, true, {64, 16385}, {4, 1}, mw_semiglobal_long, slices_2<swmi_semiglobal_long_slices_for>, host_2l<swmi_semiglobal_long>,
     dev_2l<swmi_semiglobal_long_device>, time_2l<swmi_semiglobal_long_time_device>, swmi_semiglobal_long_release_workspaces},
    {"semiglobal_long_affine", "launch_sgfull_affine", "launch_sgfull_long_affine", SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, 2, "lengths", 1,
     256, true, false, false, true, true, {64, 16385}, {4, 1}, mw_semiglobal_long, slices_2<swmi_semiglobal_long_affine_slices_for>,
     host_2a<swmi_semiglobal_long_affine>, dev_2a<swmi_semiglobal_long_affine_device>, time_2a<swmi_semiglobal_long_affine_time_device>,
     swmi_semiglobal_long_affine_release_workspaces},
};

static const Family *g_f;
static size_t mw_of(const Shape &a) { return g_f->move_words(a.len1, a.len2); }
static size_t carry_words(const Shape &a) { return g_f->striped && a.len2 > kStripe ? a.len1 * (g_f->affine ? 2 : 1) : 0; }

// the parameters of case number c: gaps over the family's whole domain (under the domain rule they stay within it at
// 65536 x 65536: P <= 64), every mask in turn
static Call call_of(const Shape &a, unsigned c)
{
    c &= 15;
    const int step = g_f->domain && a.len1 + a.len2 > 65536 ? 4 : 8;
    return {a.len1, a.len2, g_sm, int(c) * step + (c == 15 ? step - 1 : 0), g_f->affine ? (16 * step - 1) - int(c) * step : 0, g_f->mask ? c : 0};
}

static std::vector<size_t> slices(const Shape &a, size_t n, bool tb)
{
    std::vector<size_t> s(g_f->slices_for(n, a.len1, a.len2, tb, nullptr, 0));
    CHECK(g_f->slices_for(n, a.len1, a.len2, tb, s.data(), s.size()) == s.size());
    return s;
}
static size_t full_slice(const Shape &a, bool tb) { return slices(a, size_t(1) << 24, tb)[0]; }

// ---- the launch log (fake_hip.cpp fake_table) ----
struct Launch { std::string name; size_t n; int stream, len1, len2, tb; unsigned mask; int gap, extend; unsigned sm; size_t mw; void *carry; };
static std::vector<Launch> launches()
{
    std::vector<Launch> out;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) {
        const char *l = strstr(fake_hip_log_at(k), " launch_");
        if (!l) continue;
        char name[64];
        Launch x{};
        CHECK(sscanf(l, " %63s n%zu stream%d len%dx%d tb%d mask%u gap%d extend%d sm%u mw%zu carry%p", name, &x.n, &x.stream, &x.len1, &x.len2,
                     &x.tb, &x.mask, &x.gap, &x.extend, &x.sm, &x.mw, &x.carry) == 12);
        x.name = name;
        out.push_back(x);
    }
    return out;
}

// what every launch of a call must show: the slice's size, the call's shape, gaps, mask and matrix unchanged, the striped
// launcher exactly where a length exceeds 16384, and a carry exactly where len2 does
static void check_launches(const std::vector<Launch> &l, const std::vector<size_t> &sizes, const Call &c, bool tb)
{
    CHECK(l.size() == sizes.size());
    const bool striped = g_f->striped && (c.len1 > kStripe || c.len2 > kStripe);
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].name == (striped ? g_f->striped : g_f->launcher) && l[i].n == sizes[i] && l[i].tb == tb);
        CHECK(l[i].len1 == int(c.len1) && l[i].len2 == int(c.len2) && l[i].mw == g_f->move_words(c.len1, c.len2));
        CHECK(l[i].mask == c.mask && l[i].gap == c.gap && l[i].extend == c.extend && l[i].sm == fake_hip_matrix_sum(c.sm));
        CHECK((l[i].carry != nullptr) == (g_f->striped && c.len2 > kStripe) && (reinterpret_cast<uintptr_t>(l[i].carry) & 7) == 0);
    }
}

// ---- the fake's results for index id ----
static uint32_t walk_of(const Shape &a, uint32_t id) { return uint32_t((id >> 20) % (32 * mw_of(a) + 1)); }
static uint64_t move_word(uint32_t id, size_t w) { return 0xC0DEull << 48 | uint64_t(id) << 16 | w; }

// alignment k of a batch whose slices are `sizes`: index k | walk << 20, the walk bounded per slice by 70 moves, none, and
// the full row in turn (k < 2^20 whenever there is a walk)
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

// every result of alignment k; move words from `words` on must hold the sentinel (SIZE_MAX: the whole row was written)
static void check_results(const Shape &a, const std::vector<uint32_t> &id, size_t k, const int32_t *scores, const int32_t *ends,
                          const uint64_t *moves, const uint32_t *counts, size_t words)
{
    uint32_t i = 0;
    memcpy(&i, &id[k], a.len1 < 4 ? a.len1 : 4);
    const size_t mw = mw_of(a), ne = g_f->n_ends;
    bool ok = scores[k] == int32_t(2 * i + 1);
    for (size_t e = 0; e < ne; ++e) ok = ok && ends[k * ne + e] == int32_t(8 * i + e + 3);
    if (moves) {
        ok = ok && counts[k] == walk_of(a, i) + g_f->count_offset;
        for (size_t w = 0; w < mw; ++w) ok = ok && moves[k * mw + w] == (w < words ? move_word(i, w) : kSentinel);
    }
    if (!ok) {
        fprintf(stderr, "%s len %zu x %zu: alignment %zu (index %#x, %zu move words copied) has wrong results\n", g_f->name, a.len1, a.len2,
                k, i, words);
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
    std::vector<int32_t> scores(n, -1), ends(n * g_f->n_ends, -1);
    std::vector<uint64_t> moves(tb ? n * mw : 0, kSentinel);
    std::vector<uint32_t> counts(tb ? n : 0, 0);          // (a pipeline that read them before the copy-back saw no walk)
    fake_hip_log_clear();
    CHECK(g_f->host(call, {s1.data(), s2.data(), n, scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? counts.data() : nullptr,
                           nullptr, 0, nullptr}) == SWMI_OK);

    // one launch per slice, alternating between two streams
    const std::vector<Launch> l = launches();
    check_launches(l, sizes, call, tb);
    for (size_t i = 0; i < l.size(); ++i) {
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
    printf("  host   %5zu x %5zu n %7zu %-10s gaps %3d %3d mask %2u: %zu slices, move words per slice", a.len1, a.len2, n,
           tb ? "traceback" : "ends-only", call.gap, call.extend, call.mask, sizes.size());
    for (size_t w : words) printf(" %zu", w);
    printf(": ok\n");
}

// the workspace a device call of n alignments needs on its stream: one slice's codes (with a traceback) and carry
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

// one device-entry call on `st` with buffers of exactly n alignments; returns the log of the call less its launches
static std::vector<std::string> device_case(const Shape &a, size_t n, bool tb, hipStream_t st, int stream_id, unsigned c)
{
    const Call call = call_of(a, c);
    const std::vector<size_t> sizes = slices(a, n, tb);
    const std::vector<uint32_t> id = indices(a, sizes, tb);
    const size_t mw = mw_of(a);
    void *s1, *s2, *scores, *ends, *moves = nullptr, *counts = nullptr;
    CHECK(hipMalloc(&s1, n * a.len1) == hipSuccess && hipMalloc(&s2, n * a.len2) == hipSuccess);
    CHECK(hipMalloc(&scores, n * 4) == hipSuccess && hipMalloc(&ends, n * g_f->n_ends * 4) == hipSuccess);
    if (tb) CHECK(hipMalloc(&moves, n * mw * 8) == hipSuccess && hipMalloc(&counts, n * 4) == hipSuccess);
    fill_seq1(a, id, static_cast<uint8_t *>(s1));
    memset(s2, 0, n * a.len2);
    fake_hip_log_clear();
    CHECK(g_f->device(call, {s1, s2, n, scores, ends, moves, counts, st, 0, nullptr}) == SWMI_OK);
    const std::vector<Launch> l = launches();
    check_launches(l, sizes, call, tb);
    for (const Launch &x : l) CHECK(x.stream == stream_id && x.carry == l[0].carry);
    for (size_t k = 0; k < n; ++k)      // (the fake's launches write at once; the device entry copies nothing)
        check_results(a, id, k, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(counts), SIZE_MAX);
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k)
        if (!strstr(fake_hip_log_at(k), " launch_")) log.push_back(fake_hip_log_at(k));
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    printf("  device %5zu x %5zu n %7zu %-10s gaps %3d %3d mask %2u on stream %d: %zu slices: ok\n", a.len1, a.len2, n,
           tb ? "traceback" : "ends-only", call.gap, call.extend, call.mask, stream_id, sizes.size());
    return log;
}

// ---- refusals ----
static int g_pass;      // 0: no device bound; 1: after swmi_init
enum Entry { kHost, kDevice, kTimer };
static const char *const kNotInit = "swmi_init() has not been called (or failed)";

static void refused(int rc, int code, const std::string &text, int line)
{
    if (rc == code && text == swmi_last_error()) return;
    fprintf(stderr, "line %d, pass %d: got %d \"%s\", expected %d \"%s\"\n", line, g_pass, rc, swmi_last_error(), code, text.c_str());
    exit(1);
}
#define REFUSED(rc, code, text) refused(rc, code, text, __LINE__)

static std::string lengths_text(size_t len1, size_t len2)
{
    if (g_f->fixed_len2) return "len1 " + std::to_string(len1) + " outside [1, " + std::to_string(g_f->max_len) + "]";
    return "lengths (" + std::to_string(len1) + ", " + std::to_string(len2) + ") outside [1, " + std::to_string(g_f->max_len) + "]";
}
static std::string gaps_text(int gap, int extend)
{
    if (!g_f->affine) return "gap_penalty " + std::to_string(gap) + " < 0 is outside the supported domain [0,127]";
    return "gap_open " + std::to_string(gap) + " / gap_extend " + std::to_string(extend) + " outside [0,127]";
}
static std::string domain_text(size_t total)
{
    return std::string(g_f->affine ? "max(1, |score|, gap_open, gap_extend)" : "max(1, |score|, gap)") + " * (len1 + len2) = P * " +
           std::to_string(total) + " above 2^23";
}

static void refusals()
{
    std::vector<uint8_t> seq(2 * g_f->max_len + 64, 0);
    const uint8_t *s = seq.data() + (16 - (reinterpret_cast<uintptr_t>(seq.data()) & 15)) % 16;     // (a device entry that passes
    alignas(16) int32_t sc1 = 0, e4[4] = {0, 0, 0, 0};                                              //   its checks wants 16-byte alignment)
    uint64_t mv1[2] = {0, 0};
    uint32_t ct1 = 0;
    float ms = 0.f;
    const size_t max = g_f->max_len;
    const Call good{5, g_f->fixed_len2 ? size_t(SWMI_LOCAL_SEQ2_LEN) : 5, g_sm, 3, g_f->affine ? 2 : 0, 0};
    const Bufs bufs{s, s + max + 16, 1, &sc1, e4, nullptr, nullptr, nullptr, 2, &ms};
    const auto with = [](Call c, size_t len1, size_t len2) { c.len1 = len1; c.len2 = len2; return c; };
    int8_t sm64[16], sm65[16], sm127[16], sm128[16];
    for (int i = 0; i < 16; ++i) {
        sm64[i] = int8_t(i % 5 == 0 ? 64 : -64);
        sm65[i] = int8_t(i % 5 == 0 ? 64 : -65);
        sm127[i] = int8_t(i % 5 == 0 ? 127 : -127);
        sm128[i] = int8_t(i % 5 == 0 ? 1 : -128);
    }
    for (int e = kHost; e <= kTimer; ++e) {
        const auto entry = e == kHost ? g_f->host : e == kDevice ? g_f->device : g_f->timer;
        // what the call's own arguments are refused with: a timer that checks its own first finds no device in pass 0
        const bool no_device = e == kTimer && g_f->timer_first && g_pass == 0;
        const auto args = [&](const Call &c, int code, const std::string &text, int line) {
            refused(entry(c, bufs), no_device ? SWMI_ERR_NOT_INITIALIZED : code, no_device ? kNotInit : text, line);
        };
        const int bad = SWMI_ERR_INVALID_ARGUMENT;
        args(with(good, 0, good.len2), bad, lengths_text(0, good.len2), __LINE__);
        args(with(good, max + 1, good.len2), bad, lengths_text(max + 1, good.len2), __LINE__);
        if (!g_f->fixed_len2) {
            args(with(good, 5, 0), bad, lengths_text(5, 0), __LINE__);
            args(with(good, 5, max + 1), bad, lengths_text(5, max + 1), __LINE__);
        }
        Call c = with(good, 0, good.len2);      // the lengths before everything else
        c.sm = nullptr;
        c.gap = -1;
        args(c, bad, lengths_text(0, good.len2), __LINE__);
        c = good;
        if (g_f->mask) {
            c.mask = 16;
            args(c, bad, "free_ends 16 above 15", __LINE__);
            c.gap = -1;                 // the mask before the gaps,
            args(c, bad, "free_ends 16 above 15", __LINE__);
            c = with(c, 0, 5);          // and the lengths before the mask
            args(c, bad, lengths_text(0, 5), __LINE__);
        }
        c = good;
        c.sm = nullptr;
        args(c, bad, "score_matrix is NULL", __LINE__);
        c.gap = -1;                     // the matrix before the gaps
        args(c, bad, "score_matrix is NULL", __LINE__);
        c = good;
        c.gap = -1;
        args(c, SWMI_ERR_DOMAIN, gaps_text(-1, c.extend), __LINE__);
        if (g_f->affine) {
            c.gap = 128;
            args(c, SWMI_ERR_DOMAIN, gaps_text(128, c.extend), __LINE__);
            c = good;
            c.extend = 128;
            args(c, SWMI_ERR_DOMAIN, gaps_text(c.gap, 128), __LINE__);
            c.extend = -1;
            args(c, SWMI_ERR_DOMAIN, gaps_text(c.gap, -1), __LINE__);
        }
        if (g_f->domain) {              // P (len1 + len2) just over 2^23, by the matrix and by each gap
            c = with(good, 32769, 32768);
            c.sm = sm128;
            args(c, bad, domain_text(65537), __LINE__);
            c = with(good, 65536, 65536);
            c.sm = sm65;
            args(c, bad, domain_text(131072), __LINE__);
            c.sm = sm127;               // the int8 extremes
            c.gap = 127;
            c.extend = g_f->affine ? 127 : 0;
            args(c, bad, domain_text(131072), __LINE__);
            c.sm = sm64;
            c.gap = 65;
            c.extend = g_f->affine ? 64 : 0;
            args(c, bad, domain_text(131072), __LINE__);
            if (g_f->affine) {
                c.gap = 64;
                c.extend = 65;
                args(c, bad, domain_text(131072), __LINE__);
            }
            c.gap = c.extend = 64;      // one matrix entry of 65
            if (!g_f->affine) c.extend = 0;
            sm64[0] = 65;
            args(c, bad, domain_text(131072), __LINE__);
            sm64[0] = 64;
            c.gap = -1;                 // the gaps' own domain before the rule
            c.extend = good.extend;
            args(c, SWMI_ERR_DOMAIN, gaps_text(-1, c.extend), __LINE__);
        }
        if (g_f->striped && g_pass == 0) {
            // what passes the check at 65536 x 65536 then finds no device: the edge of the rule (64, -64, 64), or without a
            // rule the int8 extremes (127, -127, 127)
            c = with(good, 65536, 65536);
            c.sm = g_f->domain ? sm64 : sm127;
            c.gap = g_f->domain ? 64 : 127;
            c.extend = g_f->affine ? c.gap : 0;
            refused(entry(c, bufs), SWMI_ERR_NOT_INITIALIZED, kNotInit, __LINE__);
        }
        // the buffers: checked by the pipeline once the arguments have passed, by the timer only with a device
        const bool unbound = e == kTimer && g_pass == 0;
        const auto buffers = [&](Bufs b, const std::string &text, int line) {
            refused(entry(good, b), unbound ? SWMI_ERR_NOT_INITIALIZED : bad, unbound ? kNotInit : text, line);
        };
        // one of moves / counts: a timer that checks the pair itself refuses it without a device too
        const auto pair = [&](Bufs b, const std::string &text, int line) {
            if (g_f->timer_pair) refused(entry(good, b), bad, text, line);
            else buffers(b, text, line);
        };
        const std::string null_text = e == kHost ? "NULL buffer with n = 1" : "NULL device buffer with n = 1";
        const std::string pair_text = std::string("moves and ") + g_f->count + " must both be given (traceback) or both be NULL (ends-only)";
        Bufs b = bufs;
        b.s1 = nullptr;
        buffers(b, null_text, __LINE__);
        c = good;
        c.gap = -1;                     // the arguments before the buffers
        refused(entry(c, b), no_device ? SWMI_ERR_NOT_INITIALIZED : SWMI_ERR_DOMAIN, no_device ? kNotInit : gaps_text(-1, c.extend), __LINE__);
        b = bufs;
        b.s2 = nullptr;
        buffers(b, null_text, __LINE__);
        b = bufs;
        b.scores = nullptr;
        buffers(b, null_text, __LINE__);
        b = bufs;
        b.ends = nullptr;
        buffers(b, null_text, __LINE__);
        b = bufs;
        b.moves = mv1;
        pair(b, pair_text, __LINE__);
        b.s1 = nullptr;                 // the pair before the NULLs
        pair(b, pair_text, __LINE__);
        b = bufs;
        b.counts = &ct1;
        pair(b, pair_text, __LINE__);
        b = Bufs{nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 2, &ms};       // n = 0
        if (e == kTimer) REFUSED(entry(good, b), bad, "n is 0");        // (the timer's own, before the device is looked up)
        else CHECK(entry(good, b) == SWMI_OK);
    }
    CHECK(fake_hip_log_size() == 0);
}

// Which of the timer's own arguments (iters, avg_ms, n) and the call's is checked first: with both wrong the first one's text
// comes back, with or without a device.  A wrong length alone finds the device missing first where the timer checks first.
static void timer_order()
{
    uint8_t s[8] = {0};
    int32_t sc1 = 0, e4[4] = {0, 0, 0, 0};
    float ms = 0.f;
    const Call good{5, g_f->fixed_len2 ? size_t(SWMI_LOCAL_SEQ2_LEN) : 5, g_sm, 3, g_f->affine ? 2 : 0, 0};
    Call longer = good;
    longer.len1 = g_f->max_len + 1;
    const Bufs valid{s, s, 1, &sc1, e4, nullptr, nullptr, nullptr, 2, &ms};
    Bufs no_iters = valid;
    no_iters.iters = 0;
    const int bad = SWMI_ERR_INVALID_ARGUMENT;
    const std::string timer_text = "avg_ms is NULL or iters 0 < 1", call_text = lengths_text(longer.len1, longer.len2);
    REFUSED(g_f->timer(longer, no_iters), bad, g_f->timer_first ? timer_text : call_text);
    if (g_f->timer_first && g_pass == 0) REFUSED(g_f->timer(longer, valid), SWMI_ERR_NOT_INITIALIZED, kNotInit);
    else REFUSED(g_f->timer(longer, valid), bad, call_text);
    REFUSED(g_f->timer(good, no_iters), bad, timer_text);           // (in either order before the device is looked up)
    CHECK(fake_hip_log_size() == 0);
}

// What passes the check at the top of a striped family's range is launched, through the striped launcher with a carry: under
// the domain rule its boundary from inside, without one the int8 extremes at 65536 x 65536
static void top_of_range()
{
    std::vector<uint8_t> big(2 * 65536, 0);
    int32_t sc1 = 0, e4[4] = {0, 0, 0, 0};
    int8_t sm64[16], sm127[16], sm128[16];
    for (int i = 0; i < 16; ++i) {
        sm64[i] = int8_t(i % 5 == 0 ? 64 : -64);
        sm127[i] = int8_t(i % 5 == 0 ? 127 : -127);
        sm128[i] = int8_t(i % 5 == 0 ? 1 : -128);
    }
    fake_hip_log_clear();
    const Call at64{65536, 65536, sm64, 64, g_f->affine ? 64 : 0, 0}, at128{32768, 32768, sm128, 127, g_f->affine ? 127 : 0, 0};
    const Call top{65536, 65536, sm127, 127, g_f->affine ? 127 : 0, 0};
    const std::vector<Call> calls = g_f->domain ? std::vector<Call>{at64, at128} : std::vector<Call>{top};
    for (const Call &c : calls) {
        CHECK(g_f->host(c, {big.data(), big.data() + 65536, 1, &sc1, e4, nullptr, nullptr, nullptr, 0, nullptr}) == SWMI_OK);
        const std::vector<Launch> l = launches();
        check_launches({l.back()}, {1}, c, false);
    }
    CHECK(launches().size() == calls.size());
    if (g_f->domain) printf("  domain rule: (65536, 65536) with P = 64 and (32768, 32768) with P = 128 accepted, just over 2^23 refused: ok\n");
    else printf("  no domain rule: (127, -127, 127) at 65536 x 65536 accepted and launched: ok\n");
}

// swmi_*_slices_for, no device: with the kernels' own code sizes against sizes worked out by hand, then with the fake's
static void slice_sizes()
{
    const size_t max = g_f->max_len, top = g_f->striped ? kStripe : max;      // top: the shape that sets the budget
    const Shape full{top, g_f->fixed_len2 ? size_t(SWMI_LOCAL_SEQ2_LEN) : top}, one{1, g_f->fixed_len2 ? size_t(SWMI_LOCAL_SEQ2_LEN) : 1};
    const size_t ne = 4 * g_f->n_ends, M = size_t(1) << 20;
    fake_hip_real_code_sizes(1);
    if (g_f->budget) {      // `budget` of the top shape, whatever a full-size alignment takes
        const size_t b = g_f->budget;
        CHECK((slices(full, b + 1, true) == std::vector<size_t>{b, 1}) && (slices(full, b, true) == std::vector<size_t>{b}));
        CHECK((slices(full, 2 * b + b / 3, true) == std::vector<size_t>{b, b, b / 3}) && slices(full, 0, true).empty());
    }
    // ends-only within 256 MiB: inputs, score, ends
    const size_t per = full.len1 + full.len2 + 4 + ne, eo_slice = (size_t(256) << 20) / per;
    const std::vector<size_t> eo = slices(full, 2 * eo_slice + 7, false);
    CHECK(eo.size() == 3 && eo[0] == eo_slice && eo[1] == eo_slice && eo[2] == 7 && eo_slice * per <= (size_t(256) << 20));
    if (!g_f->fixed_len2 && max >= 16384) CHECK(eo_slice == (g_f->n_ends == 4 ? 8187 : 8189));
    // a traceback slice of 4096 (x 4096) against the budget, both from the kernels' formulas by hand
    if (g_f->fixed_len2) {
        // local kernels: (len1 + 15 + 7) / 8 trips of 8 steps x 16 lanes, one dword per step pair (affine: per step); 16384: 2050 trips
        const size_t unit = g_f->affine ? 128 : 64;
        const size_t one_tb = 4096 + 128 + 4 + 16 + size_t(514) * unit * 4 + SWMI_LOCAL_MOVE_WORDS(4096) * 8 + 4;
        const size_t budget = g_f->budget ? g_f->budget * (16384 + 128 + 4 + 16 + size_t(2050) * unit * 4 + SWMI_LOCAL_MOVE_WORDS(16384) * 8 + 4)
                                          : size_t(256) << 20;
        CHECK(slices({4096, 128}, 1000000, true)[0] == budget / one_tb);
    } else {
        // tile kernels: 4 waves x 1040 trips x 256 code words at 4096 x 4096, 16 x 4112 x 256 at 16384 x 16384; 256 and 1024 move words
        const size_t unit = g_f->affine ? 8 : 4;
        const size_t one_tb = 4096 + 4096 + 4 + ne + size_t(4) * 1040 * 256 * unit + 256 * 8 + 4;
        const size_t budget = 256 * (16384 + 16384 + 4 + ne + size_t(16) * 4112 * 256 * unit + 1024 * 8 + 4);
        CHECK(slices({4096, 4096}, 1000000, true)[0] == budget / one_tb);
    }
    // the cap of 2^20 alignments per slice
    CHECK((slices(one, 3 * M + 5, false) == std::vector<size_t>{M, M, M, 5}));
    if (g_f->budget) CHECK(slices(one, M + 1, true).size() == 2);
    fake_hip_real_code_sizes(0);
    // with the fake's code sizes: the full-slice value and the splits {1}, {S}, {S, 1}, {S, S, S / 2}
    if (g_f->budget) CHECK(full_slice(full, true) == g_f->budget);
    for (int tb = 0; tb < 2; ++tb) {
        const Shape &a = tb ? g_f->tb : g_f->eo;
        const size_t S = full_slice(a, tb);
        CHECK(S > 1 && S <= M);
        CHECK((slices(a, 1, tb) == std::vector<size_t>{1}) && (slices(a, S, tb) == std::vector<size_t>{S}));
        CHECK((slices(a, S + 1, tb) == std::vector<size_t>{S, 1}) && (slices(a, 2 * S + S / 2, tb) == std::vector<size_t>{S, S, S / 2}));
    }
    // out of range: 0, and nothing written
    size_t untouched = 77;
    CHECK(g_f->slices_for(10, 0, one.len2, 1, &untouched, 1) == 0 && g_f->slices_for(10, max + 1, one.len2, 1, &untouched, 1) == 0);
    if (!g_f->fixed_len2) CHECK(g_f->slices_for(10, 5, 0, 1, &untouched, 1) == 0 && g_f->slices_for(10, 5, max + 1, 0, &untouched, 1) == 0);
    CHECK(untouched == 77 && fake_hip_log_size() == 0);
    printf("  slices_for against hand-computed sizes, the full slice, the splits, out of range, no device: ok\n");
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    for (const Family &f : kFamilies)
        if (argv[1] == std::string(f.name)) g_f = &f;
    CHECK(g_f && "unknown family");
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 1 : -1);

    // every argument error and n = 0 come back before any device is touched and before anything is launched
    for (g_pass = 0; g_pass < 2; ++g_pass) {
        refusals();
        timer_order();
        if (g_pass == 0) {
            slice_sizes();
            CHECK(swmi_init(0) == SWMI_OK);
            fake_hip_log_clear();
        }
    }
    printf("  lengths of 0 and %zu, %sgaps outside their domain, NULLs, one of moves / %s, n = 0%s: refused with their texts through the "
           "host entry, the device entry and the timer, without a device and with one, nothing launched: ok\n",
           g_f->max_len + 1, g_f->mask ? "a mask of 16, " : "", g_f->count, g_f->domain ? ", calls outside the domain rule" : "");
    printf("  the timer checks %s first: ok\n", g_f->timer_first ? "its own arguments" : "the call's arguments");
    if (g_f->striped) top_of_range();

    // host entry: n = 1, one slice, one slice + 1, two and a half slices; a family with a mask twice, for every mask once
    const Shape &tb_a = g_f->tb, &eo_a = g_f->eo;
    unsigned c = 0;
    for (const Shape *a : {&tb_a, &eo_a}) {
        const bool tb = a == &tb_a;
        const size_t s = full_slice(*a, tb);
        for (size_t n : {size_t(1), s, s + 1, 2 * s + s / 2})
            for (int twice = 0; twice < (g_f->mask ? 2 : 1); ++twice) host_case(*a, n, tb, c++);
    }

    // device entry on two streams; the second call on stream A grows its workspace (after synchronising that stream)
    hipStream_t sa, sb;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    fake_hip_log_clear();
    CHECK(hipStreamSynchronize(sa) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess);
    int ida = 0, idb = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &ida) == 1 && sscanf(fake_hip_log_at(1), "dev0 stream_sync stream%d", &idb) == 1);
    const size_t s = full_slice(tb_a, true), big = 2 * s + s / 2;
    CHECK(has(device_case(tb_a, 3, true, sa, ida, c++), workspace_malloc(tb_a, 3, true)));
    CHECK(has(device_case(tb_a, big, true, sb, idb, c++), workspace_malloc(tb_a, big, true)));
    std::vector<std::string> log = device_case(tb_a, big, true, sa, ida, c++);
    CHECK(log.size() == 2 && log[0] == "dev0 stream_sync stream" + std::to_string(ida) && log[1] == workspace_malloc(tb_a, big, true));
    log = device_case(tb_a, 5, true, sb, idb, c++);             // fits: no synchronisation, no allocation
    CHECK(log.empty());
    log = device_case(eo_a, 7, false, sa, ida, c++);            // ends-only: no workspace, nothing but the launch
    CHECK(log.empty());

    if (g_f->striped) {
        // which launcher a shape reaches, and the carry (check_launches): the fixed-length launcher, the same across, the
        // striped launcher without a carry, and with one
        const Shape wide{64, 16385}, tall{16385, 17}, small{300, 16384}, small2{16384, 300};
        for (const Shape *a : {&small, &small2, &tall, &wide})
            for (int tb = 1; tb >= 0; --tb) host_case(*a, 7, tb != 0, c++);
        CHECK(device_case(wide, 7, false, sa, ida, c++).empty());          // ends-only on a stream that has a workspace: the carry fits
        CHECK(device_case(tall, 9, false, sa, ida, c++).empty());          // the striped launcher without a carry: no workspace
        // an ends-only call with a carry takes a workspace of the carry alone, on a fresh stream
        hipStream_t sc;
        CHECK(hipStreamCreateWithFlags(&sc, 0) == hipSuccess);
        fake_hip_log_clear();
        CHECK(hipStreamSynchronize(sc) == hipSuccess);
        int idc = 0;
        CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &idc) == 1);
        log = device_case(wide, 9, false, sc, idc, c++);
        CHECK(workspace_bytes(wide, 9, false) == ((9 * carry_words(wide) * 4 + 15) & ~size_t(15)) && has(log, workspace_malloc(wide, 9, false)));
        CHECK(device_case(tall, 9, false, sc, idc, c++).empty());
        CHECK(device_case(small, 9, true, sc, idc, c++).size() == 2);      // grows: codes beside the carry's bytes
        CHECK(device_case(wide, 3, true, sc, idc, c++).empty());           // codes and carry fit
        CHECK(hipStreamDestroy(sc) == hipSuccess);
    }

    // the timer: one untimed call, then `iters` timed ones (the fake's events are 1 ms apart)
    void *d[6];
    const size_t n = 5, mw = mw_of(tb_a);
    const size_t bytes[6] = {n * tb_a.len1, n * tb_a.len2, n * 4, n * g_f->n_ends * 4, n * mw * 8, n * 4};
    for (int k = 0; k < 6; ++k) {
        CHECK(hipMalloc(&d[k], bytes[k]) == hipSuccess);
        memset(d[k], 0, bytes[k]);
    }
    float ms = 0.f;
    fake_hip_log_clear();
    const Call timed = call_of(tb_a, c++);
    CHECK(g_f->timer(timed, {d[0], d[1], n, d[2], d[3], d[4], d[5], sb, 4, &ms}) == SWMI_OK);
    const std::vector<Launch> l = launches();
    CHECK(ms == 0.25f && l.size() == 5);
    check_launches(l, std::vector<size_t>(5, n), timed, true);
    for (const Launch &x : l) CHECK(x.stream == idb);
    printf("  timer: 1 + 4 launches on the caller's stream, %.2f ms each: ok\n", ms);

    if (g_f->release) {     // the release frees the workspaces and the host sets; the next calls allocate them again
        CHECK(g_f->release() == SWMI_OK);
        CHECK(has(device_case(tb_a, 5, true, sb, idb, c++), workspace_malloc(tb_a, 5, true)));
        host_case(tb_a, s + 1, true, c++);
        size_t mallocs = 0;
        for (size_t k = 0; k < fake_hip_log_size(); ++k) mallocs += strstr(fake_hip_log_at(k), " malloc ") != nullptr;
        CHECK(mallocs >= 2 * 7);        // two sets of seq1, seq2, scores, ends, counts, codes, moves
        CHECK(g_f->release() == SWMI_OK);
        printf("  release_workspaces, then both entries again: ok\n");
    }
    for (void *p : d) CHECK(hipFree(p) == hipSuccess);
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    CHECK(swmi_shutdown() == SWMI_OK);
    // after the shutdown: argument errors and n = 0 as before, a real call reports that nothing is initialised, the release
    // and the slice arithmetic need no device
    {
        uint8_t b1[8] = {0}, b2[128] = {0};
        int32_t sc[1], en[4];
        const Call good{5, g_f->fixed_len2 ? size_t(SWMI_LOCAL_SEQ2_LEN) : 5, g_sm, 3, g_f->affine ? 2 : 0, 0};
        Call worse = good;
        worse.gap = -1;
        const Bufs one{b1, b2, 1, sc, en, nullptr, nullptr, nullptr, 2, nullptr}, none{b1, b2, 0, sc, en, nullptr, nullptr, nullptr, 2, nullptr};
        CHECK(g_f->host(good, none) == SWMI_OK && g_f->device(good, none) == SWMI_OK);
        REFUSED(g_f->host(worse, one), SWMI_ERR_DOMAIN, gaps_text(-1, worse.extend));
        REFUSED(g_f->host(good, one), SWMI_ERR_NOT_INITIALIZED, kNotInit);
        REFUSED(g_f->device(good, one), SWMI_ERR_NOT_INITIALIZED, kNotInit);
        if (g_f->release) REFUSED(g_f->release(), SWMI_ERR_NOT_INITIALIZED, kNotInit);
        CHECK(slices(tb_a, 10, true).size() == 1);
        printf("  after swmi_shutdown: ok\n");
    }
    printf("table host fake ok: %s\n", g_f->name);
    return 0;
}
