// local_full_affine_host_fake.cpp -- the host side of the any-length affine local aligner (swmi_local_full_affine*,
// local_full_affine_api.cpp through the slice pipeline of swmi_table.cpp) on a fake GPU (fake_hip.cpp), plus the stand-in for its launcher, which fake_hip.cpp does
// not know.  The stand-in follows fake_hip.cpp's table stand-ins: alignment k of a launch reads its index `id` from the first
// (up to) four bytes of its seq1 and writes score 2 id + 1, ends[e] = 8 id + e + 3 (four of them), and with a traceback
// (id >> 20) % (32 move_words + 1) steps and move word w = 0xC0DE << 48 | id << 16 | w in every word of its row; it touches
// the first and last byte of every buffer it is handed, codes included, so that ASan sees a buffer that is too small.  Code
// workspaces take a constant 512 qwords per alignment, so a traceback slice is a few thousand alignments -- except while
// g_real_sizes is set, when the stand-in gives the kernel's own code size, for the slice sizes worked out by hand.
// Built and run by tests/test_local_full_affine_host_fake.py (g++, ASan + UBSan, no GPU).
//
// Before any device exists: the argument checks in the order the header gives them, n = 0, and swmi_local_full_affine_slices_for
// against hand-computed sizes (257 alignments of 16384 x 16384 with traceback -> 256 and 1; ends-only within 256 MiB; the cap
// of 2^20 alignments).
// Host entry, traceback and ends-only, at n = 1, one slice, one slice + 1 and two and a half slices: every score, end and
// count, every move word up to the slice's longest walk and the sentinel past it, one launch per slice alternating between
// two streams, one 2-D move copy per slice that has a walk, as wide as its longest walk.  Device entry on two streams,
// growing a stream's workspace.  The timer's warm-up call.  The release of the workspaces, and calls after it; the entries after swmi_shutdown.
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
constexpr size_t kCodeWords = 1024;                      // dwords: 512 qwords
constexpr int kOpen = 5, kExtend = 2;
static int8_t g_sm[16];
static bool g_real_sizes = false;

// ---- the launcher stand-in ------------------------------------------------------------------------------------------------
struct Launch { size_t n; hipStream_t stream; int len1, len2; bool traceback; };
static std::mutex g_launch_mu;
static std::vector<Launch> g_launches;

namespace swmi {
size_t local_full_affine_code_qwords(int len1, int len2)
{
    if (!g_real_sizes) return kCodeWords / 2;
    return size_t((len2 + 1023) / 1024) * size_t((len1 + 63 + 31) / 32 * 8) * 256;   // waves x trips x 256
}
hipError_t launch_local_full_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap_open,
                                    int gap_extend, int32_t *scores, int32_t *ends, unsigned long long *codes,
                                    unsigned long long *moves, uint32_t *steps, size_t move_words, hipStream_t st)
{
    {
        std::lock_guard<std::mutex> l(g_launch_mu);
        g_launches.push_back({n, st, len1, len2, moves != nullptr});
    }
    if (n == 0) return hipSuccess;
    CHECK(sm && gap_open == kOpen && gap_extend == kExtend && memcmp(sm, g_sm, 16) == 0);
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
static Shape shape(size_t len1, size_t len2) { return {len1, len2, SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2)}; }

static std::vector<size_t> slices(const Shape &a, size_t n, bool tb)
{
    std::vector<size_t> s(swmi_local_full_affine_slices_for(n, a.len1, a.len2, tb, nullptr, 0));
    swmi_local_full_affine_slices_for(n, a.len1, a.len2, tb, s.data(), s.size());
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

static void host_case(const Shape &a, size_t n, bool tb)
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
    CHECK(swmi_local_full_affine(s1.data(), a.len1, s2.data(), a.len2, n, g_sm, kOpen, kExtend, scores.data(), ends.data(), tb ? moves.data() : nullptr,
                          tb ? counts.data() : nullptr) == SWMI_OK);

    // one launch per slice, alternating between two streams
    const std::vector<Launch> l = take_launches();
    CHECK(l.size() == sizes.size());
    for (size_t i = 0; i < l.size(); ++i) {
        CHECK(l[i].n == sizes[i] && l[i].traceback == tb && l[i].len1 == int(a.len1) && l[i].len2 == int(a.len2));
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
    printf("  host n %7zu %-10s: %zu slices, move words per slice", n, tb ? "traceback" : "ends-only", sizes.size());
    for (size_t w : words) printf(" %zu", w);
    printf(": ok\n");
}

// one device-entry call on `st` with buffers of exactly n alignments; returns the log of the call
static std::vector<std::string> device_case(const Shape &a, size_t n, bool tb, hipStream_t st)
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
    CHECK(swmi_local_full_affine_device(s1, a.len1, s2, a.len2, n, g_sm, kOpen, kExtend, scores, ends, moves, counts, st) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    CHECK(l.size() == sizes.size());
    for (size_t i = 0; i < l.size(); ++i) CHECK(l[i].n == sizes[i] && l[i].stream == st && l[i].traceback == tb);
    for (size_t k = 0; k < n; ++k)      // (the fake's launches write at once; the device entry copies nothing)
        check_results(a, id, k, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(counts), SIZE_MAX);
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) log.push_back(fake_hip_log_at(k));
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    printf("  device n %7zu %-10s: %zu slices: ok\n", n, tb ? "traceback" : "ends-only", sizes.size());
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
    // every argument error and n = 0 come back before any device is touched
    {
        uint8_t b1[8] = {0}, b2[8] = {0};
        int32_t sc[1], en[4];
        uint64_t mv[2];
        uint32_t st[1];
        auto call = [&](size_t len1, size_t len2, const uint8_t *s1, const uint8_t *s2, const int8_t *sm, int go, int ge, int32_t *scores,
                        int32_t *ends, uint64_t *moves, uint32_t *steps, size_t n = 1) {
            return swmi_local_full_affine(s1, len1, s2, len2, n, sm, go, ge, scores, ends, moves, steps);
        };
        // the order of the header: lengths, the matrix, the gaps (domain), then the buffers
        CHECK(call(0, 5, nullptr, nullptr, nullptr, -1, 128, nullptr, nullptr, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 16385, b1, b2, g_sm, kOpen, kExtend, sc, en, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 5, b1, b2, nullptr, -1, kExtend, sc, en, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 5, nullptr, b2, g_sm, -1, kExtend, sc, en, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(call(5, 5, b1, b2, g_sm, 128, kExtend, sc, en, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(call(5, 5, b1, b2, g_sm, kOpen, -1, sc, en, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(call(5, 5, b1, b2, g_sm, kOpen, 128, sc, en, mv, st) == SWMI_ERR_DOMAIN);
        CHECK(call(5, 5, b1, b2, g_sm, 0, 127, sc, en, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT);      // moves without steps
        CHECK(call(5, 5, b1, b2, g_sm, 127, 0, sc, en, nullptr, st) == SWMI_ERR_INVALID_ARGUMENT);      // steps without moves
        CHECK(call(5, 5, nullptr, b2, g_sm, kOpen, kExtend, sc, en, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 5, b1, nullptr, g_sm, kOpen, kExtend, sc, en, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 5, b1, b2, g_sm, kOpen, kExtend, nullptr, en, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(call(5, 5, b1, b2, g_sm, kOpen, kExtend, sc, nullptr, mv, st) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(swmi_local_full_affine_device(b1, 5, b2, 0, 1, g_sm, kOpen, kExtend, sc, en, nullptr, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        CHECK(swmi_local_full_affine_device(b1, 5, b2, 5, 1, g_sm, kOpen, 300, sc, en, nullptr, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(call(5, 5, nullptr, nullptr, g_sm, kOpen, kExtend, nullptr, nullptr, nullptr, nullptr, 0) == SWMI_OK);   // n = 0
        CHECK(swmi_local_full_affine_device(nullptr, 5, nullptr, 5, 0, g_sm, kOpen, kExtend, nullptr, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
        CHECK(fake_hip_log_size() == 0);
        printf("  argument checks and n = 0 without a device: ok\n");

        // slices, with the kernel's own code size: 16 waves x 4112 trips x 256 qwords = 128.5 MiB of codes per full-size alignment
        g_real_sizes = true;
        const Shape full = shape(16384, 16384);
        CHECK(swmi::local_full_affine_code_qwords(16384, 16384) * 8 == (size_t(257) << 19));
        CHECK((slices(full, 257, true) == std::vector<size_t>{256, 1}) && (slices(full, 256, true) == std::vector<size_t>{256}));
        CHECK((slices(full, 600, true) == std::vector<size_t>{256, 256, 88}) && slices(full, 0, true).empty());
        const size_t per = 16384 + 16384 + 4 + 16;                        // ends-only: inputs, score, four ends
        const std::vector<size_t> eo = slices(full, 20000, false);
        CHECK(eo.size() == 3 && eo[0] == (size_t(256) << 20) / per && eo[0] == 8187 && eo[1] == 8187 && eo[2] == 20000 - 2 * 8187);
        // 4096 x 4096 with traceback: 4 waves x 1040 trips x 256 qwords of codes, 256 move words
        const size_t one = 4096 + 4096 + 4 + 16 + size_t(4) * 1040 * 256 * 8 + 256 * 8 + 4;
        const size_t budget = 256 * (16384 + 16384 + 4 + 16 + size_t(16) * 4112 * 256 * 8 + 1024 * 8 + 4);
        CHECK(slices(shape(4096, 4096), 1000000, true)[0] == budget / one);
        CHECK((slices(shape(1, 1), 3 * (size_t(1) << 20) + 5, false) == std::vector<size_t>{size_t(1) << 20, size_t(1) << 20, size_t(1) << 20, 5}));
        CHECK(slices(shape(1, 1), (size_t(1) << 20) + 1, true).size() == 2);
        CHECK(swmi_local_full_affine_slices_for(10, 0, 5, 1, nullptr, 0) == 0 && swmi_local_full_affine_slices_for(10, 5, 16385, 1, nullptr, 0) == 0);
        g_real_sizes = false;
        CHECK(fake_hip_log_size() == 0);
        printf("  slices_for against hand-computed sizes, no device: ok\n");
    }
    CHECK(swmi_init(0) == SWMI_OK);
    const Shape tb_a = shape(300, 777), eo_a = shape(4, 1);

    // host entry: n = 1, one slice, one slice + 1, two and a half slices
    for (const Shape *a : {&tb_a, &eo_a}) {
        const bool tb = a == &tb_a;
        const size_t s = full_slice(*a, tb);
        CHECK(s > 1);
        for (size_t n : {size_t(1), s, s + 1, 2 * s + s / 2}) host_case(*a, n, tb);
    }

    // device entry on two streams; the second call on stream A grows its workspace (after synchronising that stream)
    hipStream_t sa, sb;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    fake_hip_log_clear();
    CHECK(hipStreamSynchronize(sa) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess);
    int ida = 0, idb = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &ida) == 1 && sscanf(fake_hip_log_at(1), "dev0 stream_sync stream%d", &idb) == 1);
    const size_t s = full_slice(tb_a, true), big = 2 * s + s / 2;
    CHECK(has(device_case(tb_a, 3, true, sa), workspace_malloc(tb_a, 3)));
    CHECK(has(device_case(tb_a, big, true, sb), workspace_malloc(tb_a, big)));
    std::vector<std::string> log = device_case(tb_a, big, true, sa);
    CHECK(log.size() >= 2 && log[0] == "dev0 stream_sync stream" + std::to_string(ida) && log[1] == workspace_malloc(tb_a, big));
    log = device_case(tb_a, 5, true, sb);                       // fits: no synchronisation, no allocation
    CHECK(!has(log, "dev0 stream_sync stream" + std::to_string(idb)) && !has(log, workspace_malloc(tb_a, big)));
    log = device_case(eo_a, 7, false, sa);                      // ends-only: no workspace, nothing but the launch
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
    CHECK(swmi_local_full_affine_time_device(d[0], tb_a.len1, d[1], tb_a.len2, n, g_sm, kOpen, kExtend, d[2], d[3], d[4], d[5], sb, 4, &ms) == SWMI_OK);
    CHECK(ms == 0.25f && take_launches().size() == 5);
    printf("  timer: 1 + 4 launches, %.2f ms each: ok\n", ms);

    // the release frees the workspaces and the host sets; the next calls allocate them again
    CHECK(swmi_local_full_affine_release_workspaces() == SWMI_OK);
    CHECK(has(device_case(tb_a, 5, true, sb), workspace_malloc(tb_a, 5)));
    host_case(tb_a, s + 1, true);
    CHECK(swmi_local_full_affine_release_workspaces() == SWMI_OK);
    printf("  release_workspaces, then both entries again: ok\n");

    for (void *p : d) CHECK(hipFree(p) == hipSuccess);
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    CHECK(swmi_shutdown() == SWMI_OK);
    // after the shutdown: argument errors and n = 0 as before, a real call reports that nothing is initialised, the
    // release and the slice arithmetic need no device
    {
        uint8_t b1[8] = {0}, b2[8] = {0};
        int32_t sc[1], en[4];
        CHECK(swmi_local_full_affine(b1, 5, b2, 5, 0, g_sm, kOpen, kExtend, sc, en, nullptr, nullptr) == SWMI_OK);
        CHECK(swmi_local_full_affine(b1, 5, b2, 5, 1, g_sm, kOpen, 200, sc, en, nullptr, nullptr) == SWMI_ERR_DOMAIN);
        CHECK(swmi_local_full_affine(b1, 5, b2, 5, 1, g_sm, kOpen, kExtend, sc, en, nullptr, nullptr) == SWMI_ERR_NOT_INITIALIZED);
        CHECK(swmi_local_full_affine_device(b1, 5, b2, 5, 1, g_sm, kOpen, kExtend, sc, en, nullptr, nullptr, nullptr) == SWMI_ERR_NOT_INITIALIZED);
        CHECK(slices(tb_a, 10, true).size() == 1);
        printf("  after swmi_shutdown: ok\n");
    }
    printf("local_full_affine host fake ok\n");
    return 0;
}
