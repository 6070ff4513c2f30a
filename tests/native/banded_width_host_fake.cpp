// banded_width_host_fake.cpp -- TEST ONLY: the host side of libswmi_banded_width.so (csrc/banded_width_api.cpp) on the fake GPU
// of fake_hip.cpp, as a stand-alone program under ASan + UBSan, in the pattern of banded_ragged_host_fake.cpp.  This file holds
// the stand-in for what banded_width_api.cpp takes from the library's kernel file -- the launcher -- and hipGetDevice.  The
// stand-in knows the batch and the band of the entry call that is running and checks per launch: the band arrives as given;
// the slots, the sequences, the codes AT THE WIDTH'S SIZE, the moves and the results lie inside live device blocks (a
// device-to-device copy of the range onto itself: fake_hip.cpp aborts on a range outside a block); every slot names an
// alignment of the slice once, with that alignment's offsets, lengths, move offset and clamped diagonal; code offsets are the
// running sum of the width's code sizes in slot order, so no two ranges overlap; the slots are in the planner's order by the
// WIDTH'S swept rows (the key itself is held against values worked out by hand, swept_rows_by_hand).  It then writes for caller index c with clamped diagonal d: score = 3 c + d + band + 7000000 free_ends +
// 300000000 kind, ends = (score + 1 .. score + 4), and with a traceback steps = c % 5 (0 for an empty moves row) and every
// move word w of its row = 0xC0DE << 48 | c << 8 | (w & 255).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swmi_banded_width.h"
#include "../../smith-waterman-simd_amd/csrc/banded_internal.h"

using swmi::banded::RaggedSlot;

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t k);
extern "C" void fake_hip_log_clear();

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
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

struct Batch {
    size_t n = 0;
    std::vector<uint64_t> off1{0}, off2{0}, mo{0};
    std::vector<uint8_t> a, b;
    std::vector<int32_t> d;
    void add(size_t len1, size_t len2, int32_t diag)
    {
        const size_t c = n++;
        a.insert(a.end(), len1, 3);
        b.insert(b.end(), len2, 2);
        if (len1) a[off1.back()] = uint8_t(c * 7);
        if (len2) b[off2.back()] = uint8_t(c / 3);
        off1.push_back(a.size());
        off2.push_back(b.size());
        mo.push_back(mo.back() + SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2));
        d.push_back(diag);
    }
    size_t len1(size_t c) const { return size_t(off1[c + 1] - off1[c]); }
    size_t len2(size_t c) const { return size_t(off2[c + 1] - off2[c]); }
};

int32_t clamped(int32_t d) { return std::max(-65536, std::min(65536, d)); }

struct Launch {
    int kind, band;
    size_t n, base;
    bool tb;
    unsigned free_ends;
    const void *codes;
    hipStream_t stream;
    bool reordered;                   // the planner moved a slot
};
std::vector<Launch> g_launches;
const Batch *g_batch = nullptr;       // the batch of the entry call that is running
int g_band = 0;                       // ... and its band
size_t g_base = 0;                    // the caller index of the next launch's first alignment

void in_block(const void *p, size_t bytes)
{
    if (bytes && hipMemcpy(const_cast<void *>(p), p, bytes, hipMemcpyDeviceToDevice) != hipSuccess) abort();
}

size_t count_log(const char *needle)
{
    size_t c = 0;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) c += std::strstr(fake_hip_log_at(k), needle) != nullptr;
    return c;
}

int expected_score(size_t c, int32_t d, int band, unsigned free_ends, int kind)
{
    return int(3 * c) + d + band + 7000000 * int(free_ends) + 300000000 * kind;
}

// the header's code bytes, by hand: band / 128 bytes per lane and iteration, 64 lanes, whole trips of four iterations
size_t code_bytes(int kind, size_t len1, int band) { return size_t(band / 128) * 256 * ((len1 + (kind ? 64 : 63) + 3) / 4); }

}  // namespace

hipError_t swmi::banded::launch_banded_width(int kind, int band, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n,
                                             const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                             unsigned char *codes, unsigned long long *moves, uint32_t *steps, hipStream_t stream)
{
    const Batch &t = *g_batch;
    const bool tb = moves != nullptr;
    const size_t base = g_base;
    EXPECT(band == g_band);                                                      // the band reaches the launcher
    EXPECT(n >= 1 && base + n <= t.n);
    if (base + n > t.n) abort();
    EXPECT((steps != nullptr) == tb && (codes != nullptr) == tb);
    EXPECT(gap_open == 7 && gap_extend == 3 && sm[0] == 2 && sm[1] == -3);
    in_block(slots, n * sizeof(RaggedSlot));
    in_block(s1, size_t(t.off1[base + n] - t.off1[base]));
    in_block(s2, size_t(t.off2[base + n] - t.off2[base]));
    in_block(scores, n * 4);
    in_block(ends, n * 16);
    size_t code_total = 0;
    for (size_t c = base; c < base + n; ++c) code_total += code_bytes(kind, t.len1(c), band);
    if (tb) {
        in_block(codes, code_total);                                             // the slice's codes at the width's size
        in_block(moves, size_t(t.mo[base + n] - t.mo[base]) * 8);
        in_block(steps, n * 4);
        EXPECT((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
    }
    std::vector<char> seen(n, 0);
    uint64_t code_at = 0;
    int last_rows = 1 << 30;
    uint32_t last_index = 0;
    bool reordered = false;
    for (size_t x = 0; x < n; ++x) {
        const RaggedSlot &q = slots[x];
        EXPECT(q.index < n);
        if (q.index >= n) break;
        EXPECT(!seen[q.index]);                                                  // every alignment of the slice once
        seen[q.index] = 1;
        reordered |= q.index != x;
        const size_t c = base + q.index;
        EXPECT(q.off1 == t.off1[c] - t.off1[base] && q.off2 == t.off2[c] - t.off2[base]);
        EXPECT(size_t(q.len1) == t.len1(c) && size_t(q.len2) == t.len2(c));
        EXPECT(q.d0 == clamped(t.d[c]));
        if (q.len1) EXPECT(s1[q.off1] == uint8_t(c * 7));
        if (q.len2) EXPECT(s2[q.off2] == uint8_t(c / 3));
        if (tb) {
            EXPECT(q.move_off == t.mo[c] - t.mo[base]);
            EXPECT(q.code_off == code_at);                                       // a running sum in slot order: pairwise disjoint
            EXPECT(q.code_off % (16 * size_t(band / 128)) == 0);                 // a lane's trip is whole stores
            code_at += code_bytes(kind, size_t(q.len1), band) / 4;
            EXPECT(code_at * 4 <= code_total);
        }
        // the planner's order: the width's swept rows descending, ties in caller order
        const int rows = swmi::banded::width_swept_rows(kind, q.len1, q.len2, q.d0, band);
        EXPECT(rows >= 0 && rows <= last_rows);
        if (x && rows == last_rows) EXPECT(q.index > last_index);
        last_rows = rows;
        last_index = q.index;
        const int32_t score = expected_score(c, q.d0, band, free_ends, kind);
        scores[q.index] = score;
        for (int e = 0; e < 4; ++e) ends[4 * q.index + e] = score + 1 + e;
        if (tb) {
            const size_t mw = size_t(t.mo[c + 1] - t.mo[c]);
            steps[q.index] = mw ? uint32_t(c % 5) : 0u;
            for (size_t w = 0; w < mw; ++w) moves[q.move_off + w] = 0xC0DEull << 48 | (unsigned long long)c << 8 | (w & 255);
        }
        if (g_failed) break;
    }
    g_launches.push_back({kind, band, n, base, tb, free_ends, codes, stream, reordered});
    g_base = base + n == t.n ? 0 : base + n;                                     // (the timer runs the call again)
    return hipSuccess;
}

namespace {

const int8_t kSm[16] = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};

void check_results(const Batch &t, int band, bool tb, unsigned mask, int kind, const int32_t *scores, const int32_t *ends, const uint64_t *moves,
                   const uint32_t *steps)
{
    for (size_t c = 0; c < t.n; ++c) {
        const int score = expected_score(c, clamped(t.d[c]), band, kind == SWMI_BANDED_WIDTH_GLOBAL ? mask : 0u, kind);
        EXPECT(scores[c] == score);
        for (int e = 0; e < 4; ++e) EXPECT(ends[4 * c + e] == score + 1 + e);
        if (tb) {
            const size_t mw = size_t(t.mo[c + 1] - t.mo[c]);
            EXPECT(steps[c] == (mw ? uint32_t(c % 5) : 0u));
            if (mw) EXPECT(moves[t.mo[c]] == (0xC0DEull << 48 | (unsigned long long)c << 8) && moves[t.mo[c + 1] - 1] == (moves[t.mo[c]] | ((mw - 1) & 255)));
        }
        if (g_failed) break;
    }
}

// a host call; the slices are the header's, every launch carries the band, the results land at the caller's positions, and
// the sentinels behind every output array are untouched
void host_case(const char *name, int kind, int band, const Batch &t, bool tb, unsigned mask, size_t want_slices)
{
    std::vector<int32_t> scores(t.n + 1, -77), ends(4 * t.n + 1, -77);
    std::vector<uint64_t> moves(tb ? size_t(t.mo[t.n]) + 1 : 1, 0x5E5E5E5Eull);
    std::vector<uint32_t> steps(tb ? t.n + 1 : 1, 0x5E5Eu);
    std::vector<size_t> sizes(8, 0);
    const size_t slices = swmi_banded_width_slices_for(kind, band, t.off1.data(), t.off2.data(), t.n, tb, sizes.data(), sizes.size());
    EXPECT(slices == want_slices);
    g_launches.clear();
    g_batch = &t;
    g_band = band;
    g_base = 0;
    const uint8_t none = 0;
    const uint8_t *a = t.a.empty() ? &none : t.a.data(), *b = t.b.empty() ? &none : t.b.data();
    int rc;
    if (kind == SWMI_BANDED_WIDTH_GLOBAL)
        rc = swmi_banded_width_global(a, t.off1.data(), b, t.off2.data(), t.n, t.d.data(), band, kSm, 7, 3, mask, scores.data(), ends.data(),
                                      tb ? moves.data() : nullptr, tb ? steps.data() : nullptr);
    else
        rc = swmi_banded_width_local(a, t.off1.data(), b, t.off2.data(), t.n, t.d.data(), band, kSm, 7, 3, scores.data(), ends.data(),
                                     tb ? moves.data() : nullptr, tb ? steps.data() : nullptr);
    EXPECT(rc == SWMI_OK);
    EXPECT(g_launches.size() == slices);
    size_t total = 0;
    for (size_t s = 0; s < g_launches.size(); ++s) {
        const Launch &l = g_launches[s];
        EXPECT(l.kind == kind && l.band == band && l.n == sizes[s] && l.base == total && l.tb == tb && l.stream != nullptr);
        EXPECT(l.free_ends == (kind == SWMI_BANDED_WIDTH_GLOBAL ? mask : 0u));
        if (s > 0) EXPECT(l.stream != g_launches[s - 1].stream);                      // two sets in turn
        total += l.n;
    }
    EXPECT(total == t.n);
    check_results(t, band, tb, mask, kind, scores.data(), ends.data(), moves.data(), steps.data());
    EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves.back() == 0x5E5E5E5Eull && steps.back() == 0x5E5Eu);
    std::printf("%s: %s\n", name, g_failed ? "FAILED" : "ok");
}

// mixed shapes: lengths 0 .. top, diagonals that keep, shift and lose the band, INT32 extremes among them
Batch mixed(size_t n, size_t top)
{
    Batch t;
    for (size_t k = 0; k < n; ++k) {
        const size_t len1 = (k * 37 + 5) % (top + 1), len2 = (k * 53 + 11) % (top + 1);
        const int32_t diag = k % 13 == 0 ? INT32_MIN : k % 13 == 1 ? INT32_MAX : k % 13 == 2 ? 70000 : int32_t(k % 11) * 90 - 450;
        t.add(len1, len2, diag);
    }
    return t;
}

// the device entries: a workspace of the width's codes and the slots, reused; the timer's 1 + iters launches
void device_case(int band)
{
    const Batch t = mixed(41, 700);
    hipStream_t s;
    EXPECT(hipStreamCreateWithFlags(&s, 0) == hipSuccess);
    void *d1, *d2, *ds, *de, *dm, *dt;
    EXPECT(hipMalloc(&d1, t.a.size() + 16) == hipSuccess && hipMalloc(&d2, t.b.size() + 16) == hipSuccess);
    EXPECT(hipMalloc(&ds, (t.n + 1) * 4) == hipSuccess && hipMalloc(&de, (4 * t.n + 1) * 4) == hipSuccess &&
           hipMalloc(&dm, (size_t(t.mo[t.n]) + 1) * 8) == hipSuccess && hipMalloc(&dt, (t.n + 1) * 4) == hipSuccess);
    std::memcpy(d1, t.a.data(), t.a.size());
    std::memcpy(d2, t.b.data(), t.b.size());
    int32_t *scores = static_cast<int32_t *>(ds), *ends = static_cast<int32_t *>(de);
    uint64_t *moves = static_cast<uint64_t *>(dm);
    uint32_t *steps = static_cast<uint32_t *>(dt);
    scores[t.n] = ends[4 * t.n] = -77;
    moves[t.mo[t.n]] = 0x5E5E5E5Eull;
    steps[t.n] = 0x5E5Eu;
    g_launches.clear();
    fake_hip_log_clear();
    g_batch = &t;
    g_band = band;
    g_base = 0;
    EXPECT(swmi_banded_width_global_device(d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), band, kSm, 7, 3, 19u, ds, de, dm, dt, s) == SWMI_OK);
    EXPECT(g_launches.size() == 1 && g_launches[0].stream == s && g_launches[0].n == t.n && g_launches[0].band == band);
    size_t codes = 0;
    for (size_t c = 0; c < t.n; ++c) codes += code_bytes(1, t.len1(c), band);
    char want[64];
    std::snprintf(want, sizeof want, "malloc bytes%zu", codes + t.n * sizeof(RaggedSlot));
    EXPECT(count_log(want) == 1 && count_log("malloc") == 1);                   // one workspace: the width's codes and the slots
    check_results(t, band, true, 19u, 1, scores, ends, moves, steps);
    fake_hip_log_clear();
    EXPECT(swmi_banded_width_local_device(d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), band, kSm, 7, 3, ds, de, nullptr, nullptr, s) == SWMI_OK);
    check_results(t, band, false, 0u, 0, scores, ends, moves, steps);
    float ms = -1.f;
    EXPECT(swmi_banded_width_time_device(SWMI_BANDED_WIDTH_LOCAL, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), band, kSm, 7, 3, 77u, ds, de,
                                         dm, dt, s, 3, &ms) == SWMI_OK && ms > 0.f);
    EXPECT(g_launches.size() == 2 + 4 && count_log("malloc") == 0);             // the local kind's codes fit the global kind's
    for (size_t k = 2; k < g_launches.size(); ++k) EXPECT(g_launches[k].band == band && g_launches[k].free_ends == 0u);
    EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves[t.mo[t.n]] == 0x5E5E5E5Eull && steps[t.n] == 0x5E5Eu);
    for (void *p : {d1, d2, ds, de, dm, dt}) EXPECT(hipFree(p) == hipSuccess);
    EXPECT(swmi_banded_width_release_workspaces() == SWMI_OK);
    EXPECT(hipStreamDestroy(s) == hipSuccess);
    std::printf("device entries, band %d: %s\n", band, g_failed ? "FAILED" : "ok");
}

void refusals()
{
    int32_t out[8];
    uint64_t mv[4];
    uint32_t st[4];
    alignas(16) const uint8_t seq[16] = {};
    const uint64_t good[3] = {0, 4, 8}, bad[3] = {0, 4, 3};
    float ms;
    fake_hip_log_clear();
    g_launches.clear();
    auto text = [](const char *needle) { return std::string(swmi_banded_width_last_error()).find(needle) != std::string::npos; };
    // the band before everything else: each call also breaks every later rule
    for (int band : {0, -128, 64, 127, 129, 192, 384, 768, 2048, 1 << 30}) {
        EXPECT(swmi_banded_width_global(nullptr, bad, nullptr, bad, 2, nullptr, band, nullptr, 200, 1, 20u, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(swmi_banded_width_local(nullptr, bad, nullptr, bad, 2, nullptr, band, nullptr, 200, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(swmi_banded_width_local_device(seq + 1, bad, seq, bad, 0, nullptr, band, nullptr, 200, 1, out, out, mv, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(swmi_banded_width_time_device(2, seq, good, seq, good, 2, nullptr, band, kSm, 1, 1, 0u, out, out, mv, st, nullptr, 0, &ms) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(swmi_banded_width_slices_for(SWMI_BANDED_WIDTH_LOCAL, band, good, good, 2, 1, nullptr, 0) == 0 && text("band"));
    }
    // then the ragged header's order
    EXPECT(swmi_banded_width_global(nullptr, bad, nullptr, bad, 2, nullptr, 256, nullptr, 200, 1, 20u, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("free_ends 20"));
    EXPECT(swmi_banded_width_local(nullptr, bad, nullptr, bad, 2, nullptr, 256, nullptr, 200, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("score_matrix"));
    EXPECT(swmi_banded_width_local(nullptr, bad, nullptr, bad, 2, nullptr, 512, kSm, 200, 1, out, out, mv, nullptr) == SWMI_ERR_DOMAIN && text("outside [0,127]"));
    EXPECT(swmi_banded_width_local(nullptr, bad, nullptr, bad, 0, nullptr, 1024, kSm, 1, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("moves and steps"));
    EXPECT(swmi_banded_width_local(nullptr, nullptr, nullptr, nullptr, 0, nullptr, 1024, kSm, 1, 1, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
    EXPECT(swmi_banded_width_local(nullptr, bad, seq, bad, 2, nullptr, 128, kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("NULL buffer"));
    EXPECT(swmi_banded_width_local(seq, good, seq, bad, 2, nullptr, 128, kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("decrease"));
    EXPECT(swmi_banded_width_local_device(seq + 1, good, seq, good, 2, nullptr, 256, kSm, 1, 1, out, out, mv, st, nullptr) == SWMI_ERR_ALIGNMENT);
    EXPECT(fake_hip_log_size() == 0 && g_launches.empty());                       // no device was touched
    std::printf("refusals: %s\n", g_failed ? "FAILED" : "ok");
}

}  // namespace

// The planner's key against values worked out by hand from -band/2 <= j - i - d0 <= band/2 - 1 (the launcher's stand-in checks
// the order against the key itself).  Rows i_lo .. i_hi, the key is i_hi - i_lo:
//   (300, 300), d0 = -560, local:  i_lo = 2 - band/2 + 560 = 498, 434, 306 > 300: no row;  at 1024  50 .. 300
//   (300, 300), d0 = -100, local:  i_lo = max(1, 102 - band/2) = 38, 1, 1, 1;  i_hi = 300
//   (300, 300), d0 = -100, global: i_lo = max(0, 101 - band/2) = 37, 0, 0, 0;  i_hi = 300
//   (300, 250), d0 = +200:         i_hi = min(300, 50 + band/2) = 114, 178, 300, 300;  i_lo = 1 local, 0 global
void swept_rows_by_hand()
{
    using swmi::banded::width_swept_rows;
    const int bands[4] = {128, 256, 512, 1024};
    const int far[4] = {0, 0, 0, 250}, low_local[4] = {262, 299, 299, 299}, low_global[4] = {263, 300, 300, 300};
    const int high_local[4] = {113, 177, 299, 299}, high_global[4] = {114, 178, 300, 300};
    for (int x = 0; x < 4; ++x) {
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_LOCAL, 300, 300, -560, bands[x]) == far[x]);
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_LOCAL, 300, 300, -100, bands[x]) == low_local[x]);
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_GLOBAL, 300, 300, -100, bands[x]) == low_global[x]);
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_LOCAL, 300, 250, 200, bands[x]) == high_local[x]);
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_GLOBAL, 300, 250, 200, bands[x]) == high_global[x]);
        EXPECT(width_swept_rows(SWMI_BANDED_WIDTH_GLOBAL, 0, 250, 0, bands[x]) == 0 && width_swept_rows(SWMI_BANDED_WIDTH_LOCAL, 9, 0, 0, bands[x]) == 0);
    }
    std::printf("swept rows by hand: %s\n", g_failed ? "FAILED" : "ok");
}

int main()
{
    EXPECT(swmi_banded_width_version() == SWMI_VERSION);
    refusals();
    swept_rows_by_hand();
    // traceback, one slice, mixed shapes, both kinds, every width; the planner has work to do at every width
    for (int band : {128, 256, 512, 1024}) {
        char name[64];
        std::snprintf(name, sizeof name, "traceback, local, band %d", band);
        host_case(name, SWMI_BANDED_WIDTH_LOCAL, band, mixed(203, 900), true, 0u, 1);
        EXPECT(g_launches.size() == 1 && g_launches[0].reordered);
        std::snprintf(name, sizeof name, "traceback, global, band %d", band);
        host_case(name, SWMI_BANDED_WIDTH_GLOBAL, band, mixed(57, 300), true, 15u, 1);
        device_case(band);
    }
    // the planner's key is the width's: (300, 300) at diagonal -560 misses a band of 128 .. 512 (its first row would be
    // 2 - band / 2 + 560 > 300) and has rows 50 .. 300 at 1024, so it stays behind (100, 100) at 0 (99 rows) at the narrow
    // widths and goes in front of it at 1024
    for (int band : {128, 512, 1024}) {
        Batch t;
        t.add(100, 100, 0), t.add(300, 300, -560);
        host_case("planner key", SWMI_BANDED_WIDTH_LOCAL, band, t, true, 0u, 1);
        EXPECT(g_launches.size() == 1 && g_launches[0].reordered == (band == 1024));
    }
    // two ends-only slices, the second one ragged: the count cap of 2^20 on tiny mixed shapes (the width does not enter)
    host_case("two ends-only slices", SWMI_BANDED_WIDTH_GLOBAL, 512, mixed((size_t(1) << 20) + 5, 2), false, 10u, 2);
    // empty sequences on either side and both
    {
        Batch t;
        t.add(0, 5, 0), t.add(5, 0, 3), t.add(0, 0, 0), t.add(7, 9, -2), t.add(0, 16384, 70), t.add(16384, 0, -70), t.add(0, 0, INT32_MAX);
        host_case("empty sequences", SWMI_BANDED_WIDTH_GLOBAL, 256, t, true, 3u, 1);
    }
    EXPECT(swmi_banded_width_release_workspaces() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("banded width host fake ok\n");
    return 0;
}
