// banded_ragged_host_fake.cpp -- TEST ONLY: the host side of libswmi_banded_ragged.so and, compiled with
// -DSWMI_BANDED_WIDTH_LIBRARY like the source under test, of libswmi_banded_width.so (csrc/banded_ragged_api.cpp, DESIGN.md
// section 39) on the fake GPU of fake_hip.cpp, as a stand-alone program under ASan + UBSan.  This file holds the stand-in for
// what the source takes from the library's kernel file -- the launcher -- and hipGetDevice.  The stand-in knows the batch and the
// band of the entry call that is running and which caller index the launch's first alignment has, and checks per launch: the
// band arrives as given (128 in the ragged build, which has no band to give); the slots, the sequences, the codes AT THE
// WIDTH'S SIZE, the moves and the results lie inside live device blocks for the sizes the kernels touch (a device-to-device copy
// of the range onto itself: fake_hip.cpp aborts on a range outside a block; every slot's range is shown to lie inside the range
// copied); every slot names an alignment of the slice once, with that alignment's offsets, lengths, move offset and CLAMPED
// diagonal, and its sequence starts with that alignment's marker bytes; code offsets are the running sum of the width's code
// sizes (written out by hand, code_bytes) in slot order, so no two overlap, each aligned to a lane's whole stores; the slots are
// in the planner's order by the width's swept rows (the key itself is held against values worked out by hand,
// swept_rows_by_hand); kind, mask, gaps and matrix are recorded for the cases to hold against what they gave.  It then writes
// for caller index c with clamped diagonal d: score = 3 c + d + band + 7000000 free_ends + 300000000 kind, ends = (score + 1 ..
// score + 4), and with a traceback steps = c % 5 (0 for an empty moves row) and every move word w of its row =
// 0xC0DE << 48 | c << 8 | (w & 255).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

// ---- what the two builds differ in: the header, the entries' prefix and their band argument, the widths the cases run at,
// ---- the spread of the mixed batches' diagonals, the closing line, and which launcher the stand-in is ----
#ifdef SWMI_BANDED_WIDTH_LIBRARY
#include "../../include/swmi_banded_width.h"
#define BANDED(name) swmi_banded_width_##name
#define BAND(band) band,
constexpr bool kHasBand = true;
constexpr int kLocal = SWMI_BANDED_WIDTH_LOCAL, kGlobal = SWMI_BANDED_WIDTH_GLOBAL;
constexpr std::initializer_list<int> kBands = {128, 256, 512, 1024};
constexpr int kDiagStep = 90;
const char *const kClosing = "banded width host fake ok";
#else
#include "../../include/swmi_banded_ragged.h"
#define BANDED(name) swmi_banded_ragged_##name
#define BAND(band)
constexpr bool kHasBand = false;
constexpr int kLocal = SWMI_BANDED_RAGGED_LOCAL, kGlobal = SWMI_BANDED_RAGGED_GLOBAL;
constexpr std::initializer_list<int> kBands = {128};
constexpr int kDiagStep = 9;
const char *const kClosing = "banded ragged host fake ok";
#endif
#include "../../smith-waterman-simd_amd/csrc/banded_internal.h"

using swmi::banded::RaggedSlot;

static hipError_t fake_launch(int kind, int band, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n, const int8_t *sm,
                              int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes,
                              unsigned long long *moves, uint32_t *steps, hipStream_t stream);
#ifdef SWMI_BANDED_WIDTH_LIBRARY
hipError_t swmi::banded::launch_banded_width(int kind, int band, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n,
                                             const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                             unsigned char *codes, unsigned long long *moves, uint32_t *steps, hipStream_t stream)
{
    return fake_launch(kind, band, s1, s2, slots, n, sm, gap_open, gap_extend, free_ends, scores, ends, codes, moves, steps, stream);
}
#else
hipError_t swmi::banded::launch_banded_ragged(int kind, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n, const int8_t *sm,
                                              int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                              unsigned char *codes, unsigned long long *moves, uint32_t *steps, hipStream_t stream)
{
    return fake_launch(kind, swmi::banded::kBandWidth, s1, s2, slots, n, sm, gap_open, gap_extend, free_ends, scores, ends, codes, moves, steps,
                       stream);
}
#endif
// ---- below this line the two builds are one text ----

// the width a case runs at: the one it names in the width build, 128 in the ragged build
constexpr int at(int band) { return kHasBand ? band : swmi::banded::kBandWidth; }

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
    int open, extend, sm_sum;
    unsigned free_ends;
    const void *codes, *slots;
    hipStream_t stream;
    bool reordered;                   // the planner moved a slot
};
std::vector<Launch> g_launches;
const Batch *g_batch = nullptr;       // the batch of the entry call that is running
int g_band = 0;                       // ... its band
bool g_diag = true;                   // ... called with its diagonals
size_t g_base = 0;                    // the caller index of the next launch's first alignment

void running(const Batch &t, int band, bool with_diag)
{
    g_batch = &t;
    g_band = band;
    g_diag = with_diag;
    g_base = 0;
}

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

// the headers' code bytes, by hand: band / 128 bytes per lane and iteration, 64 lanes, whole trips of four iterations
size_t code_bytes(int kind, size_t len1, int band) { return size_t(band / 128) * 256 * ((len1 + (kind ? 64 : 63) + 3) / 4); }

}  // namespace

static hipError_t fake_launch(int kind, int band, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n, const int8_t *sm,
                              int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes,
                              unsigned long long *moves, uint32_t *steps, hipStream_t stream)
{
    const Batch &t = *g_batch;
    const bool tb = moves != nullptr;
    const size_t base = g_base;
    EXPECT(band == g_band);                                                      // the band reaches the launcher
    EXPECT(n >= 1 && base + n <= t.n);
    if (base + n > t.n) abort();
    EXPECT((steps != nullptr) == tb && (codes != nullptr) == tb);
    // the ranges a launch of these n alignments may touch
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
    int sum = 0;
    for (int x = 0; x < 16; ++x) sum += sm[x] * (x + 1);
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
        // the slot is that alignment's, slice-relative, so every range below lies inside the ranges copied above
        EXPECT(q.off1 == t.off1[c] - t.off1[base] && q.off2 == t.off2[c] - t.off2[base]);
        EXPECT(size_t(q.len1) == t.len1(c) && size_t(q.len2) == t.len2(c));
        EXPECT(q.d0 == (g_diag ? clamped(t.d[c]) : 0));                          // the caller's diagonal, clamped
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
    g_launches.push_back({kind, band, n, base, tb, gap_open, gap_extend, sum, free_ends, codes, slots, stream, reordered});
    g_base = base + n == t.n ? 0 : base + n;                                     // (the timer runs the call again)
    return hipSuccess;
}

namespace {

const int8_t kSm[16] = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};
int sm_sum()
{
    int s = 0;
    for (int x = 0; x < 16; ++x) s += kSm[x] * (x + 1);
    return s;
}

void check_results(const Batch &t, int band, bool with_diag, bool tb, unsigned mask, int kind, const int32_t *scores, const int32_t *ends,
                   const uint64_t *moves, const uint32_t *steps)
{
    for (size_t c = 0; c < t.n; ++c) {
        const int score = expected_score(c, with_diag ? clamped(t.d[c]) : 0, band, kind == kGlobal ? mask : 0u, kind);
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

// a host call: the slices are the header's, every launch carries the call's band, kind, mask, gaps and matrix, two buffer sets
// take the slices in turn, the copies are the slices', the results land at the caller's positions, and the sentinels behind
// every output array are untouched
void host_case(const char *name, int kind, int band, const Batch &t, bool with_diag, bool tb, unsigned mask, size_t want_slices)
{
    std::vector<int32_t> scores(t.n + 1, -77), ends(4 * t.n + 1, -77);
    std::vector<uint64_t> moves(tb ? size_t(t.mo[t.n]) + 1 : 1, 0x5E5E5E5Eull);
    std::vector<uint32_t> steps(tb ? t.n + 1 : 1, 0x5E5Eu);
    std::vector<size_t> sizes(8, 0);
    const size_t slices = BANDED(slices_for)(kind, BAND(band) t.off1.data(), t.off2.data(), t.n, tb, sizes.data(), sizes.size());
    EXPECT(slices == want_slices);
    g_launches.clear();
    fake_hip_log_clear();
    running(t, band, with_diag);
    const uint8_t none = 0;
    const uint8_t *a = t.a.empty() ? &none : t.a.data(), *b = t.b.empty() ? &none : t.b.data();
    const int32_t *dg = with_diag ? t.d.data() : nullptr;
    uint64_t *mv = tb ? moves.data() : nullptr;
    uint32_t *st = tb ? steps.data() : nullptr;
    if (kind == kGlobal)
        EXPECT(BANDED(global)(a, t.off1.data(), b, t.off2.data(), t.n, dg, BAND(band) kSm, 7, 3, mask, scores.data(), ends.data(), mv, st) == SWMI_OK);
    else
        EXPECT(BANDED(local)(a, t.off1.data(), b, t.off2.data(), t.n, dg, BAND(band) kSm, 7, 3, scores.data(), ends.data(), mv, st) == SWMI_OK);
    EXPECT(g_launches.size() == slices);
    size_t total = 0;
    for (size_t s = 0; s < g_launches.size(); ++s) {
        const Launch &l = g_launches[s];
        EXPECT(l.kind == kind && l.band == band && l.n == sizes[s] && l.base == total && l.tb == tb);
        EXPECT(l.open == 7 && l.extend == 3 && l.sm_sum == sm_sum() && l.stream != nullptr);
        EXPECT(l.free_ends == (kind == kGlobal ? mask : 0u));                         // the mask reaches every launch as given
        if (s > 0) EXPECT(l.stream != g_launches[s - 1].stream);                      // two sets in turn
        if (s > 1) EXPECT(l.stream == g_launches[s - 2].stream);
        total += l.n;
    }
    EXPECT(total == t.n);
    // per slice: the two sequence buffers (none of an empty side) and the slots up; scores, ends (and steps, moves) down
    size_t ups = 0, downs = 0, first = 0;
    for (size_t s = 0; s < slices && s < sizes.size(); first += sizes[s], ++s) {
        ups += 1 + (t.off1[first + sizes[s]] > t.off1[first]) + (t.off2[first + sizes[s]] > t.off2[first]);
        downs += 2 + (tb ? 1 + (t.mo[first + sizes[s]] > t.mo[first]) : 0);
    }
    EXPECT(count_log("memcpy kind1") == ups && count_log("memcpy kind2") == downs);
    check_results(t, band, with_diag, tb, mask, kind, scores.data(), ends.data(), moves.data(), steps.data());
    EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves.back() == 0x5E5E5E5Eull && steps.back() == 0x5E5Eu);
    std::printf("%s, band %d: %s\n", name, band, g_failed ? "FAILED" : "ok");
}

// mixed shapes: lengths 0 .. top, diagonals that keep, shift and lose the band, INT32 extremes among them
Batch mixed(size_t n, size_t top)
{
    Batch t;
    for (size_t k = 0; k < n; ++k) {
        const size_t len1 = (k * 37 + 5) % (top + 1), len2 = (k * 53 + 11) % (top + 1);
        const int32_t diag = k % 13 == 0 ? INT32_MIN : k % 13 == 1 ? INT32_MAX : k % 13 == 2 ? 70000 : int32_t(k % 11) * kDiagStep - 5 * kDiagStep;
        t.add(len1, len2, diag);
    }
    return t;
}

// device calls on two streams of the caller's: a workspace per stream of the width's codes and the slots, reused by the same
// call, and the timer
void device_case(int band)
{
    const Batch small = mixed(23, 60), large = mixed(41, 700);
    hipStream_t st[2];
    EXPECT(hipStreamCreateWithFlags(&st[0], 0) == hipSuccess && hipStreamCreateWithFlags(&st[1], 0) == hipSuccess);
    for (int round = 0; round < 3; ++round) {
        const Batch &t = round == 1 ? large : small;
        const int kind = round == 2 ? kLocal : kGlobal;
        const unsigned mask = round == 0 ? 0u : 19u;
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
        hipStream_t s = st[round == 2 ? 1 : 0];
        auto call = [&](bool with_diag, bool tb, unsigned m) {
            running(t, band, with_diag);
            const int32_t *dg = with_diag ? t.d.data() : nullptr;
            if (kind == kGlobal)
                return BANDED(global_device)(d1, t.off1.data(), d2, t.off2.data(), t.n, dg, BAND(band) kSm, 2, 9, m, ds, de, tb ? dm : nullptr,
                                             tb ? dt : nullptr, s);
            return BANDED(local_device)(d1, t.off1.data(), d2, t.off2.data(), t.n, dg, BAND(band) kSm, 2, 9, ds, de, tb ? dm : nullptr,
                                        tb ? dt : nullptr, s);
        };
        g_launches.clear();
        fake_hip_log_clear();
        EXPECT(call(true, true, mask) == SWMI_OK);
        EXPECT(g_launches.size() == 1 && g_launches[0].stream == s && g_launches[0].n == t.n && g_launches[0].tb && g_launches[0].kind == kind);
        EXPECT(g_launches[0].band == band && g_launches[0].open == 2 && g_launches[0].extend == 9 && g_launches[0].free_ends == (kind ? mask : 0u));
        // rounds 0 and 2 make a stream's first workspace, round 1 outgrows stream 0's: one allocation of the width's codes and the slots each
        size_t codes = 0;
        for (size_t c = 0; c < t.n; ++c) codes += code_bytes(kind, t.len1(c), band);
        char want[64];
        std::snprintf(want, sizeof want, "malloc bytes%zu", codes + t.n * sizeof(RaggedSlot));
        EXPECT(count_log(want) == 1 && count_log("malloc") == 1);
        EXPECT(count_log("memcpy kind1") == 1 && count_log("memcpy kind2") == 0);     // the slots go up; the matrix rides in the launch
        check_results(t, band, true, true, mask, kind, scores, ends, moves, steps);
        // the same call again, without diagonals, and an ends-only call reuse the workspace: no second allocation
        fake_hip_log_clear();
        EXPECT(call(false, true, mask) == SWMI_OK);
        check_results(t, band, false, true, mask, kind, scores, ends, moves, steps);
        EXPECT(call(true, false, 16u) == SWMI_OK);
        check_results(t, band, true, false, 16u, kind, scores, ends, moves, steps);
        EXPECT(count_log("malloc") == 0 && g_launches.size() == 3 && !g_launches[2].tb && g_launches[2].codes == nullptr);
        EXPECT(g_launches[1].codes == g_launches[0].codes && g_launches[1].slots == g_launches[0].slots);
        // the timer: 1 + iters launches
        float ms = -1.f;
        running(t, band, true);
        EXPECT(BANDED(time_device)(kind, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), BAND(band) kSm, 2, 9, mask, ds, de, dm, dt, s, 3,
                                   &ms) == SWMI_OK && ms > 0.f);
        EXPECT(g_launches.size() == 3 + 4 && count_log("malloc") == 0);
        for (size_t k = 3; k < g_launches.size(); ++k)
            EXPECT(g_launches[k].free_ends == (kind ? mask : 0u) && g_launches[k].kind == kind && g_launches[k].band == band);
        // the timer of the local kind behind the global kind's calls: its codes fit theirs, and it drops the mask
        if (kind == kGlobal) {
            EXPECT(BANDED(time_device)(kLocal, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), BAND(band) kSm, 2, 9, 77u, ds, de, dm, dt, s, 3,
                                       &ms) == SWMI_OK && ms > 0.f);
            EXPECT(g_launches.size() == 3 + 4 + 4 && count_log("malloc") == 0);
            for (size_t k = 7; k < g_launches.size(); ++k) EXPECT(g_launches[k].free_ends == 0u && g_launches[k].kind == kLocal && g_launches[k].band == band);
            g_launches.resize(7);
        }
        EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves[t.mo[t.n]] == 0x5E5E5E5Eull && steps[t.n] == 0x5E5Eu);
        // a refused mask reaches no launch and touches no device, through any entry
        fake_hip_log_clear();
        for (unsigned bad : {20u, 24u, 32u, 0xFFFFFFFFu}) {
            EXPECT(BANDED(global_device)(d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), BAND(band) kSm, 2, 9, bad, ds, de, dm, dt, s) ==
                   SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(std::string(BANDED(last_error)()).find("free_ends") != std::string::npos);
            EXPECT(BANDED(time_device)(kGlobal, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), BAND(band) kSm, 2, 9, bad, ds, de, dm, dt, s, 3,
                                       &ms) == SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(BANDED(global)(t.a.data(), t.off1.data(), t.b.data(), t.off2.data(), t.n, t.d.data(), BAND(band) kSm, 2, 9, bad, scores, ends,
                                  nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        }
        EXPECT(g_launches.size() == 3 + 4 && fake_hip_log_size() == 0);
        for (void *p : {d1, d2, ds, de, dm, dt}) EXPECT(hipFree(p) == hipSuccess);
    }
    EXPECT(BANDED(release_workspaces)() == SWMI_OK);
    EXPECT(hipStreamDestroy(st[0]) == hipSuccess && hipStreamDestroy(st[1]) == hipSuccess);
    std::printf("device entries, band %d: %s\n", band, g_failed ? "FAILED" : "ok");
}

void refusals()
{
    int32_t out[8];
    uint64_t mv[4];
    uint32_t st[4];
    alignas(16) const uint8_t seq[16] = {};
    const uint64_t good[3] = {0, 4, 8}, bad[3] = {0, 4, 3}, long_[3] = {0, 4, 4 + 16385};
    fake_hip_log_clear();
    g_launches.clear();
    auto text = [](const char *needle) { return std::string(BANDED(last_error)()).find(needle) != std::string::npos; };
#ifdef SWMI_BANDED_WIDTH_LIBRARY
    // the band before everything else: each call also breaks every later rule
    float ms;
    for (int band : {0, -128, 64, 127, 129, 192, 384, 768, 2048, 1 << 30}) {
        EXPECT(BANDED(global)(nullptr, bad, nullptr, bad, 2, nullptr, band, nullptr, 200, 1, 20u, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(BANDED(local)(nullptr, bad, nullptr, bad, 2, nullptr, band, nullptr, 200, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(BANDED(local_device)(seq + 1, bad, seq, bad, 0, nullptr, band, nullptr, 200, 1, out, out, mv, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(BANDED(time_device)(2, seq, good, seq, good, 2, nullptr, band, kSm, 1, 1, 0u, out, out, mv, st, nullptr, 0, &ms) == SWMI_ERR_INVALID_ARGUMENT && text("band"));
        EXPECT(BANDED(slices_for)(kLocal, band, good, good, 2, 1, nullptr, 0) == 0 && text("band"));
    }
#endif
    // (then) in the ragged header's order: each call also breaks every later rule
    EXPECT(BANDED(global)(nullptr, bad, nullptr, bad, 2, nullptr, BAND(256) nullptr, 200, 1, 20u, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("free_ends 20"));
    EXPECT(BANDED(local)(nullptr, bad, nullptr, bad, 2, nullptr, BAND(256) nullptr, 200, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("score_matrix"));
    EXPECT(BANDED(local)(nullptr, bad, nullptr, bad, 2, nullptr, BAND(512) kSm, 200, 1, out, out, mv, nullptr) == SWMI_ERR_DOMAIN && text("outside [0,127]"));
    EXPECT(BANDED(local)(nullptr, bad, nullptr, bad, 0, nullptr, BAND(1024) kSm, 1, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("moves and steps"));
    EXPECT(BANDED(local)(nullptr, nullptr, nullptr, nullptr, 0, nullptr, BAND(1024) kSm, 1, 1, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
    EXPECT(BANDED(local)(nullptr, bad, seq, bad, 2, nullptr, BAND(128) kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("NULL buffer"));
    EXPECT(BANDED(local)(seq, nullptr, seq, good, 2, nullptr, BAND(128) kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("NULL"));
    EXPECT(BANDED(local)(seq, good, seq, bad, 2, nullptr, BAND(128) kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("decrease"));
    EXPECT(BANDED(global)(seq, long_, seq, good, 2, nullptr, BAND(512) kSm, 1, 1, 0u, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("above 16384"));
    EXPECT(BANDED(local_device)(seq + 1, bad, seq, good, 2, nullptr, BAND(256) kSm, 1, 1, out, out, mv, st, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("decrease"));
    EXPECT(BANDED(local_device)(seq + 1, good, seq, good, 2, nullptr, BAND(256) kSm, 1, 1, out, out, mv, st, nullptr) == SWMI_ERR_ALIGNMENT);
    EXPECT(BANDED(slices_for)(kLocal, BAND(1024) good, bad, 2, 1, nullptr, 0) == 0);
    EXPECT(fake_hip_log_size() == 0 && g_launches.empty());                       // no device was touched
    std::printf("refusals: %s\n", g_failed ? "FAILED" : "ok");
}

// The planner's key, which both libraries sort by, against values worked out by hand from -band/2 <= j - i - d0 <= band/2 - 1
// (the launcher's stand-in checks the order against the key itself).  Rows i_lo .. i_hi, the key is i_hi - i_lo:
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
        EXPECT(width_swept_rows(kLocal, 300, 300, -560, bands[x]) == far[x]);
        EXPECT(width_swept_rows(kLocal, 300, 300, -100, bands[x]) == low_local[x]);
        EXPECT(width_swept_rows(kGlobal, 300, 300, -100, bands[x]) == low_global[x]);
        EXPECT(width_swept_rows(kLocal, 300, 250, 200, bands[x]) == high_local[x]);
        EXPECT(width_swept_rows(kGlobal, 300, 250, 200, bands[x]) == high_global[x]);
        EXPECT(width_swept_rows(kGlobal, 0, 250, 0, bands[x]) == 0 && width_swept_rows(kLocal, 9, 0, 0, bands[x]) == 0);
    }
    std::printf("swept rows by hand: %s\n", g_failed ? "FAILED" : "ok");
}

}  // namespace

int main()
{
    EXPECT(BANDED(version)() == SWMI_VERSION);
    refusals();
    swept_rows_by_hand();
    // at every width of the build: traceback, one slice, mixed shapes, both kinds -- the planner has work to do at every width
    for (int band : kBands) {
        host_case("traceback, local", kLocal, band, mixed(203, 900), true, true, 0u, 1);
        EXPECT(g_launches.size() == 1 && g_launches[0].reordered);
        host_case("traceback, global", kGlobal, band, mixed(57, 300), true, true, 15u, 1);
    }
    // the planner's key is the width's: (300, 300) at diagonal -560 misses a band of 128 .. 512 (its first row would be
    // 2 - band / 2 + 560 > 300) and has rows 50 .. 300 at 1024, so it stays behind (100, 100) at 0 (99 rows) at the narrow
    // widths and goes in front of it at 1024
    for (int band : kBands) {
        if (band == 256) continue;
        Batch t;
        t.add(100, 100, 0), t.add(300, 300, -560);
        host_case("planner key", kLocal, band, t, true, true, 0u, 1);
        EXPECT(g_launches.size() == 1 && g_launches[0].reordered == (band == 1024));
    }
    // the cases below run at one width each (the ragged build: at 128)
    // three ends-only slices, the last one ragged: the count cap of 2^20 on tiny mixed shapes, empty sequences among them (the
    // width does not enter)
    host_case("three ends-only slices", kLocal, at(256), mixed((size_t(2) << 20) + 7, 3), true, false, 0u, 3);
    host_case("two ends-only slices, global", kGlobal, at(512), mixed((size_t(1) << 20) + 5, 2), false, false, 10u, 2);
    // two ends-only slices cut by the byte budget (256 MiB), the second one ragged
    {
        Batch t;
        for (size_t k = 0; k < 12000; ++k) t.add(k % 5 == 4 ? 100 + k % 50 : 16384, k % 7 == 6 ? 0 : 16384, int32_t(k % 200) - 100);
        host_case("two slices by bytes", kGlobal, at(1024), t, true, false, 19u, 2);
    }
    host_case("traceback, global, no diagonals", kGlobal, at(256), mixed(57, 300), false, true, 15u, 1);
    // empty sequences on either side and both; a side that is empty throughout passes no byte
    {
        Batch t;
        t.add(0, 5, 0), t.add(5, 0, 3), t.add(0, 0, 0), t.add(7, 9, -2), t.add(0, 16384, 70), t.add(16384, 0, -70), t.add(0, 0, INT32_MAX);
        host_case("empty sequences, local", kLocal, at(512), t, true, true, 0u, 1);
        host_case("empty sequences, global", kGlobal, at(256), t, true, true, 3u, 1);
        Batch e1, e2, e12;
        for (size_t k = 0; k < 6; ++k) e1.add(0, 3 + k, int32_t(k)), e2.add(4 + k, 0, -int32_t(k)), e12.add(0, 0, 0);
        host_case("every seq1 empty", kGlobal, at(1024), e1, true, true, 16u, 1);
        host_case("every seq2 empty", kLocal, at(128), e2, true, false, 0u, 1);
        host_case("both sides empty", kGlobal, at(512), e12, false, true, 0u, 1);
    }
    // a second host call of the size of the largest so far reuses the sets: no allocation
    host_case("the sets are kept", kLocal, at(1024), mixed(203, 900), false, true, 0u, 1);
    EXPECT(count_log("malloc") == 0);
    // the device entries at every width of the build (each ends with a release, which frees the host entries' sets too)
    for (int band : kBands) device_case(band);
    EXPECT(BANDED(release_workspaces)() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("%s\n", kClosing);
    return 0;
}
