// banded_ragged_host_fake.cpp -- TEST ONLY: the host side of libswmi_banded_ragged.so (csrc/banded_ragged_api.cpp) on the fake
// GPU of fake_hip.cpp, as a stand-alone program under ASan + UBSan.  This file holds the stand-in for what banded_ragged_api.cpp
// takes from the library's kernel file -- the launcher -- and hipGetDevice.  The stand-in knows the batch the driver is running
// and which caller index the launch's first alignment has, and checks per launch: the slots, the sequences, the codes, the
// moves and the results lie inside live device blocks for the sizes the kernels touch (a device-to-device copy of the range onto
// itself: fake_hip.cpp aborts on a range outside a block; every slot's range is shown to lie inside the range copied); every
// slot names an alignment of the slice once, with that alignment's offsets, lengths, move offset and CLAMPED diagonal, and its
// sequence starts with that alignment's marker bytes; code offsets are the running sum in slot order, so no two overlap; the
// slots are in the planner's order; kind, mask, gaps and matrix arrive as given.  It then writes for caller index c with
// clamped diagonal d: score = 3 c + d + 7000000 free_ends + 300000000 kind, ends = (score + 1 .. score + 4), and with a
// traceback steps = c % 5 (0 for an empty moves row) and every move word w of its row = 0xC0DE << 48 | c << 8 | (w & 255).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swmi_banded_ragged.h"
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
    int kind;
    size_t n, base;
    bool tb;
    int open, extend, sm_sum;
    unsigned free_ends;
    const void *codes, *slots;
    hipStream_t stream;
};
std::vector<Launch> g_launches;
const Batch *g_batch = nullptr;       // the batch of the entry call that is running
bool g_diag = true;                   // ... called with its diagonals
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

int expected_score(size_t c, int32_t d, unsigned free_ends, int kind) { return int(3 * c) + d + 7000000 * int(free_ends) + 300000000 * kind; }

}  // namespace

hipError_t swmi::banded::launch_banded_ragged(int kind, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n, const int8_t *sm,
                                              int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                              unsigned char *codes, unsigned long long *moves, uint32_t *steps, hipStream_t stream)
{
    const Batch &t = *g_batch;
    const bool tb = moves != nullptr;
    const size_t base = g_base;
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
    for (size_t c = base; c < base + n; ++c) code_total += swmi::banded::ragged_code_bytes(kind, t.len1(c));
    if (tb) {
        in_block(codes, code_total);
        in_block(moves, size_t(t.mo[base + n] - t.mo[base]) * 8);
        in_block(steps, n * 4);
        EXPECT((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
    }
    int sum = 0;
    for (int x = 0; x < 16; ++x) sum += sm[x] * (x + 1);
    g_launches.push_back({kind, n, base, tb, gap_open, gap_extend, sum, free_ends, codes, slots, stream});
    std::vector<char> seen(n, 0);
    uint64_t code_at = 0;
    int last_rows = 1 << 30;
    uint32_t last_index = 0;
    for (size_t x = 0; x < n; ++x) {
        const RaggedSlot &q = slots[x];
        EXPECT(q.index < n);
        if (q.index >= n) break;
        EXPECT(!seen[q.index]);                                                  // every alignment of the slice once
        seen[q.index] = 1;
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
            code_at += swmi::banded::ragged_code_bytes(kind, size_t(q.len1)) / 4;
            EXPECT(code_at * 4 <= code_total);
        }
        // the planner's order: swept rows descending, ties in caller order
        const int rows = swmi::banded::ragged_swept_rows(kind, q.len1, q.len2, q.d0);
        EXPECT(rows >= 0 && rows <= last_rows);
        if (x && rows == last_rows) EXPECT(q.index > last_index);
        last_rows = rows;
        last_index = q.index;
        const int32_t score = expected_score(c, q.d0, free_ends, kind);
        scores[q.index] = score;
        for (int e = 0; e < 4; ++e) ends[4 * q.index + e] = score + 1 + e;
        if (tb) {
            const size_t mw = size_t(t.mo[c + 1] - t.mo[c]);
            steps[q.index] = mw ? uint32_t(c % 5) : 0u;
            for (size_t w = 0; w < mw; ++w) moves[q.move_off + w] = 0xC0DEull << 48 | (unsigned long long)c << 8 | (w & 255);
        }
        if (g_failed) break;
    }
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

void check_results(const Batch &t, bool with_diag, bool tb, unsigned mask, int kind, const int32_t *scores, const int32_t *ends,
                   const uint64_t *moves, const uint32_t *steps)
{
    for (size_t c = 0; c < t.n; ++c) {
        const int score = expected_score(c, with_diag ? clamped(t.d[c]) : 0, kind == SWMI_BANDED_RAGGED_GLOBAL ? mask : 0u, kind);
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

int call_host(int kind, const Batch &t, bool with_diag, unsigned mask, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    g_batch = &t;
    g_diag = with_diag;
    g_base = 0;
    const uint8_t none = 0;
    const uint8_t *a = t.a.empty() ? &none : t.a.data(), *b = t.b.empty() ? &none : t.b.data();
    if (kind == SWMI_BANDED_RAGGED_GLOBAL)
        return swmi_banded_ragged_global(a, t.off1.data(), b, t.off2.data(), t.n, with_diag ? t.d.data() : nullptr, kSm, 7, 3, mask, scores, ends,
                                         moves, steps);
    return swmi_banded_ragged_local(a, t.off1.data(), b, t.off2.data(), t.n, with_diag ? t.d.data() : nullptr, kSm, 7, 3, scores, ends, moves, steps);
}

// a host call; the results at the caller's positions, sentinels behind every output array untouched
void host_case(const char *name, int kind, const Batch &t, bool with_diag, bool tb, unsigned mask, size_t want_slices)
{
    std::vector<int32_t> scores(t.n + 1, -77), ends(4 * t.n + 1, -77);
    std::vector<uint64_t> moves(tb ? size_t(t.mo[t.n]) + 1 : 1, 0x5E5E5E5Eull);
    std::vector<uint32_t> steps(tb ? t.n + 1 : 1, 0x5E5Eu);
    std::vector<size_t> sizes(8, 0);
    const size_t slices = swmi_banded_ragged_slices_for(kind, t.off1.data(), t.off2.data(), t.n, tb, sizes.data(), sizes.size());
    EXPECT(slices == want_slices);
    g_launches.clear();
    fake_hip_log_clear();
    EXPECT(call_host(kind, t, with_diag, mask, scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? steps.data() : nullptr) == SWMI_OK);
    EXPECT(g_launches.size() == slices);
    size_t total = 0;
    for (size_t s = 0; s < g_launches.size(); ++s) {
        const Launch &l = g_launches[s];
        EXPECT(l.kind == kind && l.n == sizes[s] && l.base == total && l.tb == tb);
        EXPECT(l.open == 7 && l.extend == 3 && l.sm_sum == sm_sum() && l.stream != nullptr);
        EXPECT(l.free_ends == (kind == SWMI_BANDED_RAGGED_GLOBAL ? mask : 0u));      // the mask reaches every launch as given
        if (s > 0) EXPECT(l.stream != g_launches[s - 1].stream);                      // two sets in turn
        if (s > 1) EXPECT(l.stream == g_launches[s - 2].stream);
        total += l.n;
    }
    EXPECT(total == t.n);
    // per slice: the two sequence buffers (none of an empty side) and the slots up; scores, ends (and steps, moves) down
    size_t ups = 0, downs = 0, at = 0;
    for (size_t s = 0; s < slices && s < sizes.size(); at += sizes[s], ++s) {
        ups += 1 + (t.off1[at + sizes[s]] > t.off1[at]) + (t.off2[at + sizes[s]] > t.off2[at]);
        downs += 2 + (tb ? 1 + (t.mo[at + sizes[s]] > t.mo[at]) : 0);
    }
    EXPECT(count_log("memcpy kind1") == ups && count_log("memcpy kind2") == downs);
    check_results(t, with_diag, tb, mask, kind, scores.data(), ends.data(), moves.data(), steps.data());
    EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves.back() == 0x5E5E5E5Eull && steps.back() == 0x5E5Eu);
    std::printf("%s: %s\n", name, g_failed ? "FAILED" : "ok");
}

// mixed shapes: lengths 0 .. top, diagonals that keep, shift and lose the band, INT32 extremes among them
Batch mixed(size_t n, size_t top)
{
    Batch t;
    for (size_t k = 0; k < n; ++k) {
        const size_t len1 = (k * 37 + 5) % (top + 1), len2 = (k * 53 + 11) % (top + 1);
        const int32_t diag = k % 13 == 0 ? INT32_MIN : k % 13 == 1 ? INT32_MAX : k % 13 == 2 ? 70000 : int32_t(k % 11) * 9 - 45;
        t.add(len1, len2, diag);
    }
    return t;
}

// device calls on two streams of the caller's: a workspace per stream, reused by the same call, and the timer
void device_case()
{
    const Batch small = mixed(23, 60), large = mixed(41, 700);
    hipStream_t st[2];
    EXPECT(hipStreamCreateWithFlags(&st[0], 0) == hipSuccess && hipStreamCreateWithFlags(&st[1], 0) == hipSuccess);
    for (int round = 0; round < 3; ++round) {
        const Batch &t = round == 1 ? large : small;
        const int kind = round == 2 ? SWMI_BANDED_RAGGED_LOCAL : SWMI_BANDED_RAGGED_GLOBAL;
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
            g_batch = &t;
            g_diag = with_diag;
            g_base = 0;
            const int32_t *dg = with_diag ? t.d.data() : nullptr;
            if (kind == SWMI_BANDED_RAGGED_GLOBAL)
                return swmi_banded_ragged_global_device(d1, t.off1.data(), d2, t.off2.data(), t.n, dg, kSm, 2, 9, m, ds, de, tb ? dm : nullptr,
                                                        tb ? dt : nullptr, s);
            return swmi_banded_ragged_local_device(d1, t.off1.data(), d2, t.off2.data(), t.n, dg, kSm, 2, 9, ds, de, tb ? dm : nullptr,
                                                   tb ? dt : nullptr, s);
        };
        g_launches.clear();
        fake_hip_log_clear();
        EXPECT(call(true, true, mask) == SWMI_OK);
        EXPECT(g_launches.size() == 1 && g_launches[0].stream == s && g_launches[0].n == t.n && g_launches[0].tb && g_launches[0].kind == kind);
        EXPECT(g_launches[0].open == 2 && g_launches[0].extend == 9 && g_launches[0].free_ends == (kind ? mask : 0u));
        // rounds 0 and 2 make a stream's first workspace, round 1 outgrows stream 0's: one allocation of codes and slots each
        size_t codes = 0;
        for (size_t c = 0; c < t.n; ++c) codes += swmi::banded::ragged_code_bytes(kind, t.len1(c));
        char want[64];
        std::snprintf(want, sizeof want, "malloc bytes%zu", codes + t.n * sizeof(RaggedSlot));
        EXPECT(count_log(want) == 1 && count_log("malloc") == 1);
        EXPECT(count_log("memcpy kind1") == 1 && count_log("memcpy kind2") == 0);     // the slots go up; the matrix rides in the launch
        check_results(t, true, true, mask, kind, scores, ends, moves, steps);
        // the same call again, without diagonals, and an ends-only call reuse the workspace: no second allocation
        fake_hip_log_clear();
        EXPECT(call(false, true, mask) == SWMI_OK);
        check_results(t, false, true, mask, kind, scores, ends, moves, steps);
        EXPECT(call(true, false, 16u) == SWMI_OK);
        check_results(t, true, false, 16u, kind, scores, ends, moves, steps);
        EXPECT(count_log("malloc") == 0 && g_launches.size() == 3 && !g_launches[2].tb && g_launches[2].codes == nullptr);
        EXPECT(g_launches[1].codes == g_launches[0].codes && g_launches[1].slots == g_launches[0].slots);
        // the timer: 1 + iters launches
        float ms = -1.f;
        g_batch = &t;
        g_diag = true;
        g_base = 0;
        EXPECT(swmi_banded_ragged_time_device(kind, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), kSm, 2, 9, mask, ds, de, dm, dt, s, 3,
                                              &ms) == SWMI_OK && ms > 0.f);
        EXPECT(g_launches.size() == 3 + 4 && count_log("malloc") == 0);
        for (size_t k = 3; k < g_launches.size(); ++k) EXPECT(g_launches[k].free_ends == (kind ? mask : 0u) && g_launches[k].kind == kind);
        EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves[t.mo[t.n]] == 0x5E5E5E5Eull && steps[t.n] == 0x5E5Eu);
        // a refused mask reaches no launch and touches no device, through any entry
        fake_hip_log_clear();
        for (unsigned bad : {20u, 24u, 32u, 0xFFFFFFFFu}) {
            EXPECT(swmi_banded_ragged_global_device(d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), kSm, 2, 9, bad, ds, de, dm, dt, s) ==
                   SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(std::string(swmi_banded_ragged_last_error()).find("free_ends") != std::string::npos);
            EXPECT(swmi_banded_ragged_time_device(SWMI_BANDED_RAGGED_GLOBAL, d1, t.off1.data(), d2, t.off2.data(), t.n, t.d.data(), kSm, 2, 9, bad, ds,
                                                  de, dm, dt, s, 3, &ms) == SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(swmi_banded_ragged_global(t.a.data(), t.off1.data(), t.b.data(), t.off2.data(), t.n, t.d.data(), kSm, 2, 9, bad, scores, ends,
                                             nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        }
        EXPECT(g_launches.size() == 3 + 4 && fake_hip_log_size() == 0);
        for (void *p : {d1, d2, ds, de, dm, dt}) EXPECT(hipFree(p) == hipSuccess);
    }
    EXPECT(swmi_banded_ragged_release_workspaces() == SWMI_OK);
    EXPECT(hipStreamDestroy(st[0]) == hipSuccess && hipStreamDestroy(st[1]) == hipSuccess);
    std::printf("device entry: %s\n", g_failed ? "FAILED" : "ok");
}

void refusals()
{
    int32_t out[8];
    uint64_t mv[4];
    uint32_t st[4];
    const uint8_t seq[16] = {};
    const uint64_t good[3] = {0, 4, 8}, bad[3] = {0, 4, 3}, long_[3] = {0, 4, 4 + 16385};
    fake_hip_log_clear();
    g_launches.clear();
    auto text = [](const char *needle) { return std::string(swmi_banded_ragged_last_error()).find(needle) != std::string::npos; };
    // in the header's order: each call also breaks every later rule
    EXPECT(swmi_banded_ragged_global(nullptr, bad, nullptr, bad, 2, nullptr, nullptr, 200, 1, 20u, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("free_ends 20"));
    EXPECT(swmi_banded_ragged_local(nullptr, bad, nullptr, bad, 2, nullptr, nullptr, 200, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("score_matrix"));
    EXPECT(swmi_banded_ragged_local(nullptr, bad, nullptr, bad, 2, nullptr, kSm, 200, 1, out, out, mv, nullptr) == SWMI_ERR_DOMAIN && text("outside [0,127]"));
    EXPECT(swmi_banded_ragged_local(nullptr, bad, nullptr, bad, 0, nullptr, kSm, 1, 1, out, out, mv, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("moves and steps"));
    EXPECT(swmi_banded_ragged_local(nullptr, nullptr, nullptr, nullptr, 0, nullptr, kSm, 1, 1, nullptr, nullptr, nullptr, nullptr) == SWMI_OK);
    EXPECT(swmi_banded_ragged_local(nullptr, bad, seq, bad, 2, nullptr, kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("NULL buffer"));
    EXPECT(swmi_banded_ragged_local(seq, nullptr, seq, good, 2, nullptr, kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("NULL"));
    EXPECT(swmi_banded_ragged_local(seq, good, seq, bad, 2, nullptr, kSm, 1, 1, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("decrease"));
    EXPECT(swmi_banded_ragged_global(seq, long_, seq, good, 2, nullptr, kSm, 1, 1, 0u, out, out, mv, st) == SWMI_ERR_INVALID_ARGUMENT && text("above 16384"));
    EXPECT(swmi_banded_ragged_local_device(seq + 1, bad, seq, good, 2, nullptr, kSm, 1, 1, out, out, mv, st, nullptr) == SWMI_ERR_INVALID_ARGUMENT && text("decrease"));
    EXPECT(swmi_banded_ragged_local_device(seq + 1, good, seq, good, 2, nullptr, kSm, 1, 1, out, out, mv, st, nullptr) == SWMI_ERR_ALIGNMENT);
    EXPECT(swmi_banded_ragged_slices_for(SWMI_BANDED_RAGGED_LOCAL, good, bad, 2, 1, nullptr, 0) == 0);
    EXPECT(fake_hip_log_size() == 0 && g_launches.empty());                       // no device was touched
    std::printf("refusals: %s\n", g_failed ? "FAILED" : "ok");
}

}  // namespace

int main()
{
    EXPECT(swmi_banded_ragged_version() == SWMI_VERSION);
    refusals();
    // three ends-only slices, the last one ragged: the count cap of 2^20 on tiny mixed shapes, empty sequences among them
    host_case("three ends-only slices", SWMI_BANDED_RAGGED_LOCAL, mixed((size_t(2) << 20) + 7, 3), true, false, 0u, 3);
    host_case("two ends-only slices, global", SWMI_BANDED_RAGGED_GLOBAL, mixed((size_t(1) << 20) + 5, 2), false, false, 10u, 2);
    // two ends-only slices cut by the byte budget (256 MiB), the second one ragged
    {
        Batch t;
        for (size_t k = 0; k < 12000; ++k) t.add(k % 5 == 4 ? 100 + k % 50 : 16384, k % 7 == 6 ? 0 : 16384, int32_t(k % 200) - 100);
        host_case("two slices by bytes", SWMI_BANDED_RAGGED_GLOBAL, t, true, false, 19u, 2);
    }
    // traceback, one slice, mixed shapes, both kinds, with and without diagonals
    host_case("traceback, local", SWMI_BANDED_RAGGED_LOCAL, mixed(203, 900), true, true, 0u, 1);
    host_case("traceback, global, no diagonals", SWMI_BANDED_RAGGED_GLOBAL, mixed(57, 300), false, true, 15u, 1);
    // empty sequences on either side and both; a side that is empty throughout passes no byte
    {
        Batch t;
        t.add(0, 5, 0), t.add(5, 0, 3), t.add(0, 0, 0), t.add(7, 9, -2), t.add(0, 16384, 70), t.add(16384, 0, -70), t.add(0, 0, INT32_MAX);
        host_case("empty sequences, local", SWMI_BANDED_RAGGED_LOCAL, t, true, true, 0u, 1);
        host_case("empty sequences, global", SWMI_BANDED_RAGGED_GLOBAL, t, true, true, 3u, 1);
        Batch e1, e2, e12;
        for (size_t k = 0; k < 6; ++k) e1.add(0, 3 + k, int32_t(k)), e2.add(4 + k, 0, -int32_t(k)), e12.add(0, 0, 0);
        host_case("every seq1 empty", SWMI_BANDED_RAGGED_GLOBAL, e1, true, true, 16u, 1);
        host_case("every seq2 empty", SWMI_BANDED_RAGGED_LOCAL, e2, true, false, 0u, 1);
        host_case("both sides empty", SWMI_BANDED_RAGGED_GLOBAL, e12, false, true, 0u, 1);
    }
    // a second host call of the same size reuses the sets: no allocation
    host_case("the sets are kept", SWMI_BANDED_RAGGED_LOCAL, mixed(203, 900), false, true, 0u, 1);
    EXPECT(count_log("malloc") == 0);
    device_case();
    EXPECT(swmi_banded_ragged_release_workspaces() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("banded ragged host fake ok\n");
    return 0;
}
