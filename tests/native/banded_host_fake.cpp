// banded_host_fake.cpp -- TEST ONLY: the host side of libswmi_banded.so (csrc/banded_api.cpp) and, built with
// -DSWMI_BANDED_GLOBAL_LIBRARY on every file, of libswmi_banded_global.so, on the fake GPU of fake_hip.cpp, as a stand-alone
// program under ASan + UBSan.  This file holds the stand-in for what banded_api.cpp takes from the library's kernel file -- the
// launcher -- and hipGetDevice.  The stand-in checks that every operand of a launch lies inside one live device block for the
// size the kernel would touch (a device-to-device copy of the range onto itself: fake_hip.cpp aborts on a range outside a
// block) and writes, for alignment k of a launch, with id = seq1[0] | seq2[0] << 8, d its diagonal (0 without) and free_ends
// the launch's mask (0 for the local library, which has none): score = id + 1000 d + 100000 free_ends, ends = (score + 1 ..
// score + 4), and with a traceback steps = id % 5 and every move word of its row = 0xC0DE << 48 | id << 8 | w.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#ifdef SWMI_BANDED_GLOBAL_LIBRARY
#include "../../include/swmi_banded_global.h"
#else
#include "../../include/swmi_banded.h"
#endif
#include "../../smith-waterman-simd_amd/csrc/banded_internal.h"

namespace {
hipError_t fake_launch(const uint8_t *s1, int len1, const uint8_t *s2, int len2, const int32_t *diag, size_t n, const int8_t *sm, int gap_open,
                       int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes, unsigned long long *moves,
                       size_t move_words, uint32_t *steps, hipStream_t stream);
}

// ---- what differs between the two libraries: the public header (above), the entries, the launcher's name, the size of an
// ---- alignment's codes, and whether there is a mask (the local entries take none: the cases' masks are dropped here)
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
#define ENTRY(name) swmi_banded_global_##name
#define MASK_ARG(mask) mask,
constexpr bool kHasMask = true;
constexpr const char *kOk = "banded global host fake ok";
const auto align_entry = swmi_banded_global;
const auto device_entry = swmi_banded_global_device;
constexpr size_t code_bytes(size_t len1) { return swmi::banded::band_global_code_bytes(len1); }
hipError_t swmi::banded::launch_banded_global(const uint8_t *s1, int len1, const uint8_t *s2, int len2, const int32_t *diag, size_t n,
                                              const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                              unsigned char *codes, unsigned long long *moves, size_t move_words, uint32_t *steps,
                                              hipStream_t stream)
{
    return fake_launch(s1, len1, s2, len2, diag, n, sm, gap_open, gap_extend, free_ends, scores, ends, codes, moves, move_words, steps, stream);
}
#else
#define ENTRY(name) swmi_banded_##name
#define MASK_ARG(mask)
constexpr bool kHasMask = false;
constexpr const char *kOk = "banded host fake ok";
const auto align_entry = swmi_banded_local;
const auto device_entry = swmi_banded_local_device;
constexpr size_t code_bytes(size_t len1) { return swmi::banded::band_code_bytes(len1); }
hipError_t swmi::banded::launch_banded_local(const uint8_t *s1, int len1, const uint8_t *s2, int len2, const int32_t *diag, size_t n,
                                             const int8_t *sm, int gap_open, int gap_extend, int32_t *scores, int32_t *ends, unsigned char *codes,
                                             unsigned long long *moves, size_t move_words, uint32_t *steps, hipStream_t stream)
{
    return fake_launch(s1, len1, s2, len2, diag, n, sm, gap_open, gap_extend, 0u, scores, ends, codes, moves, move_words, steps, stream);
}
#endif

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t k);
extern "C" void fake_hip_log_clear();

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

namespace {
struct Launch {
    size_t n, len1, len2, move_words;
    bool diag, tb;
    int open, extend, sm_sum;
    unsigned free_ends;
    const void *codes;
    hipStream_t stream;
};
std::vector<Launch> g_launches;
int g_failed = 0;

// the mask a case's launches must show
unsigned seen(unsigned mask) { return kHasMask ? mask : 0u; }

void in_block(const void *p, size_t bytes)
{
    if (bytes && hipMemcpy(const_cast<void *>(p), p, bytes, hipMemcpyDeviceToDevice) != hipSuccess) abort();
}

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

size_t count_log(const char *needle)
{
    size_t c = 0;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) c += std::strstr(fake_hip_log_at(k), needle) != nullptr;
    return c;
}

hipError_t fake_launch(const uint8_t *s1, int len1, const uint8_t *s2, int len2, const int32_t *diag, size_t n, const int8_t *sm, int gap_open,
                       int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes, unsigned long long *moves,
                       size_t move_words, uint32_t *steps, hipStream_t stream)
{
    const bool tb = moves != nullptr;
    in_block(s1, n * size_t(len1));
    in_block(s2, n * size_t(len2));
    if (diag) in_block(diag, n * 4);
    in_block(scores, n * 4);
    in_block(ends, n * 16);
    if (tb) {
        in_block(codes, n * code_bytes(size_t(len1)));
        in_block(moves, n * move_words * 8);
        in_block(steps, n * 4);
    }
    int sum = 0;
    for (int x = 0; x < 16; ++x) sum += sm[x] * (x + 1);
    g_launches.push_back({n, size_t(len1), size_t(len2), move_words, diag != nullptr, tb, gap_open, gap_extend, sum, free_ends, codes, stream});
    for (size_t k = 0; k < n; ++k) {
        const int id = s1[k * size_t(len1)] | s2[k * size_t(len2)] << 8;
        const int score = id + 1000 * (diag ? diag[k] : 0) + 100000 * int(free_ends);
        scores[k] = score;
        for (int e = 0; e < 4; ++e) ends[4 * k + e] = score + 1 + e;
        if (tb) {
            steps[k] = uint32_t(id % 5);
            for (size_t w = 0; w < move_words; ++w) moves[k * move_words + w] = 0xC0DEull << 48 | (unsigned long long)id << 8 | w;
        }
    }
    return hipSuccess;
}

struct Batch {
    size_t n, len1, len2;
    std::vector<uint8_t> a, b;
    std::vector<int32_t> d;
    Batch(size_t n_, size_t l1, size_t l2) : n(n_), len1(l1), len2(l2), a(n_ * l1, 3), b(n_ * l2, 2), d(n_)
    {
        for (size_t k = 0; k < n; ++k) {
            a[k * len1] = uint8_t(k * 7);
            b[k * len2] = uint8_t(k / 3);
            d[k] = int32_t(k % 11) - 5;
        }
    }
    int id(size_t k) const { return a[k * len1] | b[k * len2] << 8; }
};

const int8_t kSm[16] = {2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2, -3, -3, -3, -3, 2};
int sm_sum()
{
    int s = 0;
    for (int x = 0; x < 16; ++x) s += kSm[x] * (x + 1);
    return s;
}

// a host call; the results at the caller's positions, sentinels behind every output array untouched
void host_case(const char *name, const Batch &t, bool with_diag, bool tb, unsigned mask, size_t want_slices)
{
    const size_t mw = SWMI_LOCAL_FULL_MOVE_WORDS(t.len1, t.len2);
    std::vector<int32_t> scores(t.n + 1, -77), ends(4 * t.n + 1, -77);
    std::vector<uint64_t> moves(tb ? t.n * mw + 1 : 1, 0x5E5E5E5Eull);
    std::vector<uint32_t> steps(tb ? t.n + 1 : 1, 0x5E5Eu);
    std::vector<size_t> sizes(8, 0);
    const size_t slices = ENTRY(slices_for)(t.n, t.len1, t.len2, tb, sizes.data(), sizes.size());
    EXPECT(slices == want_slices);
    g_launches.clear();
    fake_hip_log_clear();
    const int rc = align_entry(t.a.data(), t.len1, t.b.data(), t.len2, t.n, with_diag ? t.d.data() : nullptr, kSm, 7, 3, MASK_ARG(mask)
                               scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? steps.data() : nullptr);
    EXPECT(rc == SWMI_OK);
    EXPECT(g_launches.size() == slices);
    size_t total = 0;
    for (size_t s = 0; s < g_launches.size(); ++s) {
        const Launch &l = g_launches[s];
        EXPECT(l.n == sizes[s] && l.len1 == t.len1 && l.len2 == t.len2 && l.move_words == mw && l.diag == with_diag && l.tb == tb);
        EXPECT(l.open == 7 && l.extend == 3 && l.sm_sum == sm_sum() && l.stream != nullptr);
        EXPECT(l.free_ends == seen(mask));                                 // the mask reaches every launch as given
        if (s > 0) EXPECT(l.stream != g_launches[s - 1].stream);          // two sets in turn
        if (s > 1) EXPECT(l.stream == g_launches[s - 2].stream);
        total += l.n;
    }
    EXPECT(total == t.n);
    // per slice: seq1, seq2 (and the diagonals) up; scores, ends (and steps, moves) down
    EXPECT(count_log("memcpy kind1") == slices * (with_diag ? 3 : 2));
    EXPECT(count_log("memcpy kind2") == slices * (tb ? 4 : 2));
    for (size_t k = 0; k < t.n; ++k) {
        const int score = t.id(k) + 1000 * (with_diag ? t.d[k] : 0) + 100000 * int(seen(mask));
        EXPECT(scores[k] == score);
        for (int e = 0; e < 4; ++e) EXPECT(ends[4 * k + e] == score + 1 + e);
        if (tb) {
            EXPECT(steps[k] == uint32_t(t.id(k) % 5));
            EXPECT(moves[k * mw] == (0xC0DEull << 48 | (unsigned long long)t.id(k) << 8) && moves[k * mw + mw - 1] == (moves[k * mw] | (mw - 1)));
        }
        if (g_failed) break;
    }
    EXPECT(scores[t.n] == -77 && ends[4 * t.n] == -77 && moves.back() == 0x5E5E5E5Eull && steps.back() == 0x5E5Eu);
    std::printf("%s: %s\n", name, g_failed ? "FAILED" : "ok");
}

// device calls on two streams of the caller's, a workspace per stream that grows with the call
void device_case()
{
    const Batch small(5, 40, 50), large(9, 300, 20);
    hipStream_t st[2];
    EXPECT(hipStreamCreateWithFlags(&st[0], 0) == hipSuccess && hipStreamCreateWithFlags(&st[1], 0) == hipSuccess);
    for (int round = 0; round < 3; ++round) {
        const Batch &t = round == 1 ? large : small;
        const unsigned mask = round == 0 ? 0u : round == 1 ? 15u : 19u;
        const size_t mw = SWMI_LOCAL_FULL_MOVE_WORDS(t.len1, t.len2);
        void *d1, *d2, *dd, *ds, *de, *dm, *dt;
        EXPECT(hipMalloc(&d1, t.a.size()) == hipSuccess && hipMalloc(&d2, t.b.size()) == hipSuccess && hipMalloc(&dd, t.n * 4) == hipSuccess);
        EXPECT(hipMalloc(&ds, t.n * 4) == hipSuccess && hipMalloc(&de, t.n * 16) == hipSuccess && hipMalloc(&dm, t.n * mw * 8) == hipSuccess &&
               hipMalloc(&dt, t.n * 4) == hipSuccess);
        std::memcpy(d1, t.a.data(), t.a.size());
        std::memcpy(d2, t.b.data(), t.b.size());
        std::memcpy(dd, t.d.data(), t.n * 4);
        g_launches.clear();
        fake_hip_log_clear();
        hipStream_t s = st[round == 2 ? 1 : 0];
        EXPECT(device_entry(d1, t.len1, d2, t.len2, t.n, dd, kSm, 2, 9, MASK_ARG(mask) ds, de, dm, dt, s) == SWMI_OK);
        EXPECT(g_launches.size() == 1 && g_launches[0].stream == s && g_launches[0].n == t.n && g_launches[0].tb && g_launches[0].diag);
        EXPECT(g_launches[0].open == 2 && g_launches[0].extend == 9 && g_launches[0].free_ends == seen(mask));
        // rounds 0 and 2 make a stream's first workspace, round 1 outgrows stream 0's: one allocation of one slice's codes each
        char want[64];
        std::snprintf(want, sizeof want, "malloc bytes%zu", t.n * code_bytes(t.len1));
        EXPECT(count_log(want) == 1 && count_log("malloc") == 1);
        EXPECT(count_log("memcpy kind1") + count_log("memcpy kind2") == 0);     // nothing goes up or down: the matrix rides in the launch
        for (size_t k = 0; k < t.n; ++k) EXPECT(static_cast<int32_t *>(ds)[k] == t.id(k) + 1000 * t.d[k] + 100000 * int(seen(mask)));
        // the same call again reuses the workspace; ends-only takes none
        fake_hip_log_clear();
        EXPECT(device_entry(d1, t.len1, d2, t.len2, t.n, nullptr, kSm, 2, 9, MASK_ARG(mask) ds, de, dm, dt, s) == SWMI_OK);
        EXPECT(device_entry(d1, t.len1, d2, t.len2, t.n, dd, kSm, 2, 9, MASK_ARG(16u) ds, de, nullptr, nullptr, s) == SWMI_OK);
        EXPECT(count_log("malloc") == 0 && g_launches.size() == 3 && !g_launches[1].diag && !g_launches[2].tb && g_launches[2].codes == nullptr);
        EXPECT(g_launches[1].codes == g_launches[0].codes && g_launches[1].free_ends == seen(mask) && g_launches[2].free_ends == seen(16u));
        float ms = -1.f;
        EXPECT(ENTRY(time_device)(d1, t.len1, d2, t.len2, t.n, dd, kSm, 2, 9, MASK_ARG(mask) ds, de, dm, dt, s, 3, &ms) == SWMI_OK && ms > 0.f);
        EXPECT(g_launches.size() == 3 + 4);
        for (size_t k = 3; k < g_launches.size(); ++k) EXPECT(g_launches[k].free_ends == seen(mask));
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
        // a refused mask reaches no launch, through any of the three entries
        fake_hip_log_clear();
        for (unsigned bad : {20u, 24u, 28u, 32u, 0xFFFFFFFFu}) {
            EXPECT(swmi_banded_global_device(d1, t.len1, d2, t.len2, t.n, dd, kSm, 2, 9, bad, ds, de, dm, dt, s) == SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(std::string(swmi_banded_global_last_error()).find("free_ends") != std::string::npos);
            EXPECT(swmi_banded_global_time_device(d1, t.len1, d2, t.len2, t.n, dd, kSm, 2, 9, bad, ds, de, dm, dt, s, 3, &ms) ==
                   SWMI_ERR_INVALID_ARGUMENT);
            EXPECT(swmi_banded_global(t.a.data(), t.len1, t.b.data(), t.len2, t.n, t.d.data(), kSm, 2, 9, bad, static_cast<int32_t *>(ds),
                                      static_cast<int32_t *>(de), nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
        }
        EXPECT(g_launches.size() == 3 + 4 && fake_hip_log_size() == 0);
#endif
        for (void *p : {d1, d2, dd, ds, de, dm, dt}) EXPECT(hipFree(p) == hipSuccess);
    }
    EXPECT(ENTRY(release_workspaces)() == SWMI_OK);
    EXPECT(hipStreamDestroy(st[0]) == hipSuccess && hipStreamDestroy(st[1]) == hipSuccess);
    std::printf("device entry: %s\n", g_failed ? "FAILED" : "ok");
}

}  // namespace

int main()
{
    EXPECT(ENTRY(version)() == SWMI_VERSION);
    // refusals touch no device
    int32_t out[8];
    fake_hip_log_clear();
    EXPECT(align_entry(nullptr, 4, nullptr, 4, 1, nullptr, kSm, 1, 1, MASK_ARG(0u) out, out, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(std::string(ENTRY(last_error)()).find("NULL buffer") != std::string::npos && fake_hip_log_size() == 0);
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
    EXPECT(swmi_banded_global(nullptr, 4, nullptr, 4, 1, nullptr, kSm, 1, 1, 20u, out, out, nullptr, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(std::string(swmi_banded_global_last_error()).find("free_ends 20") != std::string::npos && fake_hip_log_size() == 0);
#endif
    std::printf("refusals: %s\n", g_failed ? "FAILED" : "ok");
    // three ends-only slices: the count cap of 2^20 on the smallest shape
    host_case("three ends-only slices", Batch((size_t(2) << 20) + 7, 1, 1), true, false, 10u, 3);
    // a traceback call of one slice, with and without diagonals
    host_case("traceback, one slice", Batch(37, 70, 33), true, true, 0u, 1);
    host_case("traceback, no diagonals", Batch(6, 5, 900), false, true, 19u, 1);
    host_case("ends-only, no diagonals", Batch(6, 1, 16384), false, false, 15u, 1);
    // a second host call reuses the sets: no allocation
    host_case("the sets are kept", Batch(6, 1, 16384), false, false, 16u, 1);
    EXPECT(count_log("malloc") == 0);
    device_case();
    EXPECT(ENTRY(release_workspaces)() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("%s\n", kOk);
    return 0;
}
