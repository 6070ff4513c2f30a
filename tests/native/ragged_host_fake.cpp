// ragged_host_fake.cpp -- the host side of the ragged local aligners (swmi_local_align_ragged*, local_ragged_api.cpp through
// the slice pipeline of swmi_table.cpp) on the fake GPU of fake_hip.cpp.  This file holds the stand-ins of the ragged
// launchers (fake_hip.cpp holds the fixed-length ones and the code sizes).  Alignment k's seq2 carries k
// in its first four bytes and its seq1 byte j is (k + j) & 255; a stand-in checks every slot of a launch (lengths longest
// first, equal lengths in caller order, each result index once, its seq1 where the slot says) and writes score 2 k + 1,
// ends[e] = 8 k + e + 3, steps k % (32 move_words + 1) and move word w = 0xC0DE << 48 | k << 16 | w in every word of its row.
// Built and run by tests/test_ragged_host_fake.py (g++, ASan + UBSan, no GPU).
//
// Host entry, traceback and ends-only, one slice and several: every result at its caller position, every move word, one
// move copy per slice of exactly its alignments' words, launches alternating between the two sets' streams.  The affine
// host entry.  The device entry on two streams, growing a stream's workspace.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Launch {
    bool affine;
    size_t n;
    hipStream_t st;
};
static std::vector<Launch> g_launches;

namespace swmi {
static hipError_t fake_ragged(bool affine, const uint8_t *s1, const uint8_t *s2, const LocalWork *work, size_t n, int32_t *scores,
                              int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    g_launches.push_back({affine, n, st});
    std::vector<char> seen(n, 0);
    for (size_t slot = 0; slot < n; ++slot) {
        const LocalWork w = work[slot];
        CHECK(w.k < n && !seen[w.k]);
        seen[w.k] = 1;
        if (slot) CHECK(w.len1 < work[slot - 1].len1 || (w.len1 == work[slot - 1].len1 && w.k > work[slot - 1].k));
        uint32_t id = 0;
        memcpy(&id, s2 + 128 * size_t(w.k), 4);
        for (uint32_t j = 0; j < w.len1; ++j) CHECK(s1[size_t(w.s1_off) + j] == uint8_t(id + j));
        scores[w.k] = int32_t(2 * id + 1);
        for (int e = 0; e < 4; ++e) ends[4 * size_t(w.k) + e] = int32_t(8 * id + e + 3);
        if (!moves) continue;
        const size_t cw = affine ? local_affine_code_words(int(w.len1)) : local_code_words(int(w.len1));
        memset(codes + w.code_base, 0xA5, cw * sizeof(uint32_t));
        const size_t mw = SWMI_LOCAL_MOVE_WORDS(w.len1);
        steps[w.k] = uint32_t(id % (32 * mw + 1));
        for (size_t x = 0; x < mw; ++x) moves[w.move_base + x] = 0xC0DEull << 48 | uint64_t(id) << 16 | x;
    }
    return hipSuccess;
}
hipError_t launch_local_ragged(const uint8_t *s1, const uint8_t *s2, const LocalWork *work, size_t n, const int8_t *, int, int32_t *scores,
                               int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    return fake_ragged(false, s1, s2, work, n, scores, ends, codes, moves, steps, st);
}
hipError_t launch_local_affine_ragged(const uint8_t *s1, const uint8_t *s2, const LocalWork *work, size_t n, const int8_t *, int, int,
                                      int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps,
                                      hipStream_t st)
{
    return fake_ragged(true, s1, s2, work, n, scores, ends, codes, moves, steps, st);
}
}  // namespace swmi

static const int8_t g_sm[16] = {1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1};

struct Batch {
    std::vector<uint64_t> off, mo;
    std::vector<uint8_t> s1, s2;
    size_t n;
};

static Batch make_batch(const std::vector<uint32_t> &lens)
{
    Batch b;
    b.n = lens.size();
    b.off.assign(1, 5);                                 // offsets need not start at 0
    b.s1.assign(5, 0x77);
    b.s2.assign(128 * b.n, 0);
    for (size_t k = 0; k < b.n; ++k) {
        for (uint32_t j = 0; j < lens[k]; ++j) b.s1.push_back(uint8_t(k + j));
        b.off.push_back(b.s1.size());
        const uint32_t id = uint32_t(k);
        memcpy(&b.s2[128 * k], &id, 4);
    }
    b.mo.resize(b.n + 1);
    CHECK(swmi_local_ragged_move_offsets(b.off.data(), b.n, b.mo.data()) == SWMI_OK);
    return b;
}

static void check_results(const Batch &b, const int32_t *scores, const int32_t *ends, const uint64_t *moves, const uint32_t *steps)
{
    for (size_t k = 0; k < b.n; ++k) {
        CHECK(scores[k] == int32_t(2 * k + 1));
        for (int e = 0; e < 4; ++e) CHECK(ends[4 * k + e] == int32_t(8 * k + e + 3));
        if (!moves) continue;
        const size_t mw = b.mo[k + 1] - b.mo[k];
        CHECK(steps[k] == uint32_t(k % (32 * mw + 1)));
        for (size_t x = 0; x < mw; ++x) CHECK(moves[b.mo[k] + x] == (0xC0DEull << 48 | uint64_t(k) << 16 | x));
    }
}

// the device-to-host copies of the last call (bytes, in order)
static std::vector<size_t> d2h_copies()
{
    std::vector<size_t> out;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) {
        size_t bytes = 0;
        int st = 0;
        const char *l = strstr(fake_hip_log_at(k), "memcpy kind2 bytes");
        if (l && sscanf(l, "memcpy kind2 bytes%zu stream%d", &bytes, &st) == 2) out.push_back(bytes);
    }
    return out;
}

static void host_case(const char *name, const std::vector<uint32_t> &lens, bool affine, bool tb, size_t min_slices)
{
    const Batch b = make_batch(lens);
    std::vector<size_t> sizes(swmi_local_ragged_slices_for(b.off.data(), b.n, affine, tb, nullptr, 0));
    swmi_local_ragged_slices_for(b.off.data(), b.n, affine, tb, sizes.data(), sizes.size());
    CHECK(sizes.size() >= min_slices);
    std::vector<int32_t> scores(b.n, -1), ends(4 * b.n, -1);
    std::vector<uint64_t> moves(tb ? b.mo[b.n] : 0, 0x5E5E5E5E5E5E5E5Eull);
    std::vector<uint32_t> steps(b.n);
    g_launches.clear();
    fake_hip_log_clear();
    const int rc = affine ? swmi_local_align_affine_ragged(b.s1.data(), b.off.data(), b.s2.data(), b.n, g_sm, 3, 1, scores.data(), ends.data(),
                                                           tb ? moves.data() : nullptr, tb ? steps.data() : nullptr)
                          : swmi_local_align_ragged(b.s1.data(), b.off.data(), b.s2.data(), b.n, g_sm, 1, scores.data(), ends.data(),
                                                    tb ? moves.data() : nullptr, tb ? steps.data() : nullptr);
    CHECK(rc == SWMI_OK);
    check_results(b, scores.data(), ends.data(), tb ? moves.data() : nullptr, steps.data());
    // one launch per slice, of the slice's size, alternating between the two sets' streams when there are several
    CHECK(g_launches.size() == sizes.size());
    for (size_t k = 0; k < fake_hip_log_size(); ++k) CHECK(!strstr(fake_hip_log_at(k), " launch_local"));     // no fixed-length launcher ran
    for (size_t s = 0; s < sizes.size(); ++s) {
        CHECK(g_launches[s].n == sizes[s] && g_launches[s].affine == affine);
        if (s) CHECK(g_launches[s].st != g_launches[s - 1].st);
        if (s > 1) CHECK(g_launches[s].st == g_launches[s - 2].st);
    }
    // per slice: scores, ends (, steps, then exactly the slice's move words)
    const std::vector<size_t> copies = d2h_copies();
    const size_t per = tb ? 4 : 2;
    CHECK(copies.size() == per * sizes.size());
    size_t first = 0;
    for (size_t c = 0; c < copies.size(); c += per) {
        const size_t s = c / per, m = sizes[s];
        CHECK(copies[c] == 4 * m && copies[c + 1] == 16 * m);
        if (tb) CHECK(copies[c + 2] == 4 * m && copies[c + 3] == 8 * (b.mo[first + m] - b.mo[first]));
        first += m;
    }
    printf("%s: ok (%zu alignments, %zu slices)\n", name, b.n, sizes.size());
}

static std::vector<uint32_t> lengths(size_t n, uint32_t top, uint32_t seed, size_t long_every)
{
    std::vector<uint32_t> v(n);
    uint64_t x = seed;
    for (size_t k = 0; k < n; ++k) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v[k] = long_every && k % long_every == 0 ? SWMI_LOCAL_MAX_LEN : uint32_t((x >> 33) % (top + 1));
    }
    return v;
}

static void device_case()
{
    hipStream_t sa = nullptr, sb = nullptr;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    for (int round = 0; round < 3; ++round) {
        const Batch b = make_batch(lengths(round == 0 ? 40 : 3000, 700, 9 + round, round == 2 ? 50 : 0));
        hipStream_t st = round == 1 ? sb : sa;
        void *d1, *d2, *dsc, *de, *dmv, *dst;
        CHECK(hipMalloc(&d1, b.s1.size()) == hipSuccess && hipMalloc(&d2, b.s2.size()) == hipSuccess);
        CHECK(hipMalloc(&dsc, 4 * b.n) == hipSuccess && hipMalloc(&de, 16 * b.n) == hipSuccess);
        CHECK(hipMalloc(&dmv, 8 * b.mo[b.n]) == hipSuccess && hipMalloc(&dst, 4 * b.n) == hipSuccess);
        CHECK(hipMemcpy(d1, b.s1.data(), b.s1.size(), hipMemcpyHostToDevice) == hipSuccess);
        CHECK(hipMemcpy(d2, b.s2.data(), b.s2.size(), hipMemcpyHostToDevice) == hipSuccess);
        fake_hip_log_clear();
        CHECK(swmi_local_align_ragged_device(d1, b.off.data(), d2, b.n, g_sm, 1, dsc, de, dmv, dst, st) == SWMI_OK);
        // the workspace grows on the first call on a stream and on a bigger one: a synchronisation of that stream, then one
        // allocation of the codes plus the slots
        bool grew = false;
        for (size_t k = 0; k < fake_hip_log_size(); ++k) grew = grew || strstr(fake_hip_log_at(k), "malloc bytes") != nullptr;
        CHECK(grew);                                    // sa's first call, sb's first call, a bigger call on sa
        CHECK(hipStreamSynchronize(st) == hipSuccess);
        check_results(b, static_cast<int32_t *>(dsc), static_cast<int32_t *>(de), static_cast<uint64_t *>(dmv), static_cast<uint32_t *>(dst));
        // the same call again fits: no allocation
        fake_hip_log_clear();
        CHECK(swmi_local_align_ragged_device(d1, b.off.data(), d2, b.n, g_sm, 1, dsc, de, dmv, dst, st) == SWMI_OK);
        for (size_t k = 0; k < fake_hip_log_size(); ++k) CHECK(strstr(fake_hip_log_at(k), "malloc bytes") == nullptr);
        CHECK(hipStreamSynchronize(st) == hipSuccess);
        for (void *p : {d1, d2, dsc, de, dmv, dst}) CHECK(hipFree(p) == hipSuccess);
    }
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    printf("device entry on two streams: ok\n");
}

int main()
{
    CHECK(swmi_init(0) == SWMI_OK);
    host_case("linear traceback, one slice", lengths(300, 300, 1, 0), false, true, 1);
    host_case("linear traceback, several slices", lengths(150000, 300, 2, 5000), false, true, 3);
    host_case("linear ends-only", lengths(5000, 16384, 3, 0), false, false, 1);
    host_case("affine traceback, several slices", lengths(20000, 2000, 4, 7), true, true, 2);
    host_case("affine ends-only", lengths(777, 40, 5, 0), true, false, 1);
    host_case("empty seq1s only", std::vector<uint32_t>(33, 0), false, true, 1);
    device_case();
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("ragged host fake ok\n");
    return 0;
}
