// tile_ragged_host_fake.cpp -- the host side of the three kinds of ragged aligner on the wavefront-tiled sweep
// (tile_ragged_api.cpp through the slice pipeline of swmi_table.cpp) on a fake GPU (fake_hip.cpp), plus the stand-ins for the
// six ragged launchers and the three wave-count functions (fake_hip.cpp holds the fixed-length ones and the code sizes).  One
// driver, one row of data per kind (kFamilies): `local` (swmi_local_full[_affine]_ragged*), `global`
// (swmi_global_full[_affine]_ragged*) or `semiglobal` (swmi_semiglobal_full[_affine]_ragged*) on the command line.  The code
// workspaces take fake_hip.cpp's constant 1024 dwords (512 qwords with affine gaps) per alignment, so a traceback slice is a
// few thousand alignments.  Built once and run per kind by tests/test_tile_ragged_host_fake.py (g++, ASan + UBSan, no GPU).
//
// A stand-in launch checks that the matrix, the gaps and (global) the mask are the call's, copies its slots and computes every
// slot's results from ALL bytes of the sequences the slot names (so ASan sees a slot that points outside the buffers): score =
// 3 len1 + 5 len2 + sum(seq1) + 7 sum(seq2) + 1000 mask, ends[e] = score + e + 1 for the kind's four or TWO ends per
// alignment, and with a traceback (sum(seq1) + sum(seq2)) % (32 move_words + 1 - count_offset) moves, reported as that +
// count_offset (steps: 0, the semi-global lengths: 1), and move word w = 0xC0DE << 48 | score << 16 | w in every word of its
// row; it writes the first and last word of the slot's codes.  A slot with a zero length gets include/swmi.h's result -- local:
// score 0, ends (0, 0, 0 or -1, 0 or -1), steps 0; semi-global: score 0, ends (0, 0), length 1; global: the closed form (score,
// ends, steps and ceil(steps / 32) whole move words inside its row) -- and touches neither sequence nor codes, as the kernel
// does.  After a call the driver checks, launch by launch and slice by slice: each slot's offsets and lengths are those of its
// alignment relative to the slice (so inside the sequences the launch was handed); every slot has the wave count the launch
// was given -- a zero-length slot 1 -- and len1 descending inside a launch; code and move ranges are disjoint and inside their
// buffers, the codes one block without holes (a zero-length slot takes none); the launches of a slice run in descending wave
// count and together cover each of its slots once; no fixed-length launcher ran.  The ends array the entry is given holds a
// sentinel pair behind its ends-per-alignment * n int32, and the moves a sentinel behind the last row: both must survive.
//
// Cases: the refusals before any device is bound (n = 0, decreasing offsets, a traceback given by half, a gap outside its
// domain, a mask of 16); one plan-only check with the REAL code words: 300 alignments of 16384 x 16384 with affine traceback,
// whose code bases pass 2^32 dwords; the host entry, linear and affine (the global kind each under its own mask), traceback
// (slices by the byte budget) and ends-only (lengths 0 .. 4: slices by the count cap), at n = 1, one slice, one slice + 1 and
// two and a half slices; the device entry on two streams with a growing workspace; the release, then the host entry again.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/swmi.h"
#include "../../smith-waterman-simd_amd/csrc/swmi_host.h"

extern "C" size_t fake_hip_log_size();
extern "C" const char *fake_hip_log_at(size_t);
extern "C" void fake_hip_log_clear();
extern "C" void fake_hip_real_code_sizes(int on);

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            fprintf(stderr, "CHECK failed at line %d: %s (last error: %s)\n", __LINE__, #cond, swmi_last_error()); \
            exit(1);                                                                                         \
        }                                                                                                    \
    } while (0)

constexpr uint64_t kSentinel = 0x5E5E5E5E5E5E5E5Eull;
constexpr int32_t kEndSentinel = 0x5E5E5E5E;
constexpr size_t kCodeDwords = 1024;     // fake_hip.cpp kFakeCodeWords
static size_t code_words(bool affine) { return affine ? kCodeDwords / 2 : kCodeDwords; }     // in the kind's unit: dwords, qwords
constexpr int kMax = 16384;
static_assert(kMax == SWMI_LOCAL_FULL_MAX_LEN && kMax == SWMI_GLOBAL_FULL_MAX_LEN && kMax == SWMI_SGFULL_MAX_LEN);
static int8_t g_sm[16];

// what an alignment with a zero length yields: include/swmi.h
struct Zero {
    int32_t score, ends[4];
    uint32_t count;             // what the count array reports
    uint32_t moves;             // moves written: ceil(moves / 32) whole words of `word`
    uint64_t word;
};
struct Family;
static const Family *g_f;

// ---- the kinds ----
#define IN const uint8_t *s1, const uint64_t *o1, const uint8_t *s2, const uint64_t *o2, size_t n
#define OUT int32_t *sc, int32_t *en, uint64_t *mv, uint32_t *ct
#define DEV_IN const void *s1, const uint64_t *o1, const void *s2, const uint64_t *o2, size_t n
#define DEV_OUT void *sc, void *en, void *mv, void *ct, void *st
struct Family {
    const char *name;           // on the command line
    swmi::host::TileKind kind;
    size_t n_ends;              // int32 of `ends` per alignment
    const char *count;          // the count array's name in the error text, and
    uint32_t count_offset;      //   count = moves + count_offset ("steps": 0, "lengths": 1)
    int gap, open, extend;      // the gaps the driver calls with and the stand-ins insist on: linear; affine open, extend
    bool mask;                  // the entries take a mask: one per linear / affine (mask_of), folded into the score
    Zero (*zero)(size_t len1, size_t len2, bool affine, unsigned mask, bool tb);
    size_t (*move_words)(size_t len1, size_t len2);
    size_t (*slices_for)(const uint64_t *, const uint64_t *, size_t, int, int, size_t *, size_t);
    int (*host)(bool affine, IN, int gap, int extend, unsigned mask, OUT);
    int (*device)(bool affine, DEV_IN, int gap, int extend, unsigned mask, DEV_OUT);
    int (*release[2])(void);    // linear, affine
};

static Zero zero_local(size_t, size_t, bool, unsigned, bool tb) { return {0, {0, 0, tb ? 0 : -1, tb ? 0 : -1}, 0, 0, 0}; }
static Zero zero_semiglobal(size_t, size_t, bool, unsigned, bool) { return {0, {0, 0, 0, 0}, 1, 0, 0}; }
// the closed form of include/swmi.h for the global kind
static Zero zero_global(size_t len1, size_t len2, bool affine, unsigned mask, bool tb)
{
    const bool up = len2 == 0;
    const size_t L = len1 + len2;
    const unsigned begin = up ? SWMI_FREE_BEGIN1 : SWMI_FREE_BEGIN2, end = up ? SWMI_FREE_END1 : SWMI_FREE_END2;
    const int32_t cost = L == 0 ? 0 : affine ? 5 + int32_t(L - 1) * 2 : int32_t(L) * 3;     // the global row's gaps
    Zero z{0, {0, 0, 0, 0}, 0, 0, up ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull};
    if (L && !(mask & end)) {
        z.ends[0] = int32_t(len1);
        z.ends[1] = int32_t(len2);
        if (mask & begin) {
            z.ends[2] = int32_t(len1);
            z.ends[3] = int32_t(len2);
        } else {
            z.score = -cost;
            z.count = z.moves = uint32_t(L);
        }
    }
    if (!tb) z.ends[2] = z.ends[3] = -1;
    return z;
}

static const Family kFamilies[] = {
    {"local", swmi::host::kTileLocal, 4, "steps", 0, 1, 1, 2, false, zero_local,
     [](size_t a, size_t b) { return size_t(SWMI_LOCAL_FULL_MOVE_WORDS(a, b)); }, swmi_local_full_ragged_slices_for,
     [](bool affine, IN, int gap, int extend, unsigned, OUT) {
         return affine ? swmi_local_full_affine_ragged(s1, o1, s2, o2, n, g_sm, gap, extend, sc, en, mv, ct)
                       : swmi_local_full_ragged(s1, o1, s2, o2, n, g_sm, int8_t(gap), sc, en, mv, ct);
     },
     [](bool affine, DEV_IN, int gap, int extend, unsigned, DEV_OUT) {
         return affine ? swmi_local_full_affine_ragged_device(s1, o1, s2, o2, n, g_sm, gap, extend, sc, en, mv, ct, st)
                       : swmi_local_full_ragged_device(s1, o1, s2, o2, n, g_sm, int8_t(gap), sc, en, mv, ct, st);
     },
     {swmi_local_full_release_workspaces, swmi_local_full_affine_release_workspaces}},
    {"global", swmi::host::kTileGlobal, 4, "steps", 0, 3, 5, 2, true, zero_global,
     [](size_t a, size_t b) { return size_t(SWMI_GLOBAL_FULL_MOVE_WORDS(a, b)); }, swmi_global_full_ragged_slices_for,
     [](bool affine, IN, int gap, int extend, unsigned mask, OUT) {
         return affine ? swmi_global_full_affine_ragged(s1, o1, s2, o2, n, g_sm, gap, extend, mask, sc, en, mv, ct)
                       : swmi_global_full_ragged(s1, o1, s2, o2, n, g_sm, int8_t(gap), mask, sc, en, mv, ct);
     },
     [](bool affine, DEV_IN, int gap, int extend, unsigned mask, DEV_OUT) {
         return affine ? swmi_global_full_affine_ragged_device(s1, o1, s2, o2, n, g_sm, gap, extend, mask, sc, en, mv, ct, st)
                       : swmi_global_full_ragged_device(s1, o1, s2, o2, n, g_sm, int8_t(gap), mask, sc, en, mv, ct, st);
     },
     {swmi_global_full_release_workspaces, swmi_global_full_affine_release_workspaces}},
    {"semiglobal", swmi::host::kTileSemiglobal, 2, "lengths", 1, 3, 5, 2, false, zero_semiglobal,
     [](size_t a, size_t b) { return size_t(SWMI_SGFULL_MOVE_WORDS(a, b)); }, swmi_semiglobal_full_ragged_slices_for,
     [](bool affine, IN, int gap, int extend, unsigned, OUT) {
         return affine ? swmi_semiglobal_full_affine_ragged(s1, o1, s2, o2, n, g_sm, gap, extend, sc, en, mv, ct)
                       : swmi_semiglobal_full_ragged(s1, o1, s2, o2, n, g_sm, int8_t(gap), sc, en, mv, ct);
     },
     [](bool affine, DEV_IN, int gap, int extend, unsigned, DEV_OUT) {
         return affine ? swmi_semiglobal_full_affine_ragged_device(s1, o1, s2, o2, n, g_sm, gap, extend, sc, en, mv, ct, st)
                       : swmi_semiglobal_full_ragged_device(s1, o1, s2, o2, n, g_sm, int8_t(gap), sc, en, mv, ct, st);
     },
     {swmi_semiglobal_full_release_workspaces, swmi_semiglobal_full_affine_release_workspaces}},
};
#undef IN
#undef OUT
#undef DEV_IN
#undef DEV_OUT

// what the call under test was given: the launchers must see exactly this
static unsigned g_mask = 0;
static unsigned mask_of(bool affine)
{
    if (!g_f->mask) return 0;
    return affine ? SWMI_ENDS_FIT | SWMI_FREE_END1 : SWMI_FREE_BEGIN1 | SWMI_FREE_END2;
}
static int gap_of(bool affine) { return affine ? g_f->open : g_f->gap; }
static int extend_of(bool affine) { return affine ? g_f->extend : 0; }

static size_t real_code_words(int len1, int len2) { return size_t((len2 + 1023) / 1024) * size_t((len1 + 63 + 31) / 32 * 8) * 256; }
static size_t mw_of(size_t len1, size_t len2) { return g_f->move_words(len1, len2); }
// the moves of a slot with both lengths, from the sums of its sequences; the count reports them + count_offset
static uint32_t moves_of(uint32_t sums, size_t mw) { return uint32_t(sums % (32 * mw + 1 - g_f->count_offset)); }

// ---- the launcher stand-ins -------------------------------------------------------------------------------------------------
struct Launch {
    std::vector<swmi::TileWork> slots;
    int waves;
    bool affine, traceback;
    hipStream_t stream;
};
static std::mutex g_launch_mu;
static std::vector<Launch> g_launches;

static int32_t score_of(const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, uint32_t *sums)
{
    uint32_t s1 = 0, s2 = 0;
    for (size_t x = 0; x < len1; ++x) s1 += a[x];
    for (size_t x = 0; x < len2; ++x) s2 += b[x];
    *sums = s1 + s2;
    return int32_t(3 * len1 + 5 * len2 + s1 + 7 * s2 + 1000 * g_mask);
}

template <class Code>
static hipError_t fake_launch(swmi::host::TileKind kind, bool affine, const uint8_t *s1, const uint8_t *s2, const swmi::TileWork *work,
                              size_t n, int waves, const int8_t *sm, int gap, int gap_extend, unsigned free_ends, int32_t *scores,
                              int32_t *ends, Code *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    CHECK(kind == g_f->kind);                                   // the kind's own launchers, no other's
    CHECK(n > 0 && work && sm && memcmp(sm, g_sm, 16) == 0 && gap == gap_of(affine) && gap_extend == extend_of(affine));
    CHECK(free_ends == g_mask && g_mask == mask_of(affine));
    CHECK(!moves == !counts && !moves == !codes);
    {
        std::lock_guard<std::mutex> l(g_launch_mu);
        g_launches.push_back({std::vector<swmi::TileWork>(work, work + n), waves, affine, moves != nullptr, st});
    }
    const size_t ne = g_f->n_ends;
    for (size_t x = 0; x < n; ++x) {
        const swmi::TileWork w = work[x];
        if (w.len1 == 0 || w.len2 == 0) {
            CHECK(waves == 1);
            const Zero z = g_f->zero(w.len1, w.len2, affine, free_ends, moves != nullptr);
            scores[w.k] = z.score;
            for (size_t e = 0; e < ne; ++e) ends[ne * w.k + e] = z.ends[e];
            if (moves) {
                counts[w.k] = z.count;
                CHECK((z.moves + 31) / 32 <= mw_of(w.len1, w.len2));
                for (size_t v = 0; v < (z.moves + 31) / 32; ++v) moves[w.move_base + v] = z.word;
            }
            continue;
        }
        uint32_t sums = 0;
        const int32_t sc = score_of(s1 + w.s1_off, w.len1, s2 + w.s2_off, w.len2, &sums);
        scores[w.k] = sc;
        for (size_t e = 0; e < ne; ++e) ends[ne * w.k + e] = sc + int32_t(e) + 1;
        if (!moves) continue;
        const size_t mw = mw_of(w.len1, w.len2);
        counts[w.k] = moves_of(sums, mw) + g_f->count_offset;
        for (size_t v = 0; v < mw; ++v) moves[w.move_base + v] = 0xC0DEull << 48 | uint64_t(uint32_t(sc)) << 16 | v;
        codes[w.code_base] = 1;
        codes[w.code_base + kCodeDwords * 4 / sizeof(Code) - 1] = 1;
    }
    return hipSuccess;
}

namespace swmi {
using host::kTileGlobal;
using host::kTileLocal;
using host::kTileSemiglobal;
static int fake_waves(int len1, int len2) { return len1 > 0 && len2 > 0 ? (len2 + 1023) / 1024 : 1; }
int local_full_ragged_waves(int len1, int len2) { return fake_waves(len1, len2); }
int global_full_ragged_waves(int len1, int len2) { return fake_waves(len1, len2); }
int sgfull_ragged_waves(int len1, int len2) { return fake_waves(len1, len2); }
hipError_t launch_local_full_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves, const int8_t *sm,
                                    int gap, int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves,
                                    uint32_t *steps, hipStream_t st)
{
    return fake_launch(kTileLocal, false, s1, s2, work, n, waves, sm, gap, 0, 0, scores, ends, codes, moves, steps, st);
}
hipError_t launch_local_full_affine_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves,
                                           const int8_t *sm, int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                           unsigned long long *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    return fake_launch(kTileLocal, true, s1, s2, work, n, waves, sm, gap_open, gap_extend, 0, scores, ends, codes, moves, steps, st);
}
hipError_t launch_global_full_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves, const int8_t *sm,
                                     int gap, unsigned free_ends, int32_t *scores, int32_t *ends, uint32_t *codes,
                                     unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    return fake_launch(kTileGlobal, false, s1, s2, work, n, waves, sm, gap, 0, free_ends, scores, ends, codes, moves, steps, st);
}
hipError_t launch_global_full_affine_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves,
                                            const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends, int32_t *scores,
                                            int32_t *ends, unsigned long long *codes, unsigned long long *moves, uint32_t *steps,
                                            hipStream_t st)
{
    return fake_launch(kTileGlobal, true, s1, s2, work, n, waves, sm, gap_open, gap_extend, free_ends, scores, ends, codes, moves, steps,
                       st);
}
hipError_t launch_sgfull_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves, const int8_t *sm, int gap,
                                int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *lengths,
                                hipStream_t st)
{
    return fake_launch(kTileSemiglobal, false, s1, s2, work, n, waves, sm, gap, 0, 0, scores, ends, codes, moves, lengths, st);
}
hipError_t launch_sgfull_affine_ragged(const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves, const int8_t *sm,
                                       int gap_open, int gap_extend, int32_t *scores, int32_t *ends, unsigned long long *codes,
                                       unsigned long long *moves, uint32_t *lengths, hipStream_t st)
{
    return fake_launch(kTileSemiglobal, true, s1, s2, work, n, waves, sm, gap_open, gap_extend, 0, scores, ends, codes, moves, lengths,
                       st);
}
}  // namespace swmi

// ---- the driver -------------------------------------------------------------------------------------------------------------
struct Batch {
    std::vector<uint64_t> off1, off2, mo;
    std::vector<uint8_t> s1, s2;
    size_t n() const { return off1.size() - 1; }
    size_t len1(size_t k) const { return size_t(off1[k + 1] - off1[k]); }
    size_t len2(size_t k) const { return size_t(off2[k + 1] - off2[k]); }
};

static uint32_t g_rng = 12345;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

// lengths that mix every wave count with zero lengths: len2 up to 16384 in every 16th alignment, else up to 3000; or, with
// `tiny`, both lengths below it
static Batch make_batch(size_t n, size_t tiny = 0)
{
    Batch b;
    b.off1.assign(1, 0);
    b.off2.assign(1, 0);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t r = rnd() >> 8;
        const size_t len1 = tiny ? r % tiny : r % 11 == 0 ? 0 : (rnd() >> 8) % 601;
        const size_t len2 = tiny ? (r >> 4) % tiny : r % 13 == 0 ? 0 : r % 16 == 1 ? (rnd() >> 8) % (kMax + 1) : (rnd() >> 8) % 3001;
        b.off1.push_back(b.off1.back() + len1);
        b.off2.push_back(b.off2.back() + len2);
    }
    b.s1.resize(b.off1.back() + 1);
    b.s2.resize(b.off2.back() + 1);
    for (auto &x : b.s1) x = uint8_t(rnd() >> 24);
    for (auto &x : b.s2) x = uint8_t(rnd() >> 24);
    // one move layout for all three kinds: the kind's move words in caller order, which swmi_local_full_ragged_move_offsets states
    b.mo.resize(n + 1);
    CHECK(swmi_local_full_ragged_move_offsets(b.off1.data(), b.off2.data(), n, b.mo.data()) == SWMI_OK && b.mo[0] == 0);
    for (size_t k = 0; k < n; ++k) CHECK(b.mo[k + 1] == b.mo[k] + mw_of(b.len1(k), b.len2(k)));
    return b;
}

static std::vector<size_t> slices(const Batch &b, size_t n, bool affine, bool tb)
{
    std::vector<size_t> s(g_f->slices_for(b.off1.data(), b.off2.data(), n, affine, tb, nullptr, 0));
    g_f->slices_for(b.off1.data(), b.off2.data(), n, affine, tb, s.data(), s.size());
    return s;
}

static std::vector<Launch> take_launches()
{
    std::lock_guard<std::mutex> l(g_launch_mu);
    std::vector<Launch> out;
    out.swap(g_launches);
    return out;
}

// the launches of a call over b[0, n) against its slices; returns the largest slice's code words
static size_t check_launches(const Batch &b, const std::vector<size_t> &sizes, const std::vector<Launch> &l, bool affine, bool tb,
                             hipStream_t only_stream)
{
    for (size_t k = 0; k < fake_hip_log_size(); ++k) CHECK(!strstr(fake_hip_log_at(k), " launch_"));     // no fixed-length launcher ran
    size_t at = 0, first = 0, max_codes = 0;
    std::vector<hipStream_t> slice_streams;
    for (size_t s = 0; s < sizes.size(); ++s) {
        std::vector<char> seen(sizes[s], 0);
        std::vector<std::pair<uint64_t, uint64_t>> code_ranges, move_ranges;
        size_t covered = 0;
        int last_waves = 17;
        hipStream_t stream = nullptr;
        while (covered < sizes[s]) {
            CHECK(at < l.size());
            const Launch &x = l[at++];
            CHECK(x.affine == affine && x.traceback == tb && x.waves >= 1 && x.waves < last_waves);     // descending wave count
            CHECK(covered == 0 || x.stream == stream);                                                    // one stream per slice
            CHECK(!only_stream || x.stream == only_stream);
            stream = x.stream;
            last_waves = x.waves;
            uint32_t last_len1 = UINT32_MAX;
            for (const swmi::TileWork &w : x.slots) {
                CHECK(w.k < sizes[s] && !seen[w.k]);
                seen[w.k] = 1;
                const size_t k = first + w.k;
                CHECK(w.len1 == b.len1(k) && w.len2 == b.len2(k));
                CHECK(w.s1_off == b.off1[k] - b.off1[first] && w.s2_off == b.off2[k] - b.off2[first]);
                CHECK(w.s1_off + w.len1 <= b.off1[first + sizes[s]] - b.off1[first]);
                CHECK(w.s2_off + w.len2 <= b.off2[first + sizes[s]] - b.off2[first]);
                CHECK(swmi::fake_waves(int(w.len1), int(w.len2)) == x.waves);
                CHECK(w.len1 && w.len2 ? true : x.waves == 1);                                            // a zero length: the W = 1 launch
                CHECK(w.len1 <= last_len1);                                                               // longest first
                last_len1 = w.len1;
                CHECK(w.move_base == b.mo[k] - b.mo[first]);
                if (tb && w.len1 && w.len2) code_ranges.push_back({w.code_base, w.code_base + code_words(affine)});
                if (tb && mw_of(w.len1, w.len2)) move_ranges.push_back({w.move_base, w.move_base + mw_of(w.len1, w.len2)});
            }
            covered += x.slots.size();
        }
        CHECK(covered == sizes[s]);
        for (auto *r : {&code_ranges, &move_ranges}) {
            std::sort(r->begin(), r->end());
            for (size_t i = 1; i < r->size(); ++i) CHECK((*r)[i - 1].second <= (*r)[i].first);
        }
        if (!code_ranges.empty()) {
            CHECK(code_ranges.back().second == code_ranges.size() * code_words(affine));                          // one block, no holes
            max_codes = std::max(max_codes, size_t(code_ranges.back().second));
        }
        if (!move_ranges.empty()) CHECK(move_ranges.back().second <= b.mo[first + sizes[s]] - b.mo[first]);
        slice_streams.push_back(stream);
        first += sizes[s];
    }
    CHECK(at == l.size());
    for (size_t s = 1; !only_stream && s < sizes.size(); ++s) CHECK(slice_streams[s] != slice_streams[s - 1]);   // two buffer sets
    return max_codes;
}

// every result at its caller position; `ends` holds n_ends * n int32 and the sentinel pair, `moves` the sentinel behind mo[n]
static void check_results(const Batch &b, size_t n, bool affine, bool tb, const int32_t *scores, const int32_t *ends, const uint64_t *moves,
                          const uint32_t *counts)
{
    const size_t ne = g_f->n_ends;
    for (size_t k = 0; k < n; ++k) {
        const size_t len1 = b.len1(k), len2 = b.len2(k), mw = mw_of(len1, len2);
        bool ok = true;
        if (!len1 || !len2) {
            const Zero z = g_f->zero(len1, len2, affine, mask_of(affine), tb);
            ok = scores[k] == z.score && (!tb || counts[k] == z.count);
            for (size_t e = 0; e < ne; ++e) ok = ok && ends[ne * k + e] == z.ends[e];
            for (size_t v = 0; tb && v < (z.moves + 31) / 32; ++v) ok = ok && v < mw && moves[b.mo[k] + v] == z.word;
        } else {
            uint32_t sums = 0;
            const int32_t sc = score_of(b.s1.data() + b.off1[k], len1, b.s2.data() + b.off2[k], len2, &sums);
            ok = scores[k] == sc;
            for (size_t e = 0; e < ne; ++e) ok = ok && ends[ne * k + e] == sc + int32_t(e) + 1;
            if (tb) {
                ok = ok && counts[k] == moves_of(sums, mw) + g_f->count_offset;
                for (size_t v = 0; v < mw; ++v) ok = ok && moves[b.mo[k] + v] == (0xC0DEull << 48 | uint64_t(uint32_t(sc)) << 16 | v);
            }
        }
        if (!ok) {
            fprintf(stderr, "alignment %zu (%zu x %zu) has wrong results\n", k, len1, len2);
            exit(1);
        }
    }
    CHECK(ends[ne * n] == kEndSentinel && ends[ne * n + 1] == kEndSentinel);      // nothing past the kind's ends per alignment
    if (tb) CHECK(moves[b.mo[n]] == kSentinel);
}

static void host_case(bool affine, const Batch &b, size_t n, bool tb)
{
    const std::vector<size_t> sizes = slices(b, n, affine, tb);
    std::vector<int32_t> scores(n, -7), ends(g_f->n_ends * n + 2, -7);
    ends[g_f->n_ends * n] = ends[g_f->n_ends * n + 1] = kEndSentinel;
    std::vector<uint64_t> moves(tb ? b.mo[n] + 1 : 0, kSentinel);
    std::vector<uint32_t> counts(tb ? n : 0, 77);
    fake_hip_log_clear();
    take_launches();
    g_mask = mask_of(affine);
    CHECK(g_f->host(affine, b.s1.data(), b.off1.data(), b.s2.data(), b.off2.data(), n, gap_of(affine), extend_of(affine), g_mask,
                    scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? counts.data() : nullptr) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    check_launches(b, sizes, l, affine, tb, nullptr);
    check_results(b, n, affine, tb, scores.data(), ends.data(), tb ? moves.data() : nullptr, tb ? counts.data() : nullptr);
    if (tb) {
        // a slice's moves come back as ONE copy of exactly its words
        std::vector<size_t> want, got;
        for (size_t s = 0, first = 0; s < sizes.size(); first += sizes[s++])
            if (b.mo[first + sizes[s]] != b.mo[first]) want.push_back(size_t(b.mo[first + sizes[s]] - b.mo[first]) * 8);
        for (size_t k = 0; k < fake_hip_log_size(); ++k) {
            size_t bytes = 0;
            const char *m = strstr(fake_hip_log_at(k), "memcpy kind2 bytes");
            if (m && sscanf(m, "memcpy kind2 bytes%zu", &bytes) == 1 && std::find(want.begin(), want.end(), bytes) != want.end())
                got.push_back(bytes);
        }
        CHECK(got == want);
    }
    printf("  host %-6s n %6zu %-10s: %zu slices, %zu launches: ok\n", affine ? "affine" : "linear", n, tb ? "traceback" : "ends-only",
           sizes.size(), l.size());
}

// one device-entry call on `st` over b[0, n); returns the log of the call
static std::vector<std::string> device_case(bool affine, const Batch &b, size_t n, bool tb, hipStream_t st, size_t *max_codes)
{
    const std::vector<size_t> sizes = slices(b, n, affine, tb);
    const size_t ne = g_f->n_ends;
    void *s1, *s2, *scores, *ends, *moves = nullptr, *counts = nullptr;
    CHECK(hipMalloc(&s1, b.off1[n] + 1) == hipSuccess && hipMalloc(&s2, b.off2[n] + 1) == hipSuccess);
    CHECK(hipMalloc(&scores, n * 4) == hipSuccess && hipMalloc(&ends, (ne * n + 2) * 4) == hipSuccess);
    if (tb) CHECK(hipMalloc(&moves, (b.mo[n] + 1) * 8) == hipSuccess && hipMalloc(&counts, n * 4) == hipSuccess);
    memcpy(s1, b.s1.data(), b.off1[n]);
    memcpy(s2, b.s2.data(), b.off2[n]);
    static_cast<int32_t *>(ends)[ne * n] = static_cast<int32_t *>(ends)[ne * n + 1] = kEndSentinel;
    if (tb)
        for (size_t w = 0; w <= b.mo[n]; ++w) static_cast<uint64_t *>(moves)[w] = kSentinel;
    fake_hip_log_clear();
    take_launches();
    g_mask = mask_of(affine);
    CHECK(g_f->device(affine, s1, b.off1.data(), s2, b.off2.data(), n, gap_of(affine), extend_of(affine), g_mask, scores, ends, moves, counts,
                      st) == SWMI_OK);
    const std::vector<Launch> l = take_launches();
    *max_codes = check_launches(b, sizes, l, affine, tb, st);
    check_results(b, n, affine, tb, static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                  static_cast<uint32_t *>(counts));
    std::vector<std::string> log;
    for (size_t k = 0; k < fake_hip_log_size(); ++k) log.push_back(fake_hip_log_at(k));
    for (void *p : {s1, s2, scores, ends, moves, counts})
        if (p) CHECK(hipFree(p) == hipSuccess);
    printf("  device %-6s n %6zu %-10s: %zu slices, %zu launches: ok\n", affine ? "affine" : "linear", n, tb ? "traceback" : "ends-only",
           sizes.size(), l.size());
    return log;
}

static bool has(const std::vector<std::string> &log, const std::string &part)
{
    for (const std::string &l : log)
        if (l.find(part) != std::string::npos) return true;
    return false;
}

// the workspace of a device call: the largest slice's codes (16-byte rounded), then n slots
static std::string workspace_malloc(size_t max_codes, bool affine, size_t n)
{
    const size_t code_bytes = (max_codes * (affine ? 8 : 4) + 15) & ~size_t(15);
    return "malloc bytes" + std::to_string(code_bytes + n * sizeof(swmi::TileWork));
}

static void plan_only_case()
{
    fake_hip_real_code_sizes(1);
    const size_t n = 300;
    std::vector<uint64_t> off(n + 1);
    for (size_t k = 0; k <= n; ++k) off[k] = k * uint64_t(kMax);
    std::vector<size_t> sizes, bytes;
    fake_hip_log_clear();
    CHECK(swmi::host::tile_ragged_plan_check(g_f->kind, off.data(), off.data(), n, true, true, &sizes, &bytes));
    const size_t qwords = real_code_words(kMax, kMax);
    CHECK(qwords == size_t(16) * 4112 * 256);
    // the fixed-length affine aligner's traceback budget: 256 alignments of 16384 x 16384 with the kind's ends each
    const size_t budget = 256 * (2 * size_t(kMax) + 4 + 4 * g_f->n_ends + qwords * 8 + mw_of(kMax, kMax) * 8 + 4);
    CHECK(sizes.size() == 2 && sizes[0] == 255 && sizes[1] == 45);
    for (size_t b : bytes) CHECK(b <= budget);
    // slice 0's codes: just under 2^32 qwords, so its last code bases pass 2^32 counted in dwords (the pipeline's unit) and
    // 2^35 counted in bytes
    CHECK(uint64_t(sizes[0] - 1) * qwords * 2 > (uint64_t(1) << 32) && uint64_t(sizes[0]) * qwords > (uint64_t(1) << 31));
    CHECK(g_f->slices_for(off.data(), off.data(), n, 1, 1, nullptr, 0) == 2);
    CHECK(fake_hip_log_size() == 0);                                          // no device was touched
    fake_hip_real_code_sizes(0);
    printf("  plan only, 300 x (16384 x 16384) affine traceback: slices 255 + 45, code bases past 2^32 dwords: ok\n");
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    for (const Family &f : kFamilies)
        if (argv[1] == std::string(f.name)) g_f = &f;
    CHECK(g_f && "unknown kind");
    for (int i = 0; i < 16; ++i) g_sm[i] = int8_t(i % 5 == 0 ? 1 : -1);
    static_assert(sizeof(swmi::TileWork) == 48, "the slot the budget counts");
    // every argument error and n = 0 come back before any device is touched
    const uint64_t dec[3] = {0, 5, 3}, inc[3] = {0, 0, 0};
    uint8_t byte = 0;
    int32_t out[8];
    uint64_t mv[2];
    const auto refusal = [&](bool affine, const uint64_t *off, size_t n, int gap, int extend, unsigned mask, int32_t *o, uint64_t *moves) {
        return g_f->host(affine, o ? &byte : nullptr, off, o ? &byte : nullptr, off, n, gap, extend, mask, o, o, moves, nullptr);
    };
    CHECK(refusal(false, dec, 0, 1, 0, 0, nullptr, nullptr) == SWMI_OK);
    CHECK(refusal(false, dec, 2, 1, 0, 0, out, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
    CHECK(refusal(true, inc, 2, 1, 1, 0, out, mv) == SWMI_ERR_INVALID_ARGUMENT);           // moves without the count, under its name
    CHECK(swmi_last_error() == std::string("moves and ") + g_f->count + " must both be given (traceback) or both be NULL (ends-only)");
    CHECK(refusal(true, inc, 2, 1, 128, 0, out, nullptr) == SWMI_ERR_DOMAIN);
    if (g_f->mask) CHECK(refusal(true, inc, 2, 1, 1, 16, out, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
    CHECK(fake_hip_log_size() == 0);
    plan_only_case();
    CHECK(swmi_init(0) == SWMI_OK);

    // traceback: slices of a few thousand alignments by the byte budget; ends-only: lengths 0 .. 4, slices by the count cap
    const Batch b = make_batch(20000), tiny = make_batch((size_t(5) << 19) + 3, 5);
    for (int affine = 0; affine < 2; ++affine) {
        const size_t s = slices(b, b.n(), affine, true)[0];
        CHECK(s > 1 && 2 * s + s / 2 <= b.n());
        for (size_t n : {size_t(1), s, s + 1, 2 * s + s / 2}) host_case(affine, b, n, true);
        const size_t e = slices(tiny, tiny.n(), affine, false)[0];
        CHECK(e == size_t(1) << 20 && 2 * e + e / 2 <= tiny.n());
        for (size_t n : {size_t(1), e, e + 1, 2 * e + e / 2}) host_case(affine, tiny, n, false);
    }
    host_case(false, b, b.n(), false);                        // every wave count in one ends-only slice

    // device entry on two streams; the second call on stream A grows its workspace (after synchronising that stream)
    hipStream_t sa, sb;
    CHECK(hipStreamCreateWithFlags(&sa, 0) == hipSuccess && hipStreamCreateWithFlags(&sb, 0) == hipSuccess);
    fake_hip_log_clear();
    CHECK(hipStreamSynchronize(sa) == hipSuccess && hipStreamSynchronize(sb) == hipSuccess);
    int ida = 0, idb = 0;
    CHECK(sscanf(fake_hip_log_at(0), "dev0 stream_sync stream%d", &ida) == 1 && sscanf(fake_hip_log_at(1), "dev0 stream_sync stream%d", &idb) == 1);
    const size_t s = slices(b, b.n(), false, true)[0], big = 2 * s + s / 2;
    size_t codes = 0;
    std::vector<std::string> log = device_case(false, b, 3, true, sa, &codes);
    CHECK(has(log, workspace_malloc(codes, false, 3)));
    log = device_case(false, b, big, true, sb, &codes);
    CHECK(has(log, workspace_malloc(codes, false, big)));
    log = device_case(false, b, big, true, sa, &codes);
    CHECK(log.size() >= 2 && log[0] == "dev0 stream_sync stream" + std::to_string(ida) && has({log[1]}, workspace_malloc(codes, false, big)));
    log = device_case(false, b, 5, true, sb, &codes);           // fits: the workspace is not allocated again
    CHECK(!has(log, "dev0 malloc bytes"));
    log = device_case(true, b, big, true, sa, &codes);          // the affine aligner has a state of its own
    CHECK(has(log, workspace_malloc(codes, true, big)));
    log = device_case(true, b, 700, false, sb, &codes);         // ends-only: slots only
    CHECK(codes == 0 && has(log, workspace_malloc(0, true, 700)));

    CHECK(g_f->release[0]() == SWMI_OK && g_f->release[1]() == SWMI_OK);
    host_case(false, b, s + 1, true);
    CHECK(g_f->release[0]() == SWMI_OK);
    CHECK(hipStreamDestroy(sa) == hipSuccess && hipStreamDestroy(sb) == hipSuccess);
    CHECK(swmi_shutdown() == SWMI_OK);
    printf("tile ragged host fake ok: %s\n", g_f->name);
    return 0;
}
