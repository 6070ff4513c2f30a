// wide_api.cpp -- the C entries of libswmi_wide.so (include/swmi_wide.h) and, compiled a second time
// with -DSWMI_WIDE_LONG_LIBRARY, of libswmi_wide_long.so (include/swmi_wide_long.h, section 30): the wide-alphabet local and
// global aligners on a batch of mixed (len1, len2).  Everything in which the two libraries differ stands in the one block
// below the error text (section 31); nothing after it tests the define.  Self-contained: no Context of libswmi.so, no swmi_init -- every entry runs on the calling thread's
// current HIP device, with this file's own workspaces per (device, stream), its own two streams and buffer sets per device for
// the host entries, and its own thread-local error text.  Of libswmi.so, linked for the callers' expander, it calls nothing:
// the move layout is a sum of SWMI_LOCAL_LONG_MOVE_WORDS that this file makes itself.  The planner is DESIGN.md section 19's,
// as tile_ragged_api.cpp has it, with a class of slots in front of the wave counts: slices contiguous in caller order within
// a byte budget; inside a slice the alignments that the striped kernels of wide_long_affine_kernels.hip take
// (wide_long_internal.h) in one launch of the process's stripe width, then one launch of wide_affine_kernels.hip per wave
// count, widest first, longest seq1 first, results at caller positions.  A striped slot of more than 1024 columns owns a carry
// block behind the slice's codes.  This file's name lies outside csrc/swmi_*.cpp, which four host-only test programs glob.
#include "wide_long_internal.h"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace swmi {
namespace wide {
namespace {

thread_local char t_error[512] = "";

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_error, sizeof t_error, fmt, ap);
    va_end(ap);
    return code;
}

int check_both(const uint64_t *off1, const uint64_t *off2, size_t n);
void fill_move_offsets(const uint64_t *off1, const uint64_t *off2, size_t n, uint64_t *out);

}  // namespace
}  // namespace wide
}  // namespace swmi

// ---- what the two libraries differ in: the public header, the prefix of the exported names, the limits on len1 and len2,
// ---- the traceback budget, and whether there is a striped class of slots with its width rule and its two entries ----
#ifdef SWMI_WIDE_LONG_LIBRARY
#include "../../include/swmi_wide_long.h"
#define WIDE_ENTRY(name) swmi_wide_long_##name

namespace swmi {
namespace wide {
namespace {
constexpr size_t kMaxLen1 = SWMI_WIDE_LONG_MAX_LEN, kMaxLen2 = SWMI_WIDE_LONG_MAX_LEN;
// a traceback slice: what this many of the largest shape take (section 23's affine figure)
constexpr size_t kTbSliceAlignments = 16;
constexpr bool kHasStriped = true;
static_assert(kWideLongMaxLen == SWMI_WIDE_LONG_MAX_LEN && SWMI_WIDE_LONG_LOCAL == SWMI_WIDE_LOCAL && SWMI_WIDE_LONG_GLOBAL == SWMI_WIDE_GLOBAL);

// the stripe width of the process: 0 = the rule below
std::atomic<int> g_width{0};

// The stripe width of a launch of n striped slots (DESIGN.md section 30 has the measurement).  Either width keeps four
// wavefronts on a CU, whose LDS holds four profiles: one workgroup of 4 or four of 1.  4 wavefronts finish an alignment four
// times sooner and won every row of 256 alignments or fewer, by 3.6 - 3.9x; 1 wavefront has no barrier and no pipeline fill
// and won the row of 4096, by 1.24 - 1.73x.  Between them nothing was measured: the rule turns where the launch fills every
// slot of the machine at 1 wavefront, 256 CUs x 4 workgroups, which is supposed from the code.
constexpr size_t kNarrowFrom = 1024;
int stripe_width(size_t n)
{
    const int w = g_width.load(std::memory_order_relaxed);
    if (w) return w;
    return n >= kNarrowFrom ? 1 : 4;
}
}  // namespace
}  // namespace wide
}  // namespace swmi

extern "C" int swmi_wide_long_set_stripe_waves(int waves)
{
    using namespace swmi;
    bool shipped = waves == 0;
    for (int w : kWideLongWidths) shipped = shipped || w == waves;
    if (!shipped) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "stripe width %d is not shipped (0 = the library's rule, 1 or 4 wavefronts)", waves);
    wide::g_width.store(waves, std::memory_order_relaxed);
    return SWMI_OK;
}

extern "C" int swmi_wide_long_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, uint64_t *move_offsets)
{
    using namespace swmi;
    if (!move_offsets) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "move_offsets is NULL");
    const int rc = wide::check_both(seq1_offsets, seq2_offsets, n);
    if (rc != SWMI_OK) return rc;
    wide::fill_move_offsets(seq1_offsets, seq2_offsets, n, move_offsets);
    return SWMI_OK;
}
#else
#include "../../include/swmi_wide.h"
#define WIDE_ENTRY(name) swmi_wide_##name

namespace swmi {
namespace wide {
namespace {
constexpr size_t kMaxLen1 = SWMI_WIDE_MAX_LEN1, kMaxLen2 = SWMI_WIDE_MAX_LEN2;
constexpr size_t kTbSliceAlignments = 256;               // a traceback slice: what this many of the largest shape take
// No striped class: within these limits wide_long_striped is false for every shape, so no slot owns a carry block, and
// libswmi_wide.so, which does not link wide_long_affine_kernels.o, names nothing of that file.
constexpr bool kHasStriped = false;
constexpr int stripe_width(size_t) { return 0; }         // (named in a discarded statement only)
}  // namespace
}  // namespace wide
}  // namespace swmi
#endif

namespace swmi {
namespace wide {
namespace {

#define WIDE_HIP_TRY(expr)                                                                                          \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) return fail(SWMI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr size_t kMatrixBytes = SWMI_WIDE_LETTERS * SWMI_WIDE_LETTERS;
constexpr size_t kSliceBytes = size_t(256) << 20;        // an ends-only slice's device bytes
constexpr size_t kMaxSlice = size_t(1) << 20;            // alignments per slice (and per launch)
// classes of a slice's slots: the striped one where the library has it, then the unstriped wave counts 4 .. 1
constexpr int kClasses = kWideMaxWaves + (kHasStriped ? 1 : 0);
constexpr uint32_t kCarryUnit = 2;                       // int2 per unit of TileWork::pad: carry blocks start 16-byte aligned
static_assert(kWideMaxLen1 == SWMI_WIDE_MAX_LEN1 && kWideMaxLen2 == SWMI_WIDE_MAX_LEN2);
static_assert(kHasStriped || (kMaxLen1 <= size_t(kWideMaxLen1) && kMaxLen2 <= size_t(kWideMaxLen2)),
              "without the striped class every accepted shape must be the unstriped kernels'");
static_assert(sizeof(TileWork) == 48 && kMatrixBytes % 16 == 0);
// one move layout for both libraries: the two macros of swmi.h are the same expression
static_assert(SWMI_LOCAL_LONG_MOVE_WORDS(0, 0) == SWMI_LOCAL_FULL_MOVE_WORDS(0, 0) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(1, 0) == SWMI_LOCAL_FULL_MOVE_WORDS(1, 0) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(31, 2) == SWMI_LOCAL_FULL_MOVE_WORDS(31, 2) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(300, 1025) == SWMI_LOCAL_FULL_MOVE_WORDS(300, 1025) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(16384, 4096) == SWMI_LOCAL_FULL_MOVE_WORDS(16384, 4096));

// ---- the planner ----
// whether the striped kernels take the alignment
bool striped(size_t len1, size_t len2) { return kHasStriped && wide_long_striped(len1, len2); }

size_t code_qwords(size_t len1, size_t len2)
{
    if (!len1 || !len2) return 0;
    if constexpr (kHasStriped)
        if (striped(len1, len2)) return wide_long_code_qwords((int)len1, (int)len2);
    return wide_affine_code_qwords((int)len1, (int)len2);
}

// whether the slot owns a carry block: a striped slot of more than one stripe at the narrowest width shipped (at a wider
// stripe some of these blocks stay unused; the plan does not depend on the width)
bool has_carry(size_t len1, size_t len2) { return striped(len1, len2) && len2 > size_t(1024 * kWideLongMinWidth); }

// its units of TileWork::pad
size_t carry_units(size_t len1) { return (len1 + kCarryUnit - 1) / kCarryUnit; }

// the class of a slot: kClasses = striped (kWideMaxWaves + 1), else its unstriped wave count
int slot_class(size_t len1, size_t len2) { return striped(len1, len2) ? kClasses : wide_ragged_waves((int)len1, (int)len2); }

// device bytes one alignment of a slice takes: inputs, its slot, results, its carry (8 len1) where it has one, and with a
// traceback codes, moves and count
size_t ragged_bytes(bool tb, size_t len1, size_t len2)
{
    size_t b = len1 + len2 + sizeof(TileWork) + 5 * sizeof(int32_t);
    if (has_carry(len1, len2)) b += len1 * sizeof(int2);
    if (tb) b += code_qwords(len1, len2) * sizeof(uint64_t) + SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

size_t budget(bool tb) { return tb ? kTbSliceAlignments * ragged_bytes(true, kMaxLen1, kMaxLen2) : kSliceBytes; }

int check_offsets(const char *name, const uint64_t *off, size_t n, size_t max_len)
{
    if (!off) return fail(SWMI_ERR_INVALID_ARGUMENT, "%s is NULL", name);
    for (size_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return fail(SWMI_ERR_INVALID_ARGUMENT, "%s decrease at %zu", name, k);
        if (off[k + 1] - off[k] > max_len)
            return fail(SWMI_ERR_INVALID_ARGUMENT, "%s: sequence %zu has length %llu > %zu", name, k,
                        (unsigned long long)(off[k + 1] - off[k]), max_len);
    }
    return SWMI_OK;
}

int check_both(const uint64_t *off1, const uint64_t *off2, size_t n)
{
    const int rc = check_offsets("seq1_offsets", off1, n, kMaxLen1);
    return rc != SWMI_OK ? rc : check_offsets("seq2_offsets", off2, n, kMaxLen2);
}

void fill_move_offsets(const uint64_t *off1, const uint64_t *off2, size_t n, uint64_t *out)
{
    out[0] = 0;
    for (size_t k = 0; k < n; ++k) out[k + 1] = out[k] + SWMI_LOCAL_LONG_MOVE_WORDS(off1[k + 1] - off1[k], off2[k + 1] - off2[k]);
}

// Slices of checked offsets: each the longest run from where the last one ended whose ragged_bytes fit the budget, at most
// kMaxSlice alignments and at least one.  first = {0, ..., n}.
std::vector<size_t> cut(const uint64_t *off1, const uint64_t *off2, size_t n, bool tb)
{
    const size_t cap = budget(tb);
    std::vector<size_t> first{0};
    size_t bytes = 0, m = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t b = ragged_bytes(tb, size_t(off1[k + 1] - off1[k]), size_t(off2[k + 1] - off2[k]));
        if (m && (bytes + b > cap || m == kMaxSlice)) {
            first.push_back(k);
            bytes = m = 0;
        }
        bytes += b;
        ++m;
    }
    if (n) first.push_back(n);
    return first;
}

struct Plan {
    const uint64_t *off1 = nullptr, *off2 = nullptr;
    std::vector<uint64_t> move_offsets;         // n + 1
    std::vector<size_t> first;                  // slice s = alignments [first[s], first[s + 1])
    std::vector<TileWork> tiles;                // [n]: slice s's slots at [first[s], first[s + 1]), everything slice-relative
    // per slice: the slots of class C lie at [start[kClasses - C], start[kClasses - C + 1]) of the slice's slots
    std::vector<std::array<uint32_t, kClasses + 1>> start;
    std::vector<size_t> code_qwords;            // per slice
    size_t max_m = 0, max_seq1 = 0, max_seq2 = 0, max_codes = 0, max_moves = 0, max_carry = 0;   // the largest slice's (carry: in int2)
    size_t slices() const { return first.size() - 1; }
};

// The plan of a checked batch.  Every TileWork offset and base is a 64-bit running sum relative to its slice; code bases run
// in caller order; carry blocks run in slot order, TileWork::pad in units of kCarryUnit.  Inside a slice: class descending
// (striped first), then len1 descending, then caller order (a stable sort).
int make_plan(Plan &p, const uint64_t *off1, const uint64_t *off2, size_t n, bool tb)
{
    p.off1 = off1;
    p.off2 = off2;
    p.move_offsets.assign(n + 1, 0);
    if (tb) fill_move_offsets(off1, off2, n, p.move_offsets.data());
    p.first = cut(off1, off2, n, tb);
    p.tiles.resize(n);
    p.start.resize(p.slices());
    p.code_qwords.assign(p.slices(), 0);
    std::vector<uint32_t> order;
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s], b = p.first[s + 1];
        auto len1 = [&](size_t k) { return uint32_t(off1[k + 1] - off1[k]); };
        auto len2 = [&](size_t k) { return uint32_t(off2[k + 1] - off2[k]); };
        auto waves = [&](size_t k) { return slot_class(len1(k), len2(k)); };
        order.resize(b - a);
        for (size_t x = 0; x < b - a; ++x) order[x] = uint32_t(x);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            const int wx = waves(a + x), wy = waves(a + y);
            return wx != wy ? wx > wy : len1(a + x) > len1(a + y);
        });
        std::vector<uint64_t> code_base(b - a);
        uint64_t codes = 0;
        for (size_t k = a; k < b; ++k) {
            code_base[k - a] = codes;
            if (tb) codes += code_qwords(len1(k), len2(k));
        }
        std::array<uint32_t, kClasses + 1> &start = p.start[s];
        start.fill(uint32_t(b - a));
        int next = kClasses;                     // the class whose start is to be written next
        size_t carry = 0;                        // units of kCarryUnit
        for (size_t x = 0; x < b - a; ++x) {
            const size_t k = a + order[x];
            for (; next >= waves(k); --next) start[kClasses - next] = uint32_t(x);
            const bool owns = has_carry(len1(k), len2(k));
            if (owns && carry + carry_units(len1(k)) > size_t(0xFFFFFFFFu)) return fail(SWMI_ERR_INVALID_ARGUMENT, "slice %zu: carry blocks past 2^32 units", s);
            p.tiles[a + x] = {off1[k] - off1[a], off2[k] - off2[a], code_base[k - a], p.move_offsets[k] - p.move_offsets[a],
                              uint32_t(k - a), len1(k), len2(k), owns ? uint32_t(carry) : 0u};
            if (owns) carry += carry_units(len1(k));
        }
        p.max_carry = std::max(p.max_carry, carry * kCarryUnit);
        p.code_qwords[s] = size_t(codes);
        p.max_m = std::max(p.max_m, b - a);
        p.max_seq1 = std::max(p.max_seq1, size_t(off1[b] - off1[a]));
        p.max_seq2 = std::max(p.max_seq2, size_t(off2[b] - off2[a]));
        p.max_codes = std::max(p.max_codes, p.code_qwords[s]);
        p.max_moves = std::max(p.max_moves, size_t(p.move_offsets[b] - p.move_offsets[a]));
    }
    return SWMI_OK;
}

struct Params {
    WideKind kind;
    const int8_t *sm;
    int gap_open, gap_extend;
    unsigned free_ends;
};

// the launches of slice s on the one stream: the striped slots first, at the process's stripe width, then one launch per
// unstriped wave count present, widest first
hipError_t launch_slice(const Plan &p, size_t s, const Params &c, const uint8_t *s1, const uint8_t *s2, const TileWork *work,
                        const int8_t *d_sm, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                        uint32_t *counts, void *carry, hipStream_t st)
{
    const auto &start = p.start[s];
    if constexpr (kHasStriped) {
        if (start[1] > start[0]) {
            const size_t m = start[1] - start[0];
            const hipError_t e = launch_wide_long_affine_ragged(c.kind, s1, s2, work + start[0], m, stripe_width(m), d_sm, c.gap_open, c.gap_extend,
                                                                c.free_ends, scores, ends, codes, moves, counts, carry, kCarryUnit, st);
            if (e != hipSuccess) return e;
        }
    }
    for (int waves = kWideMaxWaves; waves >= 1; --waves) {
        const uint32_t a = start[kClasses - waves], b = start[kClasses - waves + 1];
        if (a == b) continue;
        const hipError_t e = launch_wide_affine_ragged(c.kind, s1, s2, work + a, size_t(b - a), waves, d_sm, c.gap_open, c.gap_extend,
                                                       c.free_ends, scores, ends, codes, moves, counts, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- device state: one per HIP device, made on first use ----
template <class T> int grow(T *&p, size_t &have, size_t need)
{
    if (have >= need) return SWMI_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    have = 0;
    WIDE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), need * sizeof(T)));
    have = need;
    return SWMI_OK;
}

struct HostSet {
    hipStream_t stream = nullptr;
    uint8_t *d1 = nullptr, *d2 = nullptr;
    int8_t *d_sm = nullptr;
    int32_t *d_scores = nullptr, *d_ends = nullptr;
    unsigned long long *d_codes = nullptr, *d_moves = nullptr;
    uint32_t *d_counts = nullptr;
    TileWork *d_work = nullptr;
    int2 *d_carry = nullptr;
    struct { size_t d1, d2, sm, scores, ends, codes, moves, counts, work, carry; } have{};
    size_t off = 0, m = 0;                          // slice in flight
    void release()
    {
        for (void *q : {(void *)d1, (void *)d2, (void *)d_sm, (void *)d_scores, (void *)d_ends, (void *)d_codes, (void *)d_moves,
                        (void *)d_counts, (void *)d_work, (void *)d_carry})
            if (q) (void)hipFree(q);
        if (stream) (void)hipStreamDestroy(stream);      // (made again by the next host call)
        *this = HostSet{};
    }
};

// a stream's workspace of the device entries -- codes of one slice, behind them its carry blocks, the matrix, the call's
// slots -- and the pinned copy of matrix and slots that the upload reads; `done` is recorded behind the upload
struct StreamSpace {
    unsigned char *dev = nullptr, *host = nullptr;
    size_t dev_bytes = 0, host_bytes = 0;
    hipEvent_t done = nullptr;
};

struct DeviceState {
    std::mutex ws_mu;                               // the device entries' workspaces
    std::map<hipStream_t, StreamSpace> spaces;
    std::mutex host_mu;                             // the host entries' sets
    HostSet sets[2];
    void release()
    {
        for (auto &x : spaces) {
            if (x.second.dev) (void)hipFree(x.second.dev);
            if (x.second.host) (void)hipHostFree(x.second.host);
            if (x.second.done) (void)hipEventDestroy(x.second.done);
        }
        spaces.clear();
        for (auto &s : sets) s.release();
    }
};

std::mutex g_mu;
std::map<int, DeviceState> g_devices;               // never erased: a reference stays valid

// the current device's state; the device must be gfx950
int current(DeviceState **out)
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return fail(SWMI_ERR_NO_DEVICE, "no current HIP device");
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_devices.find(dev);
    if (it == g_devices.end()) {
        hipDeviceProp_t prop{};
        WIDE_HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(SWMI_ERR_UNSUPPORTED_ARCH, "device %d is %s, not gfx950", dev, prop.gcnArchName);
        it = g_devices.emplace(std::piecewise_construct, std::forward_as_tuple(dev), std::forward_as_tuple()).first;
    }
    *out = &it->second;
    return SWMI_OK;
}

// ---- the entries' bodies ----
// The checks in the order of the 4-letter ragged entries: the mask, the matrix and the gaps, the moves / steps pair; then
// n = 0, the buffers, the lengths, which lie in the offsets, and last the global kind's domain rule.  1 = nothing to do.
int check_call(const Params &c, const void *seq1s, const uint64_t *off1, const void *seq2s, const uint64_t *off2, size_t n,
               const void *scores, const void *ends, const void *moves, const void *counts)
{
    if (c.kind == kWideGlobal && c.free_ends > SWMI_ENDS_OVERLAP)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", c.free_ends, SWMI_ENDS_OVERLAP);
    if (!c.sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (c.gap_open < 0 || c.gap_open > 127 || c.gap_extend < 0 || c.gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", c.gap_open, c.gap_extend);
    if (!moves != !counts)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return 1;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    const int rc = check_both(off1, off2, n);
    if (rc != SWMI_OK || c.kind != kWideGlobal) return rc;
    // the global kind's domain rule (wide_long_affine_kernels.hip): P (len1 + len2) <= 2^23
    static_assert(kHasStriped || 128 * (kMaxLen1 + kMaxLen2) <= (size_t(1) << 23),
                  "without the striped class the rule must hold for every int8 matrix at the limits, so that it refuses nothing");
    int lo = 0, hi = 0;                          // (two reductions the compiler vectorises; the short build pays for them too)
    for (size_t x = 0; x < kMatrixBytes; ++x) {
        lo = std::min(lo, int(c.sm[x]));
        hi = std::max(hi, int(c.sm[x]));
    }
    const long P = std::max({1, c.gap_open, c.gap_extend, -lo, hi});
    for (size_t k = 0; k < n; ++k) {
        const unsigned long long total = (off1[k + 1] - off1[k]) + (off2[k + 1] - off2[k]);
        if ((unsigned long long)P * total > (1ull << 23))
            return fail(SWMI_ERR_INVALID_ARGUMENT, "alignment %zu is outside the domain: P (len1 + len2) = %ld x %llu > 2^23 (P = max(1, max |score_matrix|, gap_open, gap_extend))",
                        k, P, total);
    }
    return SWMI_OK;
}

int run_device(const Params &c, const void *d_seq1s, const uint64_t *off1, const void *d_seq2s, const uint64_t *off2, size_t n,
               void *d_scores, void *d_ends, void *d_moves, void *d_counts, void *stream)
{
    int rc = check_call(c, d_seq1s, off1, d_seq2s, off2, n, d_scores, d_ends, d_moves, d_counts);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_counts)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    const bool tb = d_moves != nullptr;
    Plan p;
    rc = make_plan(p, off1, off2, n, tb);
    if (rc != SWMI_OK) return rc;
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one workspace per (device, stream), looked up, grown and handed to the launches under one lock (growing waits for this
    // stream only: earlier launches on it may still use the old one)
    std::lock_guard<std::mutex> lock(ds->ws_mu);
    StreamSpace &sp = ds->spaces[st];
    const size_t codes_only = ((tb ? p.max_codes * sizeof(uint64_t) : 0) + 15) & ~size_t(15);
    const size_t code_bytes = codes_only + p.max_carry * sizeof(int2);       // (the carry: whole units of 16 bytes)
    const size_t up_bytes = kMatrixBytes + n * sizeof(TileWork);
    if (code_bytes + up_bytes > sp.dev_bytes) {
        WIDE_HIP_TRY(hipStreamSynchronize(st));
        if (sp.dev) (void)hipFree(sp.dev);
        sp.dev = nullptr;
        sp.dev_bytes = 0;
        WIDE_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sp.dev), code_bytes + up_bytes));
        sp.dev_bytes = code_bytes + up_bytes;
    }
    // matrix and slots go up from pinned memory that the stream's last upload has finished reading
    if (sp.done) WIDE_HIP_TRY(hipEventSynchronize(sp.done));
    else WIDE_HIP_TRY(hipEventCreateWithFlags(&sp.done, hipEventDisableTiming));
    if (sp.host_bytes < up_bytes) {
        if (sp.host) (void)hipHostFree(sp.host);
        sp.host = nullptr;
        sp.host_bytes = 0;
        WIDE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sp.host), up_bytes, 0));
        sp.host_bytes = up_bytes;
    }
    memcpy(sp.host, c.sm, kMatrixBytes);
    memcpy(sp.host + kMatrixBytes, p.tiles.data(), n * sizeof(TileWork));
    unsigned char *up = sp.dev + code_bytes;
    WIDE_HIP_TRY(hipMemcpyAsync(up, sp.host, up_bytes, hipMemcpyHostToDevice, st));
    WIDE_HIP_TRY(hipEventRecord(sp.done, st));
    const int8_t *d_sm = reinterpret_cast<const int8_t *>(up);
    const TileWork *work = reinterpret_cast<const TileWork *>(up + kMatrixBytes);
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s];
        WIDE_HIP_TRY(launch_slice(p, s, c, s1 + off1[a], s2 + off2[a], work + a, d_sm, static_cast<int32_t *>(d_scores) + a,
                                  static_cast<int32_t *>(d_ends) + 4 * a, tb ? reinterpret_cast<unsigned long long *>(sp.dev) : nullptr,
                                  tb ? static_cast<unsigned long long *>(d_moves) + p.move_offsets[a] : nullptr,
                                  tb ? static_cast<uint32_t *>(d_counts) + a : nullptr, sp.dev + codes_only, st));
    }
    return SWMI_OK;
}

int run_host(const Params &c, const char *entry, const uint8_t *seq1s, const uint64_t *off1, const uint8_t *seq2s, const uint64_t *off2,
             size_t n, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *counts)
{
    int rc = check_call(c, seq1s, off1, seq2s, off2, n, scores, ends, moves, counts);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    const bool tb = moves != nullptr;
    Plan p;
    rc = make_plan(p, off1, off2, n, tb);
    if (rc != SWMI_OK) return rc;
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    std::lock_guard<std::mutex> lock(ds->host_mu);
    HostSet *sets = ds->sets;
    const int n_sets = p.slices() > 1 ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if (!s.stream) WIDE_HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        rc = grow(s.d1, s.have.d1, std::max<size_t>(p.max_seq1, 16));
        if (rc == SWMI_OK) rc = grow(s.d2, s.have.d2, std::max<size_t>(p.max_seq2, 16));
        if (rc == SWMI_OK) rc = grow(s.d_sm, s.have.sm, kMatrixBytes);
        if (rc == SWMI_OK) rc = grow(s.d_scores, s.have.scores, p.max_m);
        if (rc == SWMI_OK) rc = grow(s.d_ends, s.have.ends, p.max_m * 4);
        if (rc == SWMI_OK) rc = grow(s.d_counts, s.have.counts, p.max_m);
        if (rc == SWMI_OK) rc = grow(s.d_work, s.have.work, p.max_m);
        if (rc == SWMI_OK && tb) rc = grow(s.d_codes, s.have.codes, std::max<size_t>(p.max_codes, 2));
        if (rc == SWMI_OK && tb) rc = grow(s.d_moves, s.have.moves, std::max<size_t>(p.max_moves, 2));
        if (rc == SWMI_OK && p.max_carry) rc = grow(s.d_carry, s.have.carry, p.max_carry);
        if (rc != SWMI_OK) return rc;
    }
    // results of the slice a set holds -> host, at the caller's positions
    auto drain = [&](int which) -> hipError_t {
        HostSet &s = sets[which];
        if (s.m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(scores + s.off, s.d_scores, s.m * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess) r = hipMemcpyAsync(ends + 4 * s.off, s.d_ends, s.m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(counts + s.off, s.d_counts, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess && tb) {
            const size_t w0 = size_t(p.move_offsets[s.off]), words = size_t(p.move_offsets[s.off + s.m]) - w0;
            if (words) r = hipMemcpyAsync(moves + w0, s.d_moves, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
        }
        if (r == hipSuccess) r = hipStreamSynchronize(s.stream);
        s.m = 0;
        return r;
    };
    hipError_t e = hipSuccess;
    int turn = 0;
    for (size_t sc = 0; e == hipSuccess && sc < p.slices(); ++sc, turn ^= 1) {
        const int which = n_sets == 2 ? turn : 0;
        HostSet &s = sets[which];
        e = drain(which);                                   // (two slices ago; normally already empty)
        if (e != hipSuccess) break;
        const size_t a = p.first[sc], b = p.first[sc + 1];
        s.off = a;
        s.m = b - a;
        const size_t seq1_bytes = size_t(off1[b] - off1[a]), seq2_bytes = size_t(off2[b] - off2[a]);
        if (sc < size_t(n_sets)) e = hipMemcpyAsync(s.d_sm, c.sm, kMatrixBytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && seq1_bytes) e = hipMemcpyAsync(s.d1, seq1s + off1[a], seq1_bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && seq2_bytes) e = hipMemcpyAsync(s.d2, seq2s + off2[a], seq2_bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_work, p.tiles.data() + a, s.m * sizeof(TileWork), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = launch_slice(p, sc, c, s.d1, s.d2, s.d_work, s.d_sm, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr,
                             tb ? s.d_moves : nullptr, tb ? s.d_counts : nullptr, s.d_carry, s.stream);
        if (e == hipSuccess && n_sets == 2) e = drain(turn ^ 1);         // the previous slice, while this one computes
    }
    for (int k = 0; k < n_sets; ++k) {
        if (e == hipSuccess) e = drain(k);
        if (e != hipSuccess && sets[k].stream) (void)hipStreamSynchronize(sets[k].stream);
        sets[k].m = 0;
    }
    if (e != hipSuccess) return fail(SWMI_ERR_HIP, "%s: %s", entry, hipGetErrorString(e));
    return SWMI_OK;
}

}  // namespace
}  // namespace wide
}  // namespace swmi

using namespace swmi;
using namespace swmi::wide;

extern "C" {

const char *WIDE_ENTRY(last_error)(void) { return t_error; }

int WIDE_ENTRY(version)(void) { return SWMI_VERSION; }

int WIDE_ENTRY(release_workspaces)(void)
{
    DeviceState *ds = nullptr;
    const int rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    WIDE_HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> host_lock(ds->host_mu);
    std::lock_guard<std::mutex> lock(ds->ws_mu);
    ds->release();
    return SWMI_OK;
}

size_t WIDE_ENTRY(slices_for)(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int traceback, size_t *sizes, size_t cap)
{
    if (check_both(seq1_offsets, seq2_offsets, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(seq1_offsets, seq2_offsets, n, traceback != 0);
    for (size_t s = 0; sizes && s + 1 < first.size() && s < cap; ++s) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

int WIDE_ENTRY(local)(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets, size_t n,
                      const int8_t score_matrix[1024], int gap_open, int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves,
                      uint32_t *steps)
{
    return run_host({kWideLocal, score_matrix, gap_open, gap_extend, 0}, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, scores,
                    ends, moves, steps);
}

int WIDE_ENTRY(global)(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets, size_t n,
                       const int8_t score_matrix[1024], int gap_open, int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                       uint64_t *moves, uint32_t *steps)
{
    return run_host({kWideGlobal, score_matrix, gap_open, gap_extend, free_ends}, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n,
                    scores, ends, moves, steps);
}

int WIDE_ENTRY(local_device)(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                             size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                             void *d_moves, void *d_steps, void *stream)
{
    return run_device({kWideLocal, score_matrix, gap_open, gap_extend, 0}, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, d_scores,
                      d_ends, d_moves, d_steps, stream);
}

int WIDE_ENTRY(global_device)(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                              size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, unsigned free_ends,
                              void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return run_device({kWideGlobal, score_matrix, gap_open, gap_extend, free_ends}, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                      d_scores, d_ends, d_moves, d_steps, stream);
}

// one untimed device call first (it grows the workspace, which synchronises the stream), then HIP events around `iters`
int WIDE_ENTRY(time_device)(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                            size_t n, const int8_t score_matrix[1024], int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                            void *d_ends, void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    if (kind != SWMI_WIDE_LOCAL && kind != SWMI_WIDE_GLOBAL) return fail(SWMI_ERR_INVALID_ARGUMENT, "kind %d is neither local nor global", kind);
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    const Params c{kind == SWMI_WIDE_LOCAL ? kWideLocal : kWideGlobal, score_matrix, gap_open, gap_extend,
                   kind == SWMI_WIDE_LOCAL ? 0u : free_ends};
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_device(c, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, d_scores, d_ends, d_moves, d_steps, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = run_device(c, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, d_scores, d_ends, d_moves, d_steps, stream);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventRecord(ev[1], st);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventSynchronize(ev[1]);
    float ms = 0.f;
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (auto &x : ev)
        if (x) (void)hipEventDestroy(x);
    if (he != hipSuccess) return fail(SWMI_ERR_HIP, "%s: %s", __func__, hipGetErrorString(he));
    if (rc == SWMI_OK) *avg_ms = ms / iters;
    return rc;
}

}  // extern "C"
