// banded_ragged_api.cpp -- the C entries of libswmi_banded_ragged.so (include/swmi_banded_ragged.h): the
// banded local and the banded global / fit / overlap / extension aligner on a batch of mixed (len1, len2) with a diagonal per
// alignment; and, compiled a second time with -DSWMI_BANDED_WIDTH_LIBRARY, of libswmi_banded_width.so
// (include/swmi_banded_width.h, section 38): the same with ONE BAND WIDTH PER CALL, 128 .. 1024; and a third time with
// -DSWMI_BANDED_LONG_LIBRARY, of libswmi_banded_long.so (include/swmi_banded_long.h, section 41): the width library's entries
// for lengths up to 65536.  Everything in which the libraries differ stands in the one block below the error text (section
// 39); nothing after it tests a define.  Its
// structure is banded_api.cpp's: no Context of libswmi.so, no swmi_init -- every entry runs on the calling thread's current
// HIP device, with this file's own workspaces per (device, stream), its own two streams and buffer sets per device for the
// host entries, and its own thread-local error text.  Of libswmi.so, linked for the callers' move_offsets and expander, it
// calls nothing.  Both kinds are in this one object: the kind is a field of Call, and so is the band, which is kBandWidth
// throughout in the ragged library.  This file's name lies outside csrc/swmi_*.cpp, which four host-only test programs glob.
//
// THE PLAN.  A checked batch is cut into slices (contiguous in caller order, the header's arithmetic), and each slice's
// alignments become slots in the order the kernels take them: by swept rows at the call's width (width_swept_rows,
// banded_internal.h) descending, ties in caller order, so that the four wavefronts of a workgroup carry similar work and the
// longest alignments start first.  Every offset of a slot is relative to its slice; code offsets are a running sum in plan
// order, an alignment's codes taking band / 128 times the bytes they take at 128.
#include "banded_internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

namespace swmi {
namespace banded {
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

}  // namespace
}  // namespace banded
}  // namespace swmi

// ---- what the libraries differ in: the public header, the prefix of the exported names, the spelling of the two kinds in an
// ---- error text, whether a call carries a band (and with it the BAND parameter of seven entries and the launcher), the
// ---- longest sequence, the clamp of a diagonal and the macro of an alignment's move words, a test-only switch of the ragged
// ---- library's, and the long library's tenth export ----
#ifdef SWMI_BANDED_LONG_LIBRARY
#include "../../include/swmi_banded_long.h"
#define BANDED_ENTRY(name) swmi_banded_long_##name
#define BANDED_BAND_PARAM int band,
#define BANDED_BAND_ARG band
#define BANDED_MOVE_WORDS(len1, len2) SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2)
#define BANDED_LAUNCH_WIDTH launch_banded_long

namespace swmi {
namespace banded {
namespace {
constexpr bool kHasBand = true;
constexpr int kMaxLen = kBandLongMaxLen, kDiagClamp = kLongDiagClamp;
constexpr const char *kLocalName = "SWMI_BANDED_LONG_LOCAL", *kGlobalName = "SWMI_BANDED_LONG_GLOBAL";
static_assert(kMaxLen == SWMI_BANDED_LONG_MAX_LEN && sizeof(RaggedSlot) == SWMI_BANDED_LONG_SLOT_BYTES);
static_assert(kRaggedLocal == SWMI_BANDED_LONG_LOCAL && kRaggedGlobal == SWMI_BANDED_LONG_GLOBAL);
static_assert(width_is_legal(SWMI_BANDED_LONG_MIN) && width_is_legal(SWMI_BANDED_LONG_MAX) && kBandWidth == SWMI_BANDED_LONG_MIN);
// every band beyond the clamp misses every table, and the launcher's arithmetic on a clamped diagonal stays in int32
static_assert(kDiagClamp > kMaxLen + SWMI_BANDED_LONG_MAX / 2 && kDiagClamp + 2 * kMaxLen < (1 << 30));
// one move layout with the 16384 libraries: the two macros of swmi.h are the same expression
static_assert(SWMI_LOCAL_LONG_MOVE_WORDS(0, 0) == SWMI_LOCAL_FULL_MOVE_WORDS(0, 0) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(31, 2) == SWMI_LOCAL_FULL_MOVE_WORDS(31, 2) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(300, 1025) == SWMI_LOCAL_FULL_MOVE_WORDS(300, 1025) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(16384, 16384) == SWMI_LOCAL_FULL_MOVE_WORDS(16384, 16384) &&
              SWMI_LOCAL_LONG_MOVE_WORDS(65536, 65536) == 4096);
constexpr bool sort_enabled() { return true; }
int check_offsets(const uint64_t *off1, const uint64_t *off2, size_t n);
}  // namespace
}  // namespace banded
}  // namespace swmi

// move_offsets[0 .. n]: the running sum of SWMI_LOCAL_LONG_MOVE_WORDS over offsets that the aligning entries accept
extern "C" int swmi_banded_long_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, uint64_t *move_offsets)
{
    using namespace swmi::banded;
    if (!move_offsets) return fail(SWMI_ERR_INVALID_ARGUMENT, "move_offsets is NULL");
    const int rc = check_offsets(seq1_offsets, seq2_offsets, n);
    if (rc != SWMI_OK) return rc;
    move_offsets[0] = 0;
    for (size_t k = 0; k < n; ++k)
        move_offsets[k + 1] = move_offsets[k] + BANDED_MOVE_WORDS(seq1_offsets[k + 1] - seq1_offsets[k], seq2_offsets[k + 1] - seq2_offsets[k]);
    return SWMI_OK;
}

namespace swmi {
namespace banded {
namespace {
#elif defined(SWMI_BANDED_WIDTH_LIBRARY)
#include "../../include/swmi_banded_width.h"
#define BANDED_ENTRY(name) swmi_banded_width_##name
#define BANDED_BAND_PARAM int band,
#define BANDED_BAND_ARG band
#define BANDED_MOVE_WORDS(len1, len2) SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2)
#define BANDED_LAUNCH_WIDTH launch_banded_width

namespace swmi {
namespace banded {
namespace {
constexpr bool kHasBand = true;
constexpr int kMaxLen = kBandMaxLen, kDiagClamp = kRaggedDiagClamp;
constexpr const char *kLocalName = "SWMI_BANDED_WIDTH_LOCAL", *kGlobalName = "SWMI_BANDED_WIDTH_GLOBAL";
static_assert(kBandMaxLen == SWMI_BANDED_WIDTH_MAX_LEN && sizeof(RaggedSlot) == SWMI_BANDED_WIDTH_SLOT_BYTES);
static_assert(kRaggedLocal == SWMI_BANDED_WIDTH_LOCAL && kRaggedGlobal == SWMI_BANDED_WIDTH_GLOBAL);
static_assert(width_is_legal(SWMI_BANDED_WIDTH_MIN) && width_is_legal(SWMI_BANDED_WIDTH_MAX) && kBandWidth == SWMI_BANDED_WIDTH_MIN);
constexpr bool sort_enabled() { return true; }
#else
#include "../../include/swmi_banded_ragged.h"
#define BANDED_ENTRY(name) swmi_banded_ragged_##name
#define BANDED_BAND_PARAM
#define BANDED_BAND_ARG kBandWidth
#define BANDED_MOVE_WORDS(len1, len2) SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2)
#define BANDED_LAUNCH_WIDTH launch_banded_width      // (named in a discarded statement only)

namespace swmi {
namespace banded {
namespace {
constexpr bool kHasBand = false;
constexpr int kMaxLen = kBandMaxLen, kDiagClamp = kRaggedDiagClamp;
constexpr const char *kLocalName = "SWMI_BANDED_RAGGED_LOCAL", *kGlobalName = "SWMI_BANDED_RAGGED_GLOBAL";
static_assert(kBandMaxLen == SWMI_BANDED_RAGGED_MAX_LEN && sizeof(RaggedSlot) == SWMI_BANDED_RAGGED_SLOT_BYTES);
static_assert(kRaggedLocal == SWMI_BANDED_RAGGED_LOCAL && kRaggedGlobal == SWMI_BANDED_RAGGED_GLOBAL);
// test-only: SWMI_BANDED_RAGGED_NO_SORT=1 leaves the slots of a slice in caller order (read once)
bool sort_enabled()
{
    static const bool on = [] {
        const char *e = getenv("SWMI_BANDED_RAGGED_NO_SORT");
        return !(e && e[0] == '1');
    }();
    return on;
}
#endif
// ---- below this line the three builds are one text ----

// (no line number: the text is the same wherever the call stands, so that a line added here moves neither library's texts)
#define BANDED_HIP_TRY(expr)                                                                                        \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) return fail(SWMI_ERR_HIP, "%s failed: %s (%s)", #expr, hipGetErrorString(e_), __FILE__); \
    } while (0)

constexpr size_t kSliceBytes = size_t(256) << 20;        // an ends-only slice's device bytes
constexpr size_t kMaxSlice = size_t(1) << 20;            // alignments per slice (and per launch)
constexpr size_t kTbSliceBytes = 4383801344ull;          // a traceback slice's device bytes: banded_api.cpp's

struct Call {
    int kind, band;                             // (the band: kBandWidth in the ragged library)
    const uint64_t *off1, *off2;
    size_t n;
    const int32_t *diagonals;                   // host memory, or NULL
    const int8_t *sm;
    int gap_open, gap_extend;
    unsigned free_ends;
    size_t len1(size_t k) const { return size_t(off1[k + 1] - off1[k]); }
    size_t len2(size_t k) const { return size_t(off2[k + 1] - off2[k]); }
};

// device bytes one alignment of a slice takes: its sequences, its slot, its results, and with a traceback codes, moves, count
size_t alignment_bytes(int kind, int band, size_t len1, size_t len2, bool tb)
{
    size_t b = len1 + len2 + sizeof(RaggedSlot) + 5 * sizeof(int32_t);
    if (tb) b += width_code_bytes(kind, len1, band) + BANDED_MOVE_WORDS(len1, len2) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

int check_kind(int kind)
{
    if (kind != kRaggedLocal && kind != kRaggedGlobal)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "kind %d is neither %s nor %s", kind, kLocalName, kGlobalName);
    return SWMI_OK;
}

int check_band(int band)
{
    if (kHasBand && !width_is_legal(band)) return fail(SWMI_ERR_INVALID_ARGUMENT, "band %d is not one of 128, 256, 512, 1024", band);
    return SWMI_OK;
}

int check_offsets(const uint64_t *off1, const uint64_t *off2, size_t n)
{
    if (!off1 || !off2) return fail(SWMI_ERR_INVALID_ARGUMENT, "seq1_offsets or seq2_offsets is NULL");
    for (size_t k = 0; k < n; ++k) {
        if (off1[k + 1] < off1[k] || off2[k + 1] < off2[k]) return fail(SWMI_ERR_INVALID_ARGUMENT, "offsets decrease at alignment %zu", k);
        if (off1[k + 1] - off1[k] > uint64_t(kMaxLen) || off2[k + 1] - off2[k] > uint64_t(kMaxLen))
            return fail(SWMI_ERR_INVALID_ARGUMENT, "alignment %zu: a length above %d", k, kMaxLen);
    }
    return SWMI_OK;
}

// The checks in the header's order: the band where the call has one; the mask, the matrix, the gaps, the moves / steps pair;
// then n = 0, the buffers, the offsets.  1 = nothing to do.
int check_call(const Call &c, const void *seq1s, const void *seq2s, const void *scores, const void *ends, const void *moves,
               const void *steps)
{
    if (check_band(c.band) != SWMI_OK) return SWMI_ERR_INVALID_ARGUMENT;
    if (c.kind == kRaggedGlobal && c.free_ends > SWMI_BANDED_MAX_FREE_ENDS)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u is not a mask of SWMI_FREE_* (0..15) or SWMI_BANDED_END_ANYWHERE with SWMI_FREE_BEGIN* (16..19)", c.free_ends);
    if (!c.sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (c.gap_open < 0 || c.gap_open > 127 || c.gap_extend < 0 || c.gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", c.gap_open, c.gap_extend);
    if (!moves != !steps)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (c.n == 0) return 1;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", c.n);
    return check_offsets(c.off1, c.off2, c.n);
}

// slices of checked offsets: first = {0, ..., n}
std::vector<size_t> cut(int kind, int band, const uint64_t *off1, const uint64_t *off2, size_t n, bool tb)
{
    const size_t cap = tb ? kTbSliceBytes : kSliceBytes;
    std::vector<size_t> first{0};
    size_t bytes = 0, m = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t b = alignment_bytes(kind, band, size_t(off1[k + 1] - off1[k]), size_t(off2[k + 1] - off2[k]), tb);
        if (m && (bytes + b > cap || m == kMaxSlice)) {
            first.push_back(k);
            bytes = 0;
            m = 0;
        }
        bytes += b;
        ++m;
    }
    if (n) first.push_back(n);
    return first;
}

// A call's plan.  It lives in thread-local storage, so that a device call of some ten thousand alignments -- a few
// milliseconds of kernel -- does not pay for fresh pages of scratch arrays each time; a plan that grew past kKeepPlan alignments
// gives its arrays back when the call ends.
constexpr size_t kKeepPlan = size_t(1) << 18;
struct Plan {
    std::vector<uint64_t> move_offsets;         // n + 1 (all 0 ends-only)
    std::vector<size_t> first;                  // slice s = alignments [first[s], first[s + 1])
    RaggedSlot *slots = nullptr;                // [n], the caller's memory: slice s's slots at [first[s], first[s + 1]), slice-relative
    std::vector<uint32_t> order;                // scratch of one slice
    std::vector<int32_t> rows, diag;
    size_t max_m = 0, max_seq1 = 0, max_seq2 = 0, max_codes = 0, max_moves = 0;      // the largest slice's (codes: bytes; moves: words)
    size_t slices() const { return first.size() - 1; }
};
thread_local Plan t_plan;

struct PlanUse {                                 // the calling thread's plan for the length of one call
    Plan &p = t_plan;
    ~PlanUse()
    {
        if (p.move_offsets.capacity() > kKeepPlan) p = Plan{};
    }
};

// the slots go to `slots` (n of them): pinned memory of a device call, a vector of a host call
void make_plan(Plan &p, const Call &c, bool tb, RaggedSlot *slots)
{
    const size_t n = c.n;
    p.slots = slots;
    p.max_m = p.max_seq1 = p.max_seq2 = p.max_codes = p.max_moves = 0;
    p.move_offsets.assign(n + 1, 0);
    if (tb)
        for (size_t k = 0; k < n; ++k) p.move_offsets[k + 1] = p.move_offsets[k] + BANDED_MOVE_WORDS(c.len1(k), c.len2(k));
    p.first = cut(c.kind, c.band, c.off1, c.off2, n, tb);
    std::vector<uint32_t> &order = p.order;
    std::vector<int32_t> &rows = p.rows, &diag = p.diag;
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s], b = p.first[s + 1], m = b - a;
        order.resize(m);
        rows.resize(m);
        diag.resize(m);
        bool sorted = true;
        for (size_t x = 0; x < m; ++x) {
            const int32_t d = c.diagonals ? c.diagonals[a + x] : 0;
            diag[x] = std::max(-kDiagClamp, std::min(kDiagClamp, d));
            rows[x] = width_swept_rows(c.kind, int(c.len1(a + x)), int(c.len2(a + x)), diag[x], c.band);
            order[x] = uint32_t(x);
            if (x && rows[x] > rows[x - 1]) sorted = false;
        }
        if (!sorted && sort_enabled())
            std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return rows[x] > rows[y]; });
        uint64_t codes = 0;                      // dwords
        for (size_t x = 0; x < m; ++x) {
            const size_t k = a + order[x];
            RaggedSlot &t = p.slots[a + x];
            t.off1 = c.off1[k] - c.off1[a];
            t.off2 = c.off2[k] - c.off2[a];
            t.code_off = codes;
            t.move_off = p.move_offsets[k] - p.move_offsets[a];
            t.len1 = int32_t(c.len1(k));
            t.len2 = int32_t(c.len2(k));
            t.d0 = diag[order[x]];
            t.index = order[x];
            if (tb) codes += width_code_bytes(c.kind, c.len1(k), c.band) / 4;
        }
        p.max_m = std::max(p.max_m, m);
        p.max_seq1 = std::max(p.max_seq1, size_t(c.off1[b] - c.off1[a]));
        p.max_seq2 = std::max(p.max_seq2, size_t(c.off2[b] - c.off2[a]));
        p.max_codes = std::max(p.max_codes, size_t(codes) * 4);
        p.max_moves = std::max(p.max_moves, size_t(p.move_offsets[b] - p.move_offsets[a]));
    }
}

// ---- device state: one per HIP device, made on first use ----
template <class T> int grow(T *&p, size_t &have, size_t need)
{
    if (have >= need) return SWMI_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    have = 0;
    BANDED_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), need * sizeof(T)));
    have = need;
    return SWMI_OK;
}

struct HostSet {
    hipStream_t stream = nullptr;
    uint8_t *d1 = nullptr, *d2 = nullptr;
    RaggedSlot *d_slots = nullptr;
    int32_t *d_scores = nullptr, *d_ends = nullptr;
    unsigned char *d_codes = nullptr;
    unsigned long long *d_moves = nullptr;
    uint32_t *d_steps = nullptr;
    struct { size_t d1, d2, slots, scores, ends, codes, moves, steps; } have{};
    size_t off = 0, m = 0;                          // slice in flight
    void release()
    {
        for (void *q : {(void *)d1, (void *)d2, (void *)d_slots, (void *)d_scores, (void *)d_ends, (void *)d_codes, (void *)d_moves,
                        (void *)d_steps})
            if (q) (void)hipFree(q);
        if (stream) (void)hipStreamDestroy(stream);      // (made again by the next host call)
        *this = HostSet{};
    }
};

// a stream's workspace of the device entries -- the codes of one slice and behind them the call's slots -- and the pinned copy
// of the slots that the upload reads; `done` is recorded behind the upload
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
        BANDED_HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(SWMI_ERR_UNSUPPORTED_ARCH, "device %d is %s, not gfx950", dev, prop.gcnArchName);
        it = g_devices.emplace(std::piecewise_construct, std::forward_as_tuple(dev), std::forward_as_tuple()).first;
    }
    *out = &it->second;
    return SWMI_OK;
}

// one slice's launch, by the launcher of the kernel object the library links
hipError_t launch(const Call &c, const uint8_t *d_seq1s, const uint8_t *d_seq2s, const RaggedSlot *d_slots, size_t m, int32_t *d_scores,
                  int32_t *d_ends, unsigned char *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream)
{
    if constexpr (kHasBand)
        return BANDED_LAUNCH_WIDTH(c.kind, c.band, d_seq1s, d_seq2s, d_slots, m, c.sm, c.gap_open, c.gap_extend, c.free_ends, d_scores, d_ends,
                                   d_codes, d_moves, d_steps, stream);
    else
        return launch_banded_ragged(c.kind, d_seq1s, d_seq2s, d_slots, m, c.sm, c.gap_open, c.gap_extend, c.free_ends, d_scores, d_ends, d_codes,
                                    d_moves, d_steps, stream);
}

int run_device(const Call &c, const void *d_seq1s, const void *d_seq2s, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
               void *stream)
{
    int rc = check_call(c, d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_steps)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    const bool tb = d_moves != nullptr;
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one workspace per (device, stream), looked up, grown and handed to the launches under one lock (growing waits for this
    // stream only: earlier launches on it may still use the old one)
    std::lock_guard<std::mutex> lock(ds->ws_mu);
    StreamSpace &sp = ds->spaces[st];
    const size_t up_bytes = c.n * sizeof(RaggedSlot);
    // the slots are planned straight into pinned memory, once the stream's last upload has finished reading it
    if (sp.done) BANDED_HIP_TRY(hipEventSynchronize(sp.done));
    else BANDED_HIP_TRY(hipEventCreateWithFlags(&sp.done, hipEventDisableTiming));
    if (sp.host_bytes < up_bytes) {
        if (sp.host) (void)hipHostFree(sp.host);
        sp.host = nullptr;
        sp.host_bytes = 0;
        BANDED_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sp.host), up_bytes, 0));
        sp.host_bytes = up_bytes;
    }
    PlanUse use;
    Plan &p = use.p;
    make_plan(p, c, tb, reinterpret_cast<RaggedSlot *>(sp.host));
    const size_t code_bytes = (p.max_codes + 15) & ~size_t(15);
    if (code_bytes + up_bytes > sp.dev_bytes) {
        BANDED_HIP_TRY(hipStreamSynchronize(st));
        if (sp.dev) (void)hipFree(sp.dev);
        sp.dev = nullptr;
        sp.dev_bytes = 0;
        BANDED_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sp.dev), code_bytes + up_bytes));
        sp.dev_bytes = code_bytes + up_bytes;
    }
    // (behind whatever codes this call's slices need: an earlier call's launches on this stream read their slots in stream
    // order before this upload overwrites them)
    unsigned char *up = sp.dev + sp.dev_bytes - up_bytes;
    BANDED_HIP_TRY(hipMemcpyAsync(up, sp.host, up_bytes, hipMemcpyHostToDevice, st));
    BANDED_HIP_TRY(hipEventRecord(sp.done, st));
    const RaggedSlot *slots = reinterpret_cast<const RaggedSlot *>(up);
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s], m = p.first[s + 1] - a;
        BANDED_HIP_TRY(launch(c, s1 + c.off1[a], s2 + c.off2[a], slots + a, m, static_cast<int32_t *>(d_scores) + a,
                              static_cast<int32_t *>(d_ends) + 4 * a, tb ? sp.dev : nullptr,
                              tb ? static_cast<unsigned long long *>(d_moves) + p.move_offsets[a] : nullptr,
                              tb ? static_cast<uint32_t *>(d_steps) + a : nullptr, st));
    }
    return SWMI_OK;
}

int run_host(const Call &c, const char *entry, const uint8_t *seq1s, const uint8_t *seq2s, int32_t *scores, int32_t *ends, uint64_t *moves,
             uint32_t *steps)
{
    int rc = check_call(c, seq1s, seq2s, scores, ends, moves, steps);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    const bool tb = moves != nullptr;
    PlanUse use;
    Plan &p = use.p;
    std::vector<RaggedSlot> slots(c.n);
    make_plan(p, c, tb, slots.data());
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    std::lock_guard<std::mutex> lock(ds->host_mu);
    HostSet *sets = ds->sets;
    const int n_sets = p.slices() > 1 ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if (!s.stream) BANDED_HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        rc = grow(s.d1, s.have.d1, std::max<size_t>(p.max_seq1, 16));
        if (rc == SWMI_OK) rc = grow(s.d2, s.have.d2, std::max<size_t>(p.max_seq2, 16));
        if (rc == SWMI_OK) rc = grow(s.d_slots, s.have.slots, p.max_m);
        if (rc == SWMI_OK) rc = grow(s.d_scores, s.have.scores, std::max<size_t>(p.max_m, 4));
        if (rc == SWMI_OK) rc = grow(s.d_ends, s.have.ends, p.max_m * 4);
        if (rc == SWMI_OK && tb) rc = grow(s.d_steps, s.have.steps, std::max<size_t>(p.max_m, 4));
        if (rc == SWMI_OK && tb) rc = grow(s.d_codes, s.have.codes, std::max<size_t>(p.max_codes, 16));
        if (rc == SWMI_OK && tb) rc = grow(s.d_moves, s.have.moves, std::max<size_t>(p.max_moves, 2));
        if (rc != SWMI_OK) return rc;
    }
    // results of the slice a set holds -> host, at the caller's positions
    auto drain = [&](int which) -> hipError_t {
        HostSet &s = sets[which];
        if (s.m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(scores + s.off, s.d_scores, s.m * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess) r = hipMemcpyAsync(ends + 4 * s.off, s.d_ends, s.m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(steps + s.off, s.d_steps, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream);
        const size_t w0 = size_t(p.move_offsets[s.off]), words = size_t(p.move_offsets[s.off + s.m]) - w0;
        if (r == hipSuccess && tb && words) r = hipMemcpyAsync(moves + w0, s.d_moves, words * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
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
        s.off = p.first[sc];
        s.m = p.first[sc + 1] - s.off;
        const size_t b1 = size_t(c.off1[s.off + s.m] - c.off1[s.off]), b2 = size_t(c.off2[s.off + s.m] - c.off2[s.off]);
        if (b1) e = hipMemcpyAsync(s.d1, seq1s + c.off1[s.off], b1, hipMemcpyHostToDevice, s.stream);      // (no byte of an empty side)
        if (e == hipSuccess && b2) e = hipMemcpyAsync(s.d2, seq2s + c.off2[s.off], b2, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_slots, p.slots + s.off, s.m * sizeof(RaggedSlot), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = launch(c, s.d1, s.d2, s.d_slots, s.m, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr, tb ? s.d_moves : nullptr,
                       tb ? s.d_steps : nullptr, s.stream);
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
}  // namespace banded
}  // namespace swmi

using namespace swmi;
using namespace swmi::banded;

extern "C" {

const char *BANDED_ENTRY(last_error)(void) { return t_error; }

int BANDED_ENTRY(version)(void) { return SWMI_VERSION; }

int BANDED_ENTRY(release_workspaces)(void)
{
    DeviceState *ds = nullptr;
    const int rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    BANDED_HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> host_lock(ds->host_mu);
    std::lock_guard<std::mutex> lock(ds->ws_mu);
    ds->release();
    return SWMI_OK;
}

size_t BANDED_ENTRY(slices_for)(int kind, BANDED_BAND_PARAM const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int traceback,
                                size_t *sizes, size_t cap)
{
    if (check_kind(kind) != SWMI_OK || check_band(BANDED_BAND_ARG) != SWMI_OK) return 0;      // (here the kind first)
    if (n == 0 || check_offsets(seq1_offsets, seq2_offsets, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(kind, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, traceback != 0);
    for (size_t s = 0; s + 1 < first.size(); ++s)
        if (sizes && s < cap) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

int BANDED_ENTRY(local)(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets, size_t n,
                        const int32_t *diagonals, BANDED_BAND_PARAM const int8_t score_matrix[16], int gap_open, int gap_extend,
                        int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return run_host(Call{kRaggedLocal, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, diagonals, score_matrix, gap_open, gap_extend, 0u},
                    __func__, seq1s, seq2s, scores, ends, moves, steps);
}

int BANDED_ENTRY(global)(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets, size_t n,
                         const int32_t *diagonals, BANDED_BAND_PARAM const int8_t score_matrix[16], int gap_open, int gap_extend,
                         unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return run_host(Call{kRaggedGlobal, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, diagonals, score_matrix, gap_open, gap_extend, free_ends},
                    __func__, seq1s, seq2s, scores, ends, moves, steps);
}

int BANDED_ENTRY(local_device)(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets, size_t n,
                               const int32_t *diagonals, BANDED_BAND_PARAM const int8_t score_matrix[16], int gap_open, int gap_extend,
                               void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return run_device(Call{kRaggedLocal, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, diagonals, score_matrix, gap_open, gap_extend, 0u},
                      d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps, stream);
}

int BANDED_ENTRY(global_device)(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets, size_t n,
                                const int32_t *diagonals, BANDED_BAND_PARAM const int8_t score_matrix[16], int gap_open, int gap_extend,
                                unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return run_device(Call{kRaggedGlobal, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, diagonals, score_matrix, gap_open, gap_extend, free_ends},
                      d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps, stream);
}

// one untimed device call first (it grows the workspace, which synchronises the stream), then HIP events around `iters`
int BANDED_ENTRY(time_device)(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                              size_t n, const int32_t *diagonals, BANDED_BAND_PARAM const int8_t score_matrix[16], int gap_open, int gap_extend,
                              unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                              float *avg_ms)
{
    if (check_band(BANDED_BAND_ARG) != SWMI_OK || check_kind(kind) != SWMI_OK) return SWMI_ERR_INVALID_ARGUMENT;     // the band first
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    const Call c{kind, BANDED_BAND_ARG, seq1_offsets, seq2_offsets, n, diagonals, score_matrix, gap_open, gap_extend,
                 kind == kRaggedGlobal ? free_ends : 0u};
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_device(c, d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps, stream);
    if (rc != SWMI_OK) return rc;
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");       // (behind the call's own checks, which keep their order)
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = run_device(c, d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps, stream);
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
