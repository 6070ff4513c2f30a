// wide_api.cpp -- the C entries of libswmi_wide.so (include/swmi_wide.h) and, compiled a second time
// with -DSWMI_WIDE_LONG_LIBRARY, of libswmi_wide_long.so (include/swmi_wide_long.h, section 30): the wide-alphabet local and
// global aligners on a batch of mixed (len1, len2).  Everything in which the two libraries differ stands in the one block
// below the error text (section 31); nothing after it tests the define but the one definition of check_seq2.  Compiled a third
// time with -DSWMI_WIDE_PROFILE_LIBRARY it is the host code of libswmi_wide_profile.so (include/swmi_wide_profile.h, section
// 32), whose calls have one length and no buffer on the seq2 side and a position-specific profile for a matrix.
// Self-contained: no Context of libswmi.so, no swmi_init -- every entry runs on the calling thread's current HIP device, with
// this file's own workspaces per (device, stream), its own two streams and buffer sets per device for the host entries, and its own thread-local error text.  Of libswmi.so, linked for the callers' expander, it calls nothing:
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

struct Seq2;                                             // the seq2 side of a call (below)
int check_both(const uint64_t *off1, Seq2 q, size_t n);
void fill_move_offsets(const uint64_t *off1, Seq2 q, size_t n, uint64_t *out);

}  // namespace
}  // namespace wide
}  // namespace swmi

// ---- what the libraries differ in: the public header, the prefix of the exported names, the limits on len1 and len2,
// ---- the traceback budget, whether there is a striped class of slots with its width rule and its two entries, and what the
// ---- seq2 side and the matrix of a call are (Seq2 and the WIDE_* parameter lists: libswmi_wide_profile.so, section 32) ----
#ifdef SWMI_WIDE_PROFILE_LIBRARY
#include "../../include/swmi_wide_profile.h"
#include "wide_profile_internal.h"
#define WIDE_ENTRY(name) swmi_wide_profile_##name

namespace swmi {
namespace wide {
namespace {
constexpr size_t kMaxLen1 = SWMI_WIDE_PROFILE_MAX_LEN1, kMaxLen2 = SWMI_WIDE_PROFILE_MAX_LEN2;
constexpr size_t kTbSliceAlignments = 256;               // libswmi_wide.so's budgets
constexpr bool kHasStriped = false;
constexpr int stripe_width(size_t) { return 0; }         // (named in a discarded statement only)
static_assert(SWMI_WIDE_PROFILE_LOCAL == SWMI_WIDE_LOCAL && SWMI_WIDE_PROFILE_GLOBAL == SWMI_WIDE_GLOBAL &&
              SWMI_WIDE_PROFILE_MAX_LEN1 == kWideMaxLen1 && SWMI_WIDE_PROFILE_MAX_LEN2 == kWideMaxLen2);

// The seq2 side of a call: one length for every alignment and no buffer.  The "matrix" of a call is the profile, int8[32 len2]
// position-major in the caller's memory (NULL iff len2 = 0) and lane-ready in the workspace and the pinned upload
// (wide_profile_internal.h): the host transposes it once per call.
struct Seq2 {
    size_t len2;
};
inline size_t seq2_len(Seq2 q, size_t) { return q.len2; }
inline uint64_t seq2_at(Seq2, size_t) { return 0; }      // TileWork::s2_off: 0 and unread
constexpr bool kSeq2PerSlot = false;                     // a slot's device bytes hold no seq2; the matrix block counts once per slice
inline int check_seq2(Seq2 q, size_t)
{
    if (q.len2 > kMaxLen2) return fail(SWMI_ERR_INVALID_ARGUMENT, "len2 %zu > %zu", q.len2, kMaxLen2);
    return SWMI_OK;
}
inline bool matrix_missing(const int8_t *profile, Seq2 q) { return !profile && q.len2 != 0; }
constexpr const char *kMatrixMissing = "profile is NULL with len2 > 0";
constexpr bool kMatrixAsGiven = false;                   // the kernels read another layout than the caller's
inline size_t matrix_bytes(Seq2 q) { return wide_profile_device_bytes(q.len2); }
void fill_matrix(unsigned char *dst, const int8_t *profile, Seq2 q)
{
    const size_t row = size_t(64) * wide_profile_waves_of(q.len2) * kWideProfileEntryBytes, whole = q.len2 & ~size_t(15);
    memset(dst, 0x80, 32 * row);
    // 16 columns x 32 letters at a time: 512 contiguous bytes in, one 16-byte entry of each letter row out
    for (size_t j = 0; j < whole; j += 16)
        for (size_t a = 0; a < 32; ++a)
            for (size_t jj = 0; jj < 16; ++jj) dst[a * row + j + jj] = (unsigned char)profile[(j + jj) * 32 + a];
    for (size_t j = whole; j < q.len2; ++j)
        for (size_t a = 0; a < 32; ++a) dst[a * row + j] = (unsigned char)profile[j * 32 + a];
}
// a buffer that stands where the other builds' seq2s stands: never NULL, 16-byte aligned, never read
alignas(16) const uint8_t kNoSeq2[16] = {};
inline size_t code_qwords_unstriped(int len1, int len2) { return wide_profile_code_qwords(len1, len2); }
inline int waves_unstriped(int len1, int len2) { return wide_profile_ragged_waves(len1, len2); }
inline hipError_t launch_unstriped(WideKind kind, const uint8_t *s1, const uint8_t *, const TileWork *work, size_t n, int waves, Seq2 q,
                                   const int8_t *d_sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                   unsigned long long *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    return launch_wide_profile_ragged(kind, s1, work, n, waves, d_sm, wide_profile_waves_of(q.len2), open, extend, free_ends, scores, ends,
                                      codes, moves, steps, st);
}
}  // namespace
}  // namespace wide
}  // namespace swmi

#define WIDE_SEQ2_HOST_PARAMS
#define WIDE_SEQ2_DEVICE_PARAMS
#define WIDE_OFF2_PARAM
#define WIDE_LEN2_PARAM size_t len2,
#define WIDE_MATRIX_PARAMS const int8_t *profile, size_t len2
#define WIDE_SEQ2_HOST_ARG swmi::wide::kNoSeq2
#define WIDE_SEQ2_DEVICE_ARG swmi::wide::kNoSeq2
#define WIDE_SEQ2_ARG swmi::wide::Seq2{len2}
#define WIDE_MATRIX_ARG profile

extern "C" int swmi_wide_profile_from_sequence(const uint8_t *query, size_t len2, const int8_t score_matrix[1024], int8_t *profile_out)
{
    using namespace swmi;
    if (len2 > wide::kMaxLen2) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "len2 %zu > %zu", len2, wide::kMaxLen2);
    if (!score_matrix) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (len2 && (!query || !profile_out)) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with len2 = %zu", len2);
    for (size_t j = 0; j < len2; ++j)
        for (int a = 0; a < 32; ++a) profile_out[j * 32 + a] = score_matrix[a * 32 + (query[j] & 31)];
    return SWMI_OK;
}

extern "C" int swmi_wide_profile_move_offsets(const uint64_t *seq1_offsets, size_t n, size_t len2, uint64_t *move_offsets)
{
    using namespace swmi;
    if (!move_offsets) return wide::fail(SWMI_ERR_INVALID_ARGUMENT, "move_offsets is NULL");
    const int rc = wide::check_both(seq1_offsets, wide::Seq2{len2}, n);
    if (rc != SWMI_OK) return rc;
    wide::fill_move_offsets(seq1_offsets, wide::Seq2{len2}, n, move_offsets);
    return SWMI_OK;
}
#else
// ---- the two libraries with a seq2 per alignment and a 32 x 32 matrix ----
namespace swmi {
namespace wide {
namespace {
struct Seq2 {                                            // the seq2 side of a call: its offsets
    const uint64_t *off;
};
inline size_t seq2_len(Seq2 q, size_t k) { return size_t(q.off[k + 1] - q.off[k]); }
inline uint64_t seq2_at(Seq2 q, size_t k) { return q.off[k]; }
constexpr bool kSeq2PerSlot = true;
int check_seq2(Seq2 q, size_t n);
inline bool matrix_missing(const int8_t *sm, Seq2) { return !sm; }
constexpr const char *kMatrixMissing = "score_matrix is NULL";
constexpr bool kMatrixAsGiven = true;                    // the kernels read the caller's 1024 bytes
constexpr size_t matrix_bytes(Seq2) { return 1024; }
inline void fill_matrix(unsigned char *dst, const int8_t *sm, Seq2) { memcpy(dst, sm, 1024); }
inline size_t code_qwords_unstriped(int len1, int len2) { return wide_affine_code_qwords(len1, len2); }
inline int waves_unstriped(int len1, int len2) { return wide_ragged_waves(len1, len2); }
inline hipError_t launch_unstriped(WideKind kind, const uint8_t *s1, const uint8_t *s2, const TileWork *work, size_t n, int waves, Seq2,
                                   const int8_t *d_sm, int open, int extend, unsigned free_ends, int32_t *scores, int32_t *ends,
                                   unsigned long long *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
    return launch_wide_affine_ragged(kind, s1, s2, work, n, waves, d_sm, open, extend, free_ends, scores, ends, codes, moves, steps, st);
}
}  // namespace
}  // namespace wide
}  // namespace swmi

#define WIDE_SEQ2_HOST_PARAMS const uint8_t *seq2s, const uint64_t *seq2_offsets,
#define WIDE_SEQ2_DEVICE_PARAMS const void *d_seq2s, const uint64_t *seq2_offsets,
#define WIDE_OFF2_PARAM const uint64_t *seq2_offsets,
#define WIDE_LEN2_PARAM
#define WIDE_MATRIX_PARAMS const int8_t score_matrix[1024]
#define WIDE_SEQ2_HOST_ARG seq2s
#define WIDE_SEQ2_DEVICE_ARG d_seq2s
#define WIDE_SEQ2_ARG swmi::wide::Seq2{seq2_offsets}
#define WIDE_MATRIX_ARG score_matrix
#endif

#if defined(SWMI_WIDE_PROFILE_LIBRARY)
// (its header, prefix, limits and two entries stand above, beside its Seq2)
#elif defined(SWMI_WIDE_LONG_LIBRARY)
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
    const int rc = wide::check_both(seq1_offsets, wide::Seq2{seq2_offsets}, n);
    if (rc != SWMI_OK) return rc;
    wide::fill_move_offsets(seq1_offsets, wide::Seq2{seq2_offsets}, n, move_offsets);
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

constexpr size_t kSliceBytes = size_t(256) << 20;        // an ends-only slice's device bytes
constexpr size_t kMaxSlice = size_t(1) << 20;            // alignments per slice (and per launch)
// classes of a slice's slots: the striped one where the library has it, then the unstriped wave counts 4 .. 1
constexpr int kClasses = kWideMaxWaves + (kHasStriped ? 1 : 0);
constexpr uint32_t kCarryUnit = 2;                       // int2 per unit of TileWork::pad: carry blocks start 16-byte aligned
static_assert(kWideMaxLen1 == SWMI_WIDE_MAX_LEN1 && kWideMaxLen2 == SWMI_WIDE_MAX_LEN2);
static_assert(kHasStriped || (kMaxLen1 <= size_t(kWideMaxLen1) && kMaxLen2 <= size_t(kWideMaxLen2)),
              "without the striped class every accepted shape must be the unstriped kernels'");
static_assert(sizeof(TileWork) == 48);              // (a matrix block is whole units of 16 bytes: 1024, or a profile's entries)
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
    return code_qwords_unstriped((int)len1, (int)len2);
}

// whether the slot owns a carry block: a striped slot of more than one stripe at the narrowest width shipped (at a wider
// stripe some of these blocks stay unused; the plan does not depend on the width)
bool has_carry(size_t len1, size_t len2) { return striped(len1, len2) && len2 > size_t(1024 * kWideLongMinWidth); }

// its units of TileWork::pad
size_t carry_units(size_t len1) { return (len1 + kCarryUnit - 1) / kCarryUnit; }

// the class of a slot: kClasses = striped (kWideMaxWaves + 1), else its unstriped wave count
int slot_class(size_t len1, size_t len2) { return striped(len1, len2) ? kClasses : waves_unstriped((int)len1, (int)len2); }

// device bytes one alignment of a slice takes: inputs (`seq2_bytes` of seq2), its slot, results, its carry (8 len1) where it
// has one, and with a traceback codes, moves and count
size_t ragged_bytes(bool tb, size_t len1, size_t len2, size_t seq2_bytes)
{
    size_t b = len1 + seq2_bytes + sizeof(TileWork) + 5 * sizeof(int32_t);
    if (has_carry(len1, len2)) b += len1 * sizeof(int2);
    if (tb) b += code_qwords(len1, len2) * sizeof(uint64_t) + SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

// (the budgets are those of a seq2 per alignment in every build)
size_t budget(bool tb) { return tb ? kTbSliceAlignments * ragged_bytes(true, kMaxLen1, kMaxLen2, kMaxLen2) : kSliceBytes; }

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

#ifndef SWMI_WIDE_PROFILE_LIBRARY
int check_seq2(Seq2 q, size_t n) { return check_offsets("seq2_offsets", q.off, n, kMaxLen2); }
#endif

int check_both(const uint64_t *off1, Seq2 q, size_t n)
{
    const int rc = check_offsets("seq1_offsets", off1, n, kMaxLen1);
    return rc != SWMI_OK ? rc : check_seq2(q, n);
}

void fill_move_offsets(const uint64_t *off1, Seq2 q, size_t n, uint64_t *out)
{
    out[0] = 0;
    for (size_t k = 0; k < n; ++k) out[k + 1] = out[k] + SWMI_LOCAL_LONG_MOVE_WORDS(off1[k + 1] - off1[k], seq2_len(q, k));
}

// Slices of checked offsets: each the longest run from where the last one ended whose ragged_bytes fit the budget, at most
// kMaxSlice alignments and at least one.  first = {0, ..., n}.  Where the slots hold no seq2, the matrix block -- the profile --
// is counted once per slice.
std::vector<size_t> cut(const uint64_t *off1, Seq2 q, size_t n, bool tb)
{
    const size_t cap = budget(tb), fixed = kSeq2PerSlot ? 0 : matrix_bytes(q);
    std::vector<size_t> first{0};
    size_t bytes = fixed, m = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t len2 = seq2_len(q, k), b = ragged_bytes(tb, size_t(off1[k + 1] - off1[k]), len2, kSeq2PerSlot ? len2 : 0);
        if (m && (bytes + b > cap || m == kMaxSlice)) {
            first.push_back(k);
            bytes = fixed;
            m = 0;
        }
        bytes += b;
        ++m;
    }
    if (n) first.push_back(n);
    return first;
}

struct Plan {
    const uint64_t *off1 = nullptr;
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
int make_plan(Plan &p, const uint64_t *off1, Seq2 q, size_t n, bool tb)
{
    p.off1 = off1;
    p.move_offsets.assign(n + 1, 0);
    if (tb) fill_move_offsets(off1, q, n, p.move_offsets.data());
    p.first = cut(off1, q, n, tb);
    p.tiles.resize(n);
    p.start.resize(p.slices());
    p.code_qwords.assign(p.slices(), 0);
    std::vector<uint32_t> order;
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s], b = p.first[s + 1];
        auto len1 = [&](size_t k) { return uint32_t(off1[k + 1] - off1[k]); };
        auto len2 = [&](size_t k) { return uint32_t(seq2_len(q, k)); };
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
            p.tiles[a + x] = {off1[k] - off1[a], seq2_at(q, k) - seq2_at(q, a), code_base[k - a], p.move_offsets[k] - p.move_offsets[a],
                              uint32_t(k - a), len1(k), len2(k), owns ? uint32_t(carry) : 0u};
            if (owns) carry += carry_units(len1(k));
        }
        p.max_carry = std::max(p.max_carry, carry * kCarryUnit);
        p.code_qwords[s] = size_t(codes);
        p.max_m = std::max(p.max_m, b - a);
        p.max_seq1 = std::max(p.max_seq1, size_t(off1[b] - off1[a]));
        p.max_seq2 = std::max(p.max_seq2, size_t(seq2_at(q, b) - seq2_at(q, a)));
        p.max_codes = std::max(p.max_codes, p.code_qwords[s]);
        p.max_moves = std::max(p.max_moves, size_t(p.move_offsets[b] - p.move_offsets[a]));
    }
    return SWMI_OK;
}

struct Params {
    WideKind kind;
    const int8_t *sm;                           // the caller's matrix: 32 x 32, or the profile
    int gap_open, gap_extend;
    unsigned free_ends;
};

// the launches of slice s on the one stream: the striped slots first, at the process's stripe width, then one launch per
// unstriped wave count present, widest first
hipError_t launch_slice(const Plan &p, size_t s, const Params &c, Seq2 q, const uint8_t *s1, const uint8_t *s2, const TileWork *work,
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
        const hipError_t e = launch_unstriped(c.kind, s1, s2, work + a, size_t(b - a), waves, q, d_sm, c.gap_open, c.gap_extend, c.free_ends,
                                              scores, ends, codes, moves, counts, st);
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
    std::mutex host_mu;                             // the host entries' sets, and the pinned matrix block of a call that has to make one
    HostSet sets[2];
    unsigned char *host_sm = nullptr;
    size_t host_sm_bytes = 0;
    void release()
    {
        for (auto &x : spaces) {
            if (x.second.dev) (void)hipFree(x.second.dev);
            if (x.second.host) (void)hipHostFree(x.second.host);
            if (x.second.done) (void)hipEventDestroy(x.second.done);
        }
        spaces.clear();
        for (auto &s : sets) s.release();
        if (host_sm) (void)hipHostFree(host_sm);
        host_sm = nullptr;
        host_sm_bytes = 0;
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
int check_call(const Params &c, const void *seq1s, const uint64_t *off1, const void *seq2s, Seq2 q, size_t n,
               const void *scores, const void *ends, const void *moves, const void *counts)
{
    if (c.kind == kWideGlobal && c.free_ends > SWMI_ENDS_OVERLAP)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", c.free_ends, SWMI_ENDS_OVERLAP);
    if (matrix_missing(c.sm, q)) return fail(SWMI_ERR_INVALID_ARGUMENT, "%s", kMatrixMissing);
    if (c.gap_open < 0 || c.gap_open > 127 || c.gap_extend < 0 || c.gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", c.gap_open, c.gap_extend);
    if (!moves != !counts)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return 1;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    const int rc = check_both(off1, q, n);
    // (without the striped class the rule below refuses nothing, and a profile is not 1024 bytes)
    if (rc != SWMI_OK || c.kind != kWideGlobal || !kHasStriped) return rc;
    // the global kind's domain rule (wide_long_affine_kernels.hip): P (len1 + len2) <= 2^23
    static_assert(kHasStriped || 128 * (kMaxLen1 + kMaxLen2) <= (size_t(1) << 23),
                  "without the striped class the rule must hold for every int8 matrix at the limits, so that it refuses nothing");
    int lo = 0, hi = 0;                          // (two reductions the compiler vectorises)
    for (size_t x = 0; x < size_t(SWMI_WIDE_LETTERS * SWMI_WIDE_LETTERS); ++x) {
        lo = std::min(lo, int(c.sm[x]));
        hi = std::max(hi, int(c.sm[x]));
    }
    const long P = std::max({1, c.gap_open, c.gap_extend, -lo, hi});
    for (size_t k = 0; k < n; ++k) {
        const unsigned long long total = (off1[k + 1] - off1[k]) + seq2_len(q, k);
        if ((unsigned long long)P * total > (1ull << 23))
            return fail(SWMI_ERR_INVALID_ARGUMENT, "alignment %zu is outside the domain: P (len1 + len2) = %ld x %llu > 2^23 (P = max(1, max |score_matrix|, gap_open, gap_extend))",
                        k, P, total);
    }
    return SWMI_OK;
}

int run_device(const Params &c, const void *d_seq1s, const uint64_t *off1, const void *d_seq2s, Seq2 q, size_t n,
               void *d_scores, void *d_ends, void *d_moves, void *d_counts, void *stream)
{
    int rc = check_call(c, d_seq1s, off1, d_seq2s, q, n, d_scores, d_ends, d_moves, d_counts);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_counts)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    const bool tb = d_moves != nullptr;
    Plan p;
    rc = make_plan(p, off1, q, n, tb);
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
    const size_t sm_bytes = matrix_bytes(q), up_bytes = sm_bytes + n * sizeof(TileWork);
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
    fill_matrix(sp.host, c.sm, q);
    memcpy(sp.host + sm_bytes, p.tiles.data(), n * sizeof(TileWork));
    unsigned char *up = sp.dev + code_bytes;
    WIDE_HIP_TRY(hipMemcpyAsync(up, sp.host, up_bytes, hipMemcpyHostToDevice, st));
    WIDE_HIP_TRY(hipEventRecord(sp.done, st));
    const int8_t *d_sm = reinterpret_cast<const int8_t *>(up);
    const TileWork *work = reinterpret_cast<const TileWork *>(up + sm_bytes);
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    for (size_t s = 0; s < p.slices(); ++s) {
        const size_t a = p.first[s];
        WIDE_HIP_TRY(launch_slice(p, s, c, q, s1 + off1[a], s2 + seq2_at(q, a), work + a, d_sm, static_cast<int32_t *>(d_scores) + a,
                                  static_cast<int32_t *>(d_ends) + 4 * a, tb ? reinterpret_cast<unsigned long long *>(sp.dev) : nullptr,
                                  tb ? static_cast<unsigned long long *>(d_moves) + p.move_offsets[a] : nullptr,
                                  tb ? static_cast<uint32_t *>(d_counts) + a : nullptr, sp.dev + codes_only, st));
    }
    return SWMI_OK;
}

int run_host(const Params &c, const char *entry, const uint8_t *seq1s, const uint64_t *off1, const uint8_t *seq2s, Seq2 q,
             size_t n, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *counts)
{
    int rc = check_call(c, seq1s, off1, seq2s, q, n, scores, ends, moves, counts);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    const bool tb = moves != nullptr;
    Plan p;
    rc = make_plan(p, off1, q, n, tb);
    if (rc != SWMI_OK) return rc;
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    std::lock_guard<std::mutex> lock(ds->host_mu);
    HostSet *sets = ds->sets;
    const int n_sets = p.slices() > 1 ? 2 : 1;
    // the matrix block as the kernels read it: the caller's matrix itself, or where it has to be made (a profile) the device's
    // pinned staging block, written once per call, uploaded once per buffer set, and read by no upload any more when the call
    // returns (the last drain has synchronised both streams)
    const size_t sm_bytes = matrix_bytes(q);
    const void *sm_src = c.sm;
    if constexpr (!kMatrixAsGiven) {
        if (ds->host_sm_bytes < sm_bytes) {
            if (ds->host_sm) (void)hipHostFree(ds->host_sm);
            ds->host_sm = nullptr;
            ds->host_sm_bytes = 0;
            WIDE_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ds->host_sm), sm_bytes, 0));
            ds->host_sm_bytes = sm_bytes;
        }
        fill_matrix(ds->host_sm, c.sm, q);
        sm_src = ds->host_sm;
    }
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if (!s.stream) WIDE_HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        rc = grow(s.d1, s.have.d1, std::max<size_t>(p.max_seq1, 16));
        if (rc == SWMI_OK) rc = grow(s.d2, s.have.d2, std::max<size_t>(p.max_seq2, 16));
        if (rc == SWMI_OK) rc = grow(s.d_sm, s.have.sm, sm_bytes);
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
        const size_t seq1_bytes = size_t(off1[b] - off1[a]), seq2_bytes = size_t(seq2_at(q, b) - seq2_at(q, a));
        if (sc < size_t(n_sets)) e = hipMemcpyAsync(s.d_sm, sm_src, sm_bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && seq1_bytes) e = hipMemcpyAsync(s.d1, seq1s + off1[a], seq1_bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && seq2_bytes) e = hipMemcpyAsync(s.d2, seq2s + seq2_at(q, a), seq2_bytes, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d_work, p.tiles.data() + a, s.m * sizeof(TileWork), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = launch_slice(p, sc, c, q, s.d1, s.d2, s.d_work, s.d_sm, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr,
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

size_t WIDE_ENTRY(slices_for)(const uint64_t *seq1_offsets, WIDE_OFF2_PARAM size_t n, WIDE_LEN2_PARAM int traceback, size_t *sizes, size_t cap)
{
    if (check_both(seq1_offsets, WIDE_SEQ2_ARG, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(seq1_offsets, WIDE_SEQ2_ARG, n, traceback != 0);
    for (size_t s = 0; sizes && s + 1 < first.size() && s < cap; ++s) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

int WIDE_ENTRY(local)(const uint8_t *seq1s, const uint64_t *seq1_offsets, WIDE_SEQ2_HOST_PARAMS size_t n, WIDE_MATRIX_PARAMS, int gap_open,
                      int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return run_host({kWideLocal, WIDE_MATRIX_ARG, gap_open, gap_extend, 0}, __func__, seq1s, seq1_offsets, WIDE_SEQ2_HOST_ARG, WIDE_SEQ2_ARG, n,
                    scores, ends, moves, steps);
}

int WIDE_ENTRY(global)(const uint8_t *seq1s, const uint64_t *seq1_offsets, WIDE_SEQ2_HOST_PARAMS size_t n, WIDE_MATRIX_PARAMS, int gap_open,
                       int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return run_host({kWideGlobal, WIDE_MATRIX_ARG, gap_open, gap_extend, free_ends}, __func__, seq1s, seq1_offsets, WIDE_SEQ2_HOST_ARG,
                    WIDE_SEQ2_ARG, n, scores, ends, moves, steps);
}

int WIDE_ENTRY(local_device)(const void *d_seq1s, const uint64_t *seq1_offsets, WIDE_SEQ2_DEVICE_PARAMS size_t n, WIDE_MATRIX_PARAMS,
                             int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return run_device({kWideLocal, WIDE_MATRIX_ARG, gap_open, gap_extend, 0}, d_seq1s, seq1_offsets, WIDE_SEQ2_DEVICE_ARG, WIDE_SEQ2_ARG, n,
                      d_scores, d_ends, d_moves, d_steps, stream);
}

int WIDE_ENTRY(global_device)(const void *d_seq1s, const uint64_t *seq1_offsets, WIDE_SEQ2_DEVICE_PARAMS size_t n, WIDE_MATRIX_PARAMS,
                              int gap_open, int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves,
                              void *d_steps, void *stream)
{
    return run_device({kWideGlobal, WIDE_MATRIX_ARG, gap_open, gap_extend, free_ends}, d_seq1s, seq1_offsets, WIDE_SEQ2_DEVICE_ARG,
                      WIDE_SEQ2_ARG, n, d_scores, d_ends, d_moves, d_steps, stream);
}

// one untimed device call first (it grows the workspace, which synchronises the stream), then HIP events around `iters`
int WIDE_ENTRY(time_device)(int kind, const void *d_seq1s, const uint64_t *seq1_offsets, WIDE_SEQ2_DEVICE_PARAMS size_t n, WIDE_MATRIX_PARAMS,
                            int gap_open, int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                            void *stream, int iters, float *avg_ms)
{
    if (kind != SWMI_WIDE_LOCAL && kind != SWMI_WIDE_GLOBAL) return fail(SWMI_ERR_INVALID_ARGUMENT, "kind %d is neither local nor global", kind);
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    const Params c{kind == SWMI_WIDE_LOCAL ? kWideLocal : kWideGlobal, WIDE_MATRIX_ARG, gap_open, gap_extend,
                   kind == SWMI_WIDE_LOCAL ? 0u : free_ends};
    const Seq2 q = WIDE_SEQ2_ARG;
    const void *d_s2 = WIDE_SEQ2_DEVICE_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_device(c, d_seq1s, seq1_offsets, d_s2, q, n, d_scores, d_ends, d_moves, d_steps, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = run_device(c, d_seq1s, seq1_offsets, d_s2, q, n, d_scores, d_ends, d_moves, d_steps, stream);
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
