// banded_api.cpp -- the C entries of libswmi_banded.so (include/swmi_banded.h): banded local alignment
// with affine gaps on a batch of one (len1, len2) with a diagonal per alignment.  Self-contained as wide_api.cpp is: no Context
// of libswmi.so, no swmi_init -- every entry runs on the calling thread's current HIP device, with this file's own workspaces
// per (device, stream), its own two streams and buffer sets per device for the host entry, and its own thread-local error
// text.  Of libswmi.so, linked for the callers' expander, it calls nothing.  The slices are swmi_table.cpp's for one shape:
// equal runs in caller order within a byte budget.  This file's name lies outside csrc/swmi_*.cpp, which four host-only test
// programs glob.
//
// Compiled a second time with -DSWMI_BANDED_GLOBAL_LIBRARY it is the host side of libswmi_banded_global.so
// (include/swmi_banded_global.h).  Three things differ there: the entries' names, free_ends in Call with
// its check, and the launcher and code-size function taken from banded_internal.h.
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
#include "../../include/swmi_banded_global.h"
#define BANDED_ENTRY(name) swmi_banded_global##name
#define BANDED_ALIGN swmi_banded_global
#define BANDED_ALIGN_DEVICE swmi_banded_global_device
#define BANDED_MASK_PARAM unsigned free_ends,          // behind gap_extend in the three aligning entries
#define BANDED_MASK_ARG , free_ends                    // ... and behind it in their Call
#else
#include "../../include/swmi_banded.h"
#define BANDED_ENTRY(name) swmi_banded##name
#define BANDED_ALIGN swmi_banded_local
#define BANDED_ALIGN_DEVICE swmi_banded_local_device
#define BANDED_MASK_PARAM
#define BANDED_MASK_ARG
#endif
#include "banded_internal.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>

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

#define BANDED_HIP_TRY(expr)                                                                                        \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess) return fail(SWMI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#ifdef SWMI_BANDED_GLOBAL_LIBRARY
static_assert(kBandMaxLen == SWMI_BANDED_GLOBAL_MAX_LEN && kBandWidth == SWMI_BANDED_GLOBAL_WIDTH);
constexpr size_t code_bytes(size_t len1) { return band_global_code_bytes(len1); }
#else
static_assert(kBandMaxLen == SWMI_BANDED_MAX_LEN && kBandWidth == SWMI_BANDED_WIDTH);
constexpr size_t code_bytes(size_t len1) { return band_code_bytes(len1); }
#endif
constexpr size_t kSliceBytes = size_t(256) << 20;        // an ends-only slice's device bytes
constexpr size_t kMaxSlice = size_t(1) << 20;            // alignments per slice (and per launch)
// A traceback slice's device bytes: swmi_local_affine_slices_for's budget, 4096 alignments of its largest shape (len1 = 16384
// against 128: sequences, score, ends, 262400 code dwords, SWMI_LOCAL_MOVE_WORDS(16384) = 516 move words, steps).
constexpr size_t kTbSliceBytes = size_t(4096) * (16384 + 128 + 4 + 16 + 4 * size_t(262400) + 8 * 516 + 4);
static_assert(SWMI_LOCAL_MOVE_WORDS(16384) == 516 && kTbSliceBytes == 4383801344ull);

struct Call {
    size_t len1, len2, n;
    const int8_t *sm;
    int gap_open, gap_extend;
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
    unsigned free_ends;
#endif
    size_t move_words() const { return SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2); }
};

// device bytes one alignment of a slice takes: inputs with its diagonal, results, and with a traceback codes, moves and count
size_t alignment_bytes(const Call &c, bool tb)
{
    size_t b = c.len1 + c.len2 + sizeof(int32_t) + 5 * sizeof(int32_t);
    if (tb) b += code_bytes(c.len1) + c.move_words() * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

bool lengths_ok(size_t len1, size_t len2) { return len1 >= 1 && len1 <= size_t(kBandMaxLen) && len2 >= 1 && len2 <= size_t(kBandMaxLen); }

// alignments per slice of a call with checked lengths
size_t slice_size(const Call &c, bool tb)
{
    size_t s = (tb ? kTbSliceBytes : kSliceBytes) / alignment_bytes(c, tb);
    s = std::min(s, kMaxSlice);
    s = std::max<size_t>(s, 1);
    return std::min(s, c.n);
}

// The checks in swmi_wide.h's order: the matrix and the gaps (and the mask), the moves / steps pair; then n = 0, the buffers,
// the lengths.
// 1 = nothing to do.
int check_call(const Call &c, const void *seq1s, const void *seq2s, const void *scores, const void *ends, const void *moves,
               const void *steps)
{
    if (!c.sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (c.gap_open < 0 || c.gap_open > 127 || c.gap_extend < 0 || c.gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", c.gap_open, c.gap_extend);
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
    if (c.free_ends > SWMI_BANDED_MAX_FREE_ENDS)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u is not a mask of SWMI_FREE_* (0..15) or SWMI_BANDED_END_ANYWHERE with SWMI_FREE_BEGIN* (16..19)", c.free_ends);
#endif
    if (!moves != !steps)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (c.n == 0) return 1;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", c.n);
    if (!lengths_ok(c.len1, c.len2))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "len1 %zu / len2 %zu outside [1,%d]", c.len1, c.len2, kBandMaxLen);
    return SWMI_OK;
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
    int32_t *d_diag = nullptr, *d_scores = nullptr, *d_ends = nullptr;
    unsigned char *d_codes = nullptr;
    unsigned long long *d_moves = nullptr;
    uint32_t *d_steps = nullptr;
    struct { size_t d1, d2, diag, scores, ends, codes, moves, steps; } have{};
    size_t off = 0, m = 0;                          // slice in flight
    void release()
    {
        for (void *q : {(void *)d1, (void *)d2, (void *)d_diag, (void *)d_scores, (void *)d_ends, (void *)d_codes, (void *)d_moves,
                        (void *)d_steps})
            if (q) (void)hipFree(q);
        if (stream) (void)hipStreamDestroy(stream);      // (made again by the next host call)
        *this = HostSet{};
    }
};

struct DeviceState {
    std::mutex ws_mu;                               // the device entries' workspaces: the codes of one slice per caller stream
    std::map<hipStream_t, std::pair<unsigned char *, size_t>> spaces;
    std::mutex host_mu;                             // the host entry's sets
    HostSet sets[2];
    void release()
    {
        for (auto &x : spaces)
            if (x.second.first) (void)hipFree(x.second.first);
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

hipError_t launch(const Call &c, const uint8_t *s1, const uint8_t *s2, const int32_t *diag, size_t m, int32_t *scores, int32_t *ends,
                  unsigned char *codes, unsigned long long *moves, uint32_t *steps, hipStream_t st)
{
#ifdef SWMI_BANDED_GLOBAL_LIBRARY
    return launch_banded_global(s1, (int)c.len1, s2, (int)c.len2, diag, m, c.sm, c.gap_open, c.gap_extend, c.free_ends, scores, ends, codes,
                                moves, c.move_words(), steps, st);
#else
    return launch_banded_local(s1, (int)c.len1, s2, (int)c.len2, diag, m, c.sm, c.gap_open, c.gap_extend, scores, ends, codes, moves,
                               c.move_words(), steps, st);
#endif
}

int run_device(const Call &c, const void *d_seq1s, const void *d_seq2s, const void *d_diagonals, void *d_scores, void *d_ends,
               void *d_moves, void *d_steps, void *stream)
{
    int rc = check_call(c, d_seq1s, d_seq2s, d_scores, d_ends, d_moves, d_steps);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_diagonals) |
         reinterpret_cast<uintptr_t>(d_scores) | reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) |
         reinterpret_cast<uintptr_t>(d_steps)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    const bool tb = d_moves != nullptr;
    const size_t slice = slice_size(c, tb);
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one workspace per (device, stream), looked up, grown and handed to the launches under one lock (growing waits for this
    // stream only: earlier launches on it may still use the old one)
    std::lock_guard<std::mutex> lock(ds->ws_mu);
    unsigned char *codes = nullptr;
    if (tb) {
        auto &sp = ds->spaces[st];
        const size_t need = slice * code_bytes(c.len1);
        if (need > sp.second) {
            BANDED_HIP_TRY(hipStreamSynchronize(st));
            if (sp.first) (void)hipFree(sp.first);
            sp = {nullptr, 0};
            BANDED_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sp.first), need));
            sp.second = need;
        }
        codes = sp.first;
    }
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    const int32_t *diag = static_cast<const int32_t *>(d_diagonals);
    for (size_t a = 0; a < c.n; a += slice) {
        const size_t m = std::min(slice, c.n - a);
        BANDED_HIP_TRY(launch(c, s1 + a * c.len1, s2 + a * c.len2, diag ? diag + a : nullptr, m, static_cast<int32_t *>(d_scores) + a,
                              static_cast<int32_t *>(d_ends) + 4 * a, codes,
                              tb ? static_cast<unsigned long long *>(d_moves) + a * c.move_words() : nullptr, tb ? static_cast<uint32_t *>(d_steps) + a : nullptr,
                              st));
    }
    return SWMI_OK;
}

int run_host(const Call &c, const char *entry, const uint8_t *seq1s, const uint8_t *seq2s, const int32_t *diagonals, int32_t *scores,
             int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    int rc = check_call(c, seq1s, seq2s, scores, ends, moves, steps);
    if (rc != SWMI_OK) return rc > 0 ? SWMI_OK : rc;
    const bool tb = moves != nullptr;
    const size_t slice = slice_size(c, tb), n_slices = (c.n + slice - 1) / slice, mw = c.move_words();
    DeviceState *ds = nullptr;
    rc = current(&ds);
    if (rc != SWMI_OK) return rc;
    std::lock_guard<std::mutex> lock(ds->host_mu);
    HostSet *sets = ds->sets;
    const int n_sets = n_slices > 1 ? 2 : 1;
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if (!s.stream) BANDED_HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        rc = grow(s.d1, s.have.d1, std::max<size_t>(slice * c.len1, 16));
        if (rc == SWMI_OK) rc = grow(s.d2, s.have.d2, std::max<size_t>(slice * c.len2, 16));
        if (rc == SWMI_OK && diagonals) rc = grow(s.d_diag, s.have.diag, std::max<size_t>(slice, 4));
        if (rc == SWMI_OK) rc = grow(s.d_scores, s.have.scores, std::max<size_t>(slice, 4));
        if (rc == SWMI_OK) rc = grow(s.d_ends, s.have.ends, slice * 4);
        if (rc == SWMI_OK && tb) rc = grow(s.d_steps, s.have.steps, std::max<size_t>(slice, 4));
        if (rc == SWMI_OK && tb) rc = grow(s.d_codes, s.have.codes, slice * code_bytes(c.len1));
        if (rc == SWMI_OK && tb) rc = grow(s.d_moves, s.have.moves, slice * mw);
        if (rc != SWMI_OK) return rc;
    }
    // results of the slice a set holds -> host, at the caller's positions
    auto drain = [&](int which) -> hipError_t {
        HostSet &s = sets[which];
        if (s.m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(scores + s.off, s.d_scores, s.m * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess) r = hipMemcpyAsync(ends + 4 * s.off, s.d_ends, s.m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(steps + s.off, s.d_steps, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(moves + s.off * mw, s.d_moves, s.m * mw * sizeof(uint64_t), hipMemcpyDeviceToHost, s.stream);
        if (r == hipSuccess) r = hipStreamSynchronize(s.stream);
        s.m = 0;
        return r;
    };
    hipError_t e = hipSuccess;
    int turn = 0;
    for (size_t sc = 0; e == hipSuccess && sc < n_slices; ++sc, turn ^= 1) {
        const int which = n_sets == 2 ? turn : 0;
        HostSet &s = sets[which];
        e = drain(which);                                   // (two slices ago; normally already empty)
        if (e != hipSuccess) break;
        s.off = sc * slice;
        s.m = std::min(slice, c.n - s.off);
        e = hipMemcpyAsync(s.d1, seq1s + s.off * c.len1, s.m * c.len1, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d2, seq2s + s.off * c.len2, s.m * c.len2, hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess && diagonals)
            e = hipMemcpyAsync(s.d_diag, diagonals + s.off, s.m * sizeof(int32_t), hipMemcpyHostToDevice, s.stream);
        if (e == hipSuccess)
            e = launch(c, s.d1, s.d2, diagonals ? s.d_diag : nullptr, s.m, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr,
                       tb ? s.d_moves : nullptr, tb ? s.d_steps : nullptr, s.stream);
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

const char *BANDED_ENTRY(_last_error)(void) { return t_error; }

int BANDED_ENTRY(_version)(void) { return SWMI_VERSION; }

int BANDED_ENTRY(_release_workspaces)(void)
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

size_t BANDED_ENTRY(_slices_for)(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!lengths_ok(len1, len2)) {
        (void)fail(SWMI_ERR_INVALID_ARGUMENT, "len1 %zu / len2 %zu outside [1,%d]", len1, len2, kBandMaxLen);
        return 0;
    }
    if (n == 0) return 0;
    Call c{};
    c.len1 = len1;
    c.len2 = len2;
    c.n = n;
    const size_t s = slice_size(c, traceback != 0);
    size_t count = 0;
    for (size_t off = 0; off < n; off += s, ++count)
        if (sizes && count < cap) sizes[count] = std::min(s, n - off);
    return count;
}

int BANDED_ALIGN(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int32_t *diagonals,
                 const int8_t score_matrix[16], int gap_open, int gap_extend, BANDED_MASK_PARAM int32_t *scores, int32_t *ends,
                 uint64_t *moves, uint32_t *steps)
{
    return run_host(Call{len1, len2, n, score_matrix, gap_open, gap_extend BANDED_MASK_ARG}, __func__, seq1s, seq2s, diagonals, scores, ends,
                    moves, steps);
}

int BANDED_ALIGN_DEVICE(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const void *d_diagonals,
                        const int8_t score_matrix[16], int gap_open, int gap_extend, BANDED_MASK_PARAM void *d_scores, void *d_ends,
                        void *d_moves, void *d_steps, void *stream)
{
    return run_device(Call{len1, len2, n, score_matrix, gap_open, gap_extend BANDED_MASK_ARG}, d_seq1s, d_seq2s, d_diagonals, d_scores,
                      d_ends, d_moves, d_steps, stream);
}

// one untimed device call first (it grows the workspace, which synchronises the stream), then HIP events around `iters`
int BANDED_ENTRY(_time_device)(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const void *d_diagonals,
                               const int8_t score_matrix[16], int gap_open, int gap_extend, BANDED_MASK_PARAM void *d_scores, void *d_ends,
                               void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    const Call c{len1, len2, n, score_matrix, gap_open, gap_extend BANDED_MASK_ARG};
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = run_device(c, d_seq1s, d_seq2s, d_diagonals, d_scores, d_ends, d_moves, d_steps, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = run_device(c, d_seq1s, d_seq2s, d_diagonals, d_scores, d_ends, d_moves, d_steps, stream);
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
