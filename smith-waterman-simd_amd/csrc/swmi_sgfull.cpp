// swmi_sgfull.cpp -- host side of the exact semi-global aligner with traceback (swmi_semiglobal_full*, include/swmi.h).
//
// Its device buffers hang off Context::sgfull_state, which destroy_context (swmi_api.cpp) drops at swmi_shutdown: that file
// names no symbol of this one, so the host-only builds of swmi_api.cpp / swmi_multi.cpp (tests/test_multi_fake.py,
// tests/test_sanitizers.py) link without these kernels.
#include "swmi_host.h"

#include <initializer_list>

namespace swmi {
namespace host {
namespace {

constexpr size_t kSliceBytes = size_t(256) << 20;   // device memory of one ends-only slice's buffers
constexpr size_t kMaxSlice = size_t(1) << 20;       // alignments per slice (and per launch)

bool len_ok(size_t len) { return len >= 1 && len <= SWMI_SGFULL_MAX_LEN; }

size_t move_words(size_t len1, size_t len2) { return SWMI_SGFULL_MOVE_WORDS(len1, len2); }

// device bytes one alignment of a slice takes: inputs, results, and with a traceback the codes and the moves
size_t bytes_per_alignment(size_t len1, size_t len2, bool tb)
{
    size_t b = len1 + len2 + sizeof(int32_t) + 2 * sizeof(int32_t);
    if (tb)
        b += swmi::sgfull_code_words((int)len1, (int)len2) * sizeof(uint32_t) + move_words(len1, len2) * sizeof(uint64_t) +
             sizeof(uint32_t);
    return b;
}

// A traceback slice holds as many alignments as 256 of 16384 x 16384 (about 16.1 GiB): one workgroup per alignment, so
// that a full-size batch occupies every CU of an MI355X.  Ends-only slices hold 256 MiB of inputs and results.
size_t slice_size(size_t n, size_t len1, size_t len2, bool tb)
{
    const size_t budget = tb ? 256 * bytes_per_alignment(SWMI_SGFULL_MAX_LEN, SWMI_SGFULL_MAX_LEN, true) : kSliceBytes;
    size_t s = budget / bytes_per_alignment(len1, len2, tb);
    if (s > kMaxSlice) s = kMaxSlice;
    if (s < 1) s = 1;
    return n < s ? n : s;
}

void free_all(std::initializer_list<void *> ptrs)
{
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
}

// one set of device buffers of the host entry (two slices in flight)
struct HostSet {
    uint8_t *d1 = nullptr, *d2 = nullptr;
    int32_t *d_scores = nullptr, *d_ends = nullptr;
    uint32_t *d_codes = nullptr, *d_lengths = nullptr;
    unsigned long long *d_moves = nullptr;
    size_t seq1_bytes = 0, seq2_bytes = 0, alignments = 0, code_words = 0, move_rows = 0;   // capacity
    size_t off = 0, m = 0;                                                                // slice in flight
    void release()
    {
        free_all({d1, d2, d_scores, d_ends, d_codes, d_lengths, d_moves});
        *this = HostSet{};
    }
};

struct SgFullState {
    std::mutex mu;                                   // the device-entry workspaces
    std::map<hipStream_t, Workspace> workspaces;     // codes of one slice per caller stream
    HostSet sets[2];                                 // host entry, used under Context::mu
    void release()
    {
        for (auto &w : workspaces)
            if (w.second.ptr) (void)hipFree(w.second.ptr);
        workspaces.clear();
        for (auto &s : sets) s.release();
    }
    ~SgFullState() { release(); }
};

SgFullState &state(Context &ctx)
{
    std::lock_guard<std::mutex> lock(ctx.ws_mu);
    if (!ctx.sgfull_state) ctx.sgfull_state = std::make_shared<SgFullState>();
    return *static_cast<SgFullState *>(ctx.sgfull_state.get());
}

int check_sgfull(size_t len1, size_t len2, const int8_t *sm, int gap)
{
    if (!len_ok(len1) || !len_ok(len2))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "lengths (%zu, %zu) outside [1, %d]", len1, len2, SWMI_SGFULL_MAX_LEN);
    return check_params(sm, gap);
}

int grow(void **p, size_t *have, size_t need, size_t unit)
{
    if (*have >= need) return SWMI_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    SWMI_HIP_TRY(hipMalloc(p, need * unit));
    *have = need;
    return SWMI_OK;
}

}  // namespace
}  // namespace host
}  // namespace swmi

using namespace swmi::host;
#define HIP_TRY SWMI_HIP_TRY

extern "C" {

size_t swmi_semiglobal_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!len_ok(len1) || !len_ok(len2)) return 0;
    const size_t s = slice_size(n, len1, len2, traceback != 0);
    size_t count = 0;
    for (size_t off = 0; off < n; off += s, ++count)
        if (sizes && count < cap) sizes[count] = n - off < s ? n - off : s;
    return count;
}

int swmi_semiglobal_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_lengths, void *stream)
{
    int rc = check_sgfull(len1, len2, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    if (!d_moves != !d_lengths)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and lengths must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!d_seq1s || !d_seq2s || !d_scores || !d_ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL device buffer with n = %zu", n);
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_lengths)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = d_moves != nullptr;
    const size_t slice = slice_size(n, len1, len2, tb), mw = move_words(len1, len2);
    const size_t cw = swmi::sgfull_code_words((int)len1, (int)len2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SgFullState &fs = state(*ctx);
    // one workspace per (context, stream), looked up, grown and handed to the launches under one lock (growing waits for
    // this stream only: earlier launches on it may still use the old one)
    std::lock_guard<std::mutex> lock(fs.mu);
    uint32_t *codes = nullptr;
    if (tb) {
        Workspace &ws = fs.workspaces[st];
        const size_t need = slice * cw * sizeof(uint32_t);
        if (need > ws.bytes) {
            HIP_TRY(hipStreamSynchronize(st));
            if (ws.ptr) (void)hipFree(ws.ptr);
            ws.ptr = nullptr;
            ws.bytes = 0;
            HIP_TRY(hipMalloc(&ws.ptr, need));
            ws.bytes = need;
        }
        codes = static_cast<uint32_t *>(ws.ptr);
    }
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    for (size_t off = 0; off < n; off += slice) {
        const size_t m = n - off < slice ? n - off : slice;
        HIP_TRY(swmi::launch_sgfull(s1 + off * len1, s2 + off * len2, (int)len1, (int)len2, m, score_matrix, gap_penalty,
                                    static_cast<int32_t *>(d_scores) + off, static_cast<int32_t *>(d_ends) + 2 * off, codes,
                                    tb ? static_cast<unsigned long long *>(d_moves) + off * mw : nullptr,
                                    tb ? static_cast<uint32_t *>(d_lengths) + off : nullptr, mw, st));
    }
    return SWMI_OK;
}

int swmi_semiglobal_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                         const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves,
                         uint32_t *lengths)
{
    int rc = check_sgfull(len1, len2, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    if (!moves != !lengths)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and lengths must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = moves != nullptr;
    const size_t slice = slice_size(n, len1, len2, tb), mw = move_words(len1, len2);
    const size_t cw = swmi::sgfull_code_words((int)len1, (int)len2);
    SgFullState &fs = state(*ctx);
    std::lock_guard<std::mutex> lock(ctx->mu);
    HostSet *sets = fs.sets;
    const int n_sets = n > slice ? 2 : 1;
    hipStream_t streams[2] = {ctx->slots[0].stream, ctx->slots[1].stream};
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if ((rc = grow(reinterpret_cast<void **>(&s.d1), &s.seq1_bytes, slice * len1, 1)) != SWMI_OK) return rc;
        if ((rc = grow(reinterpret_cast<void **>(&s.d2), &s.seq2_bytes, slice * len2, 1)) != SWMI_OK) return rc;
        if (s.alignments < slice) {
            free_all({s.d_scores, s.d_ends, s.d_lengths});
            s.d_scores = nullptr; s.d_ends = nullptr; s.d_lengths = nullptr; s.alignments = 0;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_scores), slice * sizeof(int32_t)));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_ends), slice * 2 * sizeof(int32_t)));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_lengths), slice * sizeof(uint32_t)));
            s.alignments = slice;
        }
        if (tb) {
            if ((rc = grow(reinterpret_cast<void **>(&s.d_codes), &s.code_words, slice * cw, sizeof(uint32_t))) != SWMI_OK) return rc;
            if ((rc = grow(reinterpret_cast<void **>(&s.d_moves), &s.move_rows, slice * mw, sizeof(uint64_t))) != SWMI_OK) return rc;
        }
    }
    // results of the slice a set holds -> host; only as many move words per alignment as the slice's longest walk needs
    auto drain = [&](int which) -> hipError_t {
        HostSet &s = sets[which];
        hipStream_t st = streams[which];
        if (s.m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(scores + s.off, s.d_scores, s.m * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipMemcpyAsync(ends + 2 * s.off, s.d_ends, s.m * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(lengths + s.off, s.d_lengths, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        if (r == hipSuccess && tb) {
            uint32_t longest = 0;
            for (size_t k = 0; k < s.m; ++k) longest = lengths[s.off + k] > longest ? lengths[s.off + k] : longest;
            if (longest > 1) {
                const size_t pitch = mw * sizeof(uint64_t), words = (longest - 1 + 31) / 32;
                r = hipMemcpy2DAsync(moves + s.off * mw, pitch, s.d_moves, pitch, words * sizeof(uint64_t), s.m, hipMemcpyDeviceToHost, st);
                if (r == hipSuccess) r = hipStreamSynchronize(st);
            }
        }
        s.m = 0;
        return r;
    };
    hipError_t e = hipSuccess;
    int turn = 0;
    for (size_t off = 0; e == hipSuccess && off < n; off += slice, turn ^= 1) {
        const int which = n_sets == 2 ? turn : 0;
        HostSet &s = sets[which];
        hipStream_t st = streams[which];
        e = drain(which);                                   // (two slices ago; normally already empty)
        if (e != hipSuccess) break;
        s.off = off;
        s.m = n - off < slice ? n - off : slice;
        e = hipMemcpyAsync(s.d1, seq1s + off * len1, s.m * len1, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(s.d2, seq2s + off * len2, s.m * len2, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = swmi::launch_sgfull(s.d1, s.d2, (int)len1, (int)len2, s.m, score_matrix, gap_penalty, s.d_scores, s.d_ends,
                                    tb ? s.d_codes : nullptr, tb ? s.d_moves : nullptr, tb ? s.d_lengths : nullptr, mw, st);
        if (e == hipSuccess && n_sets == 2) e = drain(turn ^ 1);         // the previous slice, while this one computes
    }
    for (int k = 0; k < n_sets; ++k) {
        if (e == hipSuccess) e = drain(k);
        if (e != hipSuccess) (void)hipStreamSynchronize(streams[k]);
        sets[k].m = 0;
    }
    if (e != hipSuccess) return fail(SWMI_ERR_HIP, "swmi_semiglobal_full: %s", hipGetErrorString(e));
    return SWMI_OK;
}

int swmi_semiglobal_full_release_workspaces(void)
{
    Context *ctx = current();
    if (!ctx) return last_status();
    HIP_TRY(hipDeviceSynchronize());
    SgFullState &fs = state(*ctx);
    std::lock_guard<std::mutex> host_lock(ctx->mu);
    std::lock_guard<std::mutex> lock(fs.mu);
    fs.release();
    return SWMI_OK;
}

int swmi_semiglobal_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                     void *d_lengths, void *stream, int iters, float *avg_ms)
{
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    if (!current()) return last_status();
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one untimed call first: it grows the workspace (which synchronises the stream)
    int rc = swmi_semiglobal_full_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves,
                                         d_lengths, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = swmi_semiglobal_full_device(d_seq1s, len1, d_seq2s, len2, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves,
                                         d_lengths, stream);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventRecord(ev[1], st);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventSynchronize(ev[1]);
    float ms = 0.f;
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (auto &x : ev)
        if (x) (void)hipEventDestroy(x);
    if (he != hipSuccess) return fail(SWMI_ERR_HIP, "swmi_semiglobal_full_time_device: %s", hipGetErrorString(he));
    if (rc == SWMI_OK) *avg_ms = ms / iters;
    return rc;
}

}  // extern "C"
