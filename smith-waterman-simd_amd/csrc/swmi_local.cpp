// swmi_local.cpp -- host side of the local aligner with end cell, start cell and traceback (swmi_local_*, include/swmi.h).
//
// Its device buffers hang off Context::local_state, which destroy_context (swmi_api.cpp) drops at swmi_shutdown: that file
// names no symbol of this one, so the host-only builds of swmi_api.cpp / swmi_multi.cpp (tests/test_multi_fake.py,
// tests/test_sanitizers.py) link without the local kernels.
#include "swmi_host.h"

#include <initializer_list>

namespace swmi {
namespace host {
namespace {

constexpr size_t kSliceBytes = size_t(256) << 20;   // device memory of one slice's buffers
constexpr size_t kMaxSlice = size_t(1) << 20;       // alignments per slice (and per launch)

bool len_ok(size_t len1) { return len1 >= 1 && len1 <= SWMI_LOCAL_MAX_LEN; }

size_t move_words(size_t len1) { return SWMI_LOCAL_MOVE_WORDS(len1); }

// device bytes one alignment of a slice takes: inputs, results, and with a traceback the codes and the moves
size_t bytes_per_alignment(size_t len1, bool tb)
{
    size_t b = len1 + SWMI_LOCAL_SEQ2_LEN + sizeof(int32_t) + 4 * sizeof(int32_t);
    if (tb) b += swmi::local_code_words((int)len1) * sizeof(uint32_t) + move_words(len1) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

size_t slice_size(size_t n, size_t len1, bool tb)
{
    size_t s = kSliceBytes / bytes_per_alignment(len1, tb);
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
    uint32_t *d_codes = nullptr, *d_steps = nullptr;
    unsigned long long *d_moves = nullptr;
    size_t seq1_bytes = 0, alignments = 0, code_words = 0, move_rows = 0;   // capacity
    size_t off = 0, m = 0;                                                  // slice in flight
    void release()
    {
        free_all({d1, d2, d_scores, d_ends, d_codes, d_steps, d_moves});
        *this = HostSet{};
    }
};

struct LocalState {
    std::mutex mu;                                   // the device-entry workspaces
    std::map<hipStream_t, Workspace> workspaces;     // codes of one slice per caller stream
    HostSet sets[2];                                 // host entry, used under Context::mu
    ~LocalState()
    {
        for (auto &w : workspaces)
            if (w.second.ptr) (void)hipFree(w.second.ptr);
        for (auto &s : sets) s.release();
    }
};

LocalState &state(Context &ctx)
{
    std::lock_guard<std::mutex> lock(ctx.ws_mu);
    if (!ctx.local_state) ctx.local_state = std::make_shared<LocalState>();
    return *static_cast<LocalState *>(ctx.local_state.get());
}

int check_local(size_t len1, const int8_t *sm, int gap)
{
    if (!len_ok(len1)) return fail(SWMI_ERR_INVALID_ARGUMENT, "len1 %zu outside [1, %d]", len1, SWMI_LOCAL_MAX_LEN);
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

size_t swmi_local_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap)
{
    if (!len_ok(len1)) return 0;
    const size_t s = slice_size(n, len1, traceback != 0);
    size_t count = 0;
    for (size_t off = 0; off < n; off += s, ++count)
        if (sizes && count < cap) sizes[count] = n - off < s ? n - off : s;
    return count;
}

int swmi_local_align_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                            int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    int rc = check_local(len1, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    if (!d_moves != !d_steps) return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!d_seq1s || !d_seq2s || !d_scores || !d_ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL device buffer with n = %zu", n);
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_steps)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = d_moves != nullptr;
    const size_t slice = slice_size(n, len1, tb), mw = move_words(len1), cw = swmi::local_code_words((int)len1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LocalState &ls = state(*ctx);
    // one workspace per (context, stream), looked up, grown and handed to the launches under one lock (growing waits for
    // this stream only: earlier launches on it may still use the old one)
    std::lock_guard<std::mutex> lock(ls.mu);
    uint32_t *codes = nullptr;
    if (tb) {
        Workspace &ws = ls.workspaces[st];
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
        HIP_TRY(swmi::launch_local(s1 + off * len1, s2 + off * SWMI_LOCAL_SEQ2_LEN, (int)len1, m, score_matrix, gap_penalty,
                                   static_cast<int32_t *>(d_scores) + off, static_cast<int32_t *>(d_ends) + 4 * off, codes,
                                   tb ? static_cast<unsigned long long *>(d_moves) + off * mw : nullptr,
                                   tb ? static_cast<uint32_t *>(d_steps) + off : nullptr, mw, st));
    }
    return SWMI_OK;
}

int swmi_local_align(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    int rc = check_local(len1, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    if (!moves != !steps) return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = moves != nullptr;
    const size_t slice = slice_size(n, len1, tb), mw = move_words(len1), cw = swmi::local_code_words((int)len1);
    LocalState &ls = state(*ctx);
    std::lock_guard<std::mutex> lock(ctx->mu);
    HostSet *sets = ls.sets;
    const int n_sets = n > slice ? 2 : 1;
    hipStream_t streams[2] = {ctx->slots[0].stream, ctx->slots[1].stream};
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        if ((rc = grow(reinterpret_cast<void **>(&s.d1), &s.seq1_bytes, slice * len1, 1)) != SWMI_OK) return rc;
        if (s.alignments < slice) {
            free_all({s.d2, s.d_scores, s.d_ends, s.d_steps});
            s.d2 = nullptr; s.d_scores = nullptr; s.d_ends = nullptr; s.d_steps = nullptr; s.alignments = 0;
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d2), slice * SWMI_LOCAL_SEQ2_LEN));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_scores), slice * sizeof(int32_t)));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_ends), slice * 4 * sizeof(int32_t)));
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d_steps), slice * sizeof(uint32_t)));
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
        if (r == hipSuccess) r = hipMemcpyAsync(ends + 4 * s.off, s.d_ends, s.m * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(steps + s.off, s.d_steps, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        if (r == hipSuccess && tb) {
            uint32_t longest = 0;
            for (size_t k = 0; k < s.m; ++k) longest = steps[s.off + k] > longest ? steps[s.off + k] : longest;
            if (longest) {
                const size_t pitch = mw * sizeof(uint64_t), words = (longest + 31) / 32;
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
        if (e == hipSuccess) e = hipMemcpyAsync(s.d2, seq2s + off * SWMI_LOCAL_SEQ2_LEN, s.m * SWMI_LOCAL_SEQ2_LEN, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = swmi::launch_local(s.d1, s.d2, (int)len1, s.m, score_matrix, gap_penalty, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr,
                                   tb ? s.d_moves : nullptr, tb ? s.d_steps : nullptr, mw, st);
        if (e == hipSuccess && n_sets == 2) e = drain(turn ^ 1);         // the previous slice, while this one computes
    }
    for (int k = 0; k < n_sets; ++k) {
        if (e == hipSuccess) e = drain(k);
        if (e != hipSuccess) (void)hipStreamSynchronize(streams[k]);
        sets[k].m = 0;
    }
    if (e != hipSuccess) return fail(SWMI_ERR_HIP, "swmi_local_align: %s", hipGetErrorString(e));
    return SWMI_OK;
}

// The reference's list (source.cpp:1571-1572: from the start cell to the end cell) from the walk's moves: the start cell is
// the end cell less the moves' row / column steps, and the list applies the moves last to first.
int swmi_local_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    if ((!moves && steps) || (!positions && cap)) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (end_i < 0 || end_j < 0 || end_i > SWMI_LOCAL_MAX_LEN || end_j > SWMI_LOCAL_SEQ2_LEN)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "end cell (%d, %d) outside the matrix", end_i, end_j);
    if (steps > (uint32_t)end_i + (uint32_t)end_j) return fail(SWMI_ERR_INVALID_ARGUMENT, "%u steps cannot start inside the matrix from (%d, %d)", steps, end_i, end_j);
    int32_t i = end_i, j = end_j;
    for (uint32_t t = 0; t < steps; ++t) {
        const unsigned c = unsigned(moves[t >> 5] >> (2 * (t & 31))) & 3u;
        if (c == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "move %u is 0", t);
        i -= c != 1;
        j -= c != 2;
    }
    if (i < 0 || j < 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "the moves leave the matrix");
    const size_t count = size_t(steps) + 1 < cap ? size_t(steps) + 1 : cap;
    for (size_t k = 0; k < count; ++k) {
        positions[2 * k] = i;
        positions[2 * k + 1] = j;
        if (k + 1 < count) {
            const uint32_t t = steps - 1 - uint32_t(k);          // the move that leads from list position k to k + 1
            const unsigned c = unsigned(moves[t >> 5] >> (2 * (t & 31))) & 3u;
            i += c != 1;
            j += c != 2;
        }
    }
    return SWMI_OK;
}

int swmi_local_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                           int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                           float *avg_ms)
{
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    if (!current()) return last_status();
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one untimed call first: it grows the workspace (which synchronises the stream)
    int rc = swmi_local_align_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves, d_steps, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = swmi_local_align_device(d_seq1s, len1, d_seq2s, n, score_matrix, gap_penalty, d_scores, d_ends, d_moves, d_steps, stream);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventRecord(ev[1], st);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventSynchronize(ev[1]);
    float ms = 0.f;
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (auto &x : ev)
        if (x) (void)hipEventDestroy(x);
    if (he != hipSuccess) return fail(SWMI_ERR_HIP, "swmi_local_time_device: %s", hipGetErrorString(he));
    if (rc == SWMI_OK) *avg_ms = ms / iters;
    return rc;
}

}  // extern "C"
