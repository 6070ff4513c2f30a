// swmi_table.cpp -- the one slice pipeline of the aligners that fill the whole table, write codes and walk them: host
// entry, device entry, timer, slice arithmetic and the per-family device buffers (DESIGN.md sections 12 to 23).  What
// differs between the aligners is data (struct Table, swmi_host.h), which table_api.cpp builds per family and the ragged
// api files (local_ragged_api.cpp, tile_ragged_api.cpp) extend with a plan.  The buffers hang off Context::table_states, which destroy_context (swmi_api.cpp) drops at
// swmi_shutdown: that file names no symbol of this one, so the host-only builds of swmi_api.cpp / swmi_multi.cpp
// (tests/test_multi_fake.py, tests/test_sanitizers.py) link without the table code -- and this file names no launcher.
#include "swmi_host.h"

#include <algorithm>
#include <initializer_list>

namespace swmi {
namespace host {
namespace {

size_t slice_size(const Table &t, size_t n, bool tb)
{
    size_t s = (tb ? t.tb_slice_bytes : kTableSliceBytes) / table_slice_bytes(t, tb);
    if (s > kTableMaxSlice) s = kTableMaxSlice;
    if (s < 1) s = 1;
    return n < s ? n : s;
}

// p holds `have` elements: reallocated for `need` if that is more
template <class T> int grow(T *&p, size_t &have, size_t need)
{
    if (have >= need) return SWMI_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    have = 0;
    SWMI_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), need * sizeof(T)));
    have = need;
    return SWMI_OK;
}

// one set of device buffers of the host entry (two slices in flight)
struct HostSet {
    uint8_t *d1 = nullptr, *d2 = nullptr;
    int32_t *d_scores = nullptr, *d_ends = nullptr;
    uint32_t *d_codes = nullptr, *d_counts = nullptr;
    unsigned long long *d_moves = nullptr;
    unsigned char *d_work = nullptr;                                         // a ragged batch's slots, as bytes
    int32_t *d_carry = nullptr;                                              // a striped aligner's carry (Table::carry_words)
    struct { size_t d1, d2, scores, ends, codes, counts, moves, work, carry; } have{};   // capacity in elements
    size_t off = 0, m = 0;                                                   // slice in flight
    void release()
    {
        for (void *p : std::initializer_list<void *>{d1, d2, d_scores, d_ends, d_codes, d_counts, d_moves, d_work, d_carry})
            if (p) (void)hipFree(p);
        *this = HostSet{};
    }
};

// pinned copy of a ragged device call's slots, read by that call's upload; `done` is recorded behind the upload
struct Staging {
    unsigned char *host = nullptr;
    size_t cap = 0;                                  // bytes
    hipEvent_t done = nullptr;
};

// the device buffers of one aligner on one context
struct TableState {
    std::mutex mu;                                   // the device-entry workspaces
    std::map<hipStream_t, Workspace> workspaces;     // codes of one slice (and a ragged batch's slots) per caller stream
    std::map<hipStream_t, Staging> staging;          // ragged slots on their way to a stream's workspace
    HostSet sets[2];                                 // host entry, used under Context::mu
    void release()
    {
        for (auto &w : workspaces)
            if (w.second.ptr) (void)hipFree(w.second.ptr);
        workspaces.clear();
        for (auto &g : staging) {
            if (g.second.host) (void)hipHostFree(g.second.host);
            if (g.second.done) (void)hipEventDestroy(g.second.done);
        }
        staging.clear();
        for (auto &s : sets) s.release();
    }
    ~TableState() { release(); }
};

TableState &state(Context &ctx, TableFamily family)
{
    std::lock_guard<std::mutex> lock(ctx.ws_mu);
    std::shared_ptr<void> &p = ctx.table_states[family];
    if (!p) p = std::make_shared<TableState>();
    return *static_cast<TableState *>(p.get());
}

// Where slice by slice a batch's data lie: evenly cut for one length, as the plan says for a ragged batch.  Offsets count
// alignments (first), seq1 and seq2 bytes (seq1, seq2) and move words (moves) from the start of the caller's arrays.
struct Slices {
    const Table &t;
    size_t n, slice;            // slice: alignments per slice of a fixed-length batch
    size_t count() const { return t.plan ? t.plan->first.size() - 1 : (n + slice - 1) / slice; }
    size_t first(size_t s) const { return t.plan ? t.plan->first[s] : s * slice; }
    size_t size(size_t s) const { return t.plan ? t.plan->first[s + 1] - t.plan->first[s] : n - s * slice < slice ? n - s * slice : slice; }
    size_t seq1(size_t k) const { return t.plan ? size_t(t.plan->seq1_offsets[k]) : k * t.len1; }
    size_t seq2(size_t k) const { return t.plan && t.plan->seq2_offsets ? size_t(t.plan->seq2_offsets[k]) : k * t.len2; }
    size_t moves(size_t k) const { return t.plan ? size_t(t.plan->move_offsets[k]) : k * t.move_words; }
    size_t codes(size_t s) const { return t.plan ? t.plan->code_words[s] : size(s) * t.code_words; }
    // capacity one set of buffers needs: alignments, seq1 bytes, seq2 bytes, code dwords, move words
    size_t max_m() const { return t.plan ? t.plan->max_m : slice; }
    size_t max_seq1() const { return t.plan ? t.plan->max_seq1 : slice * t.len1; }
    size_t max_seq2() const { return t.plan && t.plan->seq2_offsets ? t.plan->max_seq2 : max_m() * t.len2; }
    size_t max_codes() const { return t.plan ? t.plan->max_codes : slice * t.code_words; }
    size_t max_moves() const { return t.plan ? t.plan->max_moves : slice * t.move_words; }
};

hipError_t launch_table(const Table &t, size_t slice, const uint8_t *s1, const uint8_t *s2, const void *work, size_t m,
                        int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts, int32_t *carry,
                        hipStream_t st)
{
    if (t.plan) return t.plan->launch(t, slice, s1, s2, work, m, scores, ends, codes, moves, counts, st);
    if (!t.carry_words) return t.launch(t, s1, s2, m, scores, ends, codes, moves, counts, st);
    Table with_carry = t;                       // the slice's carry rides in the Table (swmi_host.h)
    with_carry.carry = carry;
    return t.launch(with_carry, s1, s2, m, scores, ends, codes, moves, counts, st);
}

}  // namespace

// device bytes one alignment of a slice takes: inputs, results, and with a traceback the codes, the moves and the count
size_t table_slice_bytes(const Table &t, bool tb)
{
    size_t b = t.len1 + t.len2 + sizeof(int32_t) + t.ends * sizeof(int32_t) + t.carry_words * sizeof(int32_t);
    if (tb) b += t.code_words * sizeof(uint32_t) + t.move_words * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

int table_check_timer(size_t n, int iters, const float *avg_ms)
{
    if (!avg_ms || iters < 1) return fail(SWMI_ERR_INVALID_ARGUMENT, "avg_ms is NULL or iters %d < 1", iters);
    if (n == 0) return fail(SWMI_ERR_INVALID_ARGUMENT, "n is 0");
    return current() ? SWMI_OK : last_status();
}

size_t table_slices_for(const Table &t, size_t n, bool tb, size_t *sizes, size_t cap)
{
    const size_t s = slice_size(t, n, tb);
    size_t count = 0;
    for (size_t off = 0; off < n; off += s, ++count)
        if (sizes && count < cap) sizes[count] = n - off < s ? n - off : s;
    return count;
}

int table_device(const Table &t, const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores, void *d_ends, void *d_moves,
                 void *d_counts, void *stream)
{
    if (!d_moves != !d_counts)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and %s must both be given (traceback) or both be NULL (ends-only)", t.count);
    if (n == 0) return SWMI_OK;
    if (!d_seq1s || !d_seq2s || !d_scores || !d_ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL device buffer with n = %zu", n);
    if ((reinterpret_cast<uintptr_t>(d_seq1s) | reinterpret_cast<uintptr_t>(d_seq2s) | reinterpret_cast<uintptr_t>(d_scores) |
         reinterpret_cast<uintptr_t>(d_ends) | reinterpret_cast<uintptr_t>(d_moves) | reinterpret_cast<uintptr_t>(d_counts)) & 15)
        return fail(SWMI_ERR_ALIGNMENT, "device pointers must be 16-byte aligned");
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = d_moves != nullptr;
    const Slices sl{t, n, t.plan ? 0 : slice_size(t, n, tb)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    TableState &ts = state(*ctx, t.state);
    // one workspace per (context, stream), looked up, grown and handed to the launches under one lock (growing waits for
    // this stream only: earlier launches on it may still use the old one).  A ragged batch's slots follow the codes.
    std::lock_guard<std::mutex> lock(ts.mu);
    uint32_t *codes = nullptr;
    unsigned char *work = nullptr;
    const size_t code_bytes = ((tb ? sl.max_codes() * sizeof(uint32_t) : 0) + 15) & ~size_t(15);
    const size_t slot_bytes = t.plan ? t.plan->slot_bytes : 0;
    // a striped aligner's carry lies behind the codes (never with a plan: carry_words is a fixed-length Table's)
    const size_t carry_bytes = (sl.max_m() * t.carry_words * sizeof(int32_t) + 15) & ~size_t(15);
    int32_t *carry = nullptr;
    const size_t need = code_bytes + carry_bytes + n * slot_bytes;
    if (need) {
        Workspace &ws = ts.workspaces[st];
        if (need > ws.bytes) {
            SWMI_HIP_TRY(hipStreamSynchronize(st));
            if (ws.ptr) (void)hipFree(ws.ptr);
            ws.ptr = nullptr;
            ws.bytes = 0;
            SWMI_HIP_TRY(hipMalloc(&ws.ptr, need));
            ws.bytes = need;
        }
        codes = tb ? static_cast<uint32_t *>(ws.ptr) : nullptr;
        if (carry_bytes) carry = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(ws.ptr) + code_bytes);
        if (t.plan) {
            // the slots go up from pinned memory that the stream's last ragged upload has finished reading
            work = static_cast<unsigned char *>(ws.ptr) + code_bytes + carry_bytes;
            Staging &g = ts.staging[st];
            if (g.done) SWMI_HIP_TRY(hipEventSynchronize(g.done));
            else SWMI_HIP_TRY(hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
            if (g.cap < n * slot_bytes) {
                if (g.host) (void)hipHostFree(g.host);
                g.host = nullptr;
                g.cap = 0;
                SWMI_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&g.host), n * slot_bytes, 0));
                g.cap = n * slot_bytes;
            }
            std::copy_n(static_cast<const unsigned char *>(t.plan->slots), n * slot_bytes, g.host);
            SWMI_HIP_TRY(hipMemcpyAsync(work, g.host, n * slot_bytes, hipMemcpyHostToDevice, st));
            SWMI_HIP_TRY(hipEventRecord(g.done, st));
        }
    }
    const uint8_t *s1 = static_cast<const uint8_t *>(d_seq1s), *s2 = static_cast<const uint8_t *>(d_seq2s);
    for (size_t s = 0; s < sl.count(); ++s) {
        const size_t off = sl.first(s);
        SWMI_HIP_TRY(launch_table(t, s, s1 + sl.seq1(off), s2 + sl.seq2(off), work ? work + off * slot_bytes : nullptr, sl.size(s),
                                  static_cast<int32_t *>(d_scores) + off, static_cast<int32_t *>(d_ends) + t.ends * off, codes,
                                  tb ? static_cast<unsigned long long *>(d_moves) + sl.moves(off) : nullptr,
                                  tb ? static_cast<uint32_t *>(d_counts) + off : nullptr, carry, st));
    }
    return SWMI_OK;
}

int table_host(const Table &t, const char *entry, const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int32_t *scores,
               int32_t *ends, uint64_t *moves, uint32_t *counts)
{
    if (!moves != !counts)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and %s must both be given (traceback) or both be NULL (ends-only)", t.count);
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    Context *ctx = current();
    if (!ctx) return last_status();
    const bool tb = moves != nullptr;
    const Slices sl{t, n, t.plan ? 0 : slice_size(t, n, tb)};
    const size_t mw = t.move_words;
    const size_t slot_bytes = t.plan ? t.plan->slot_bytes : 0;
    TableState &ts = state(*ctx, t.state);
    std::lock_guard<std::mutex> lock(ctx->mu);
    HostSet *sets = ts.sets;
    const int n_sets = sl.count() > 1 ? 2 : 1;
    hipStream_t streams[2] = {ctx->slots[0].stream, ctx->slots[1].stream};
    for (int k = 0; k < n_sets; ++k) {
        HostSet &s = sets[k];
        s.off = s.m = 0;
        const size_t slice = sl.max_m();
        int rc = grow(s.d1, s.have.d1, sl.max_seq1());
        if (rc == SWMI_OK) rc = grow(s.d2, s.have.d2, sl.max_seq2());
        if (rc == SWMI_OK) rc = grow(s.d_scores, s.have.scores, slice);
        if (rc == SWMI_OK) rc = grow(s.d_ends, s.have.ends, slice * t.ends);
        if (rc == SWMI_OK) rc = grow(s.d_counts, s.have.counts, slice);
        if (rc == SWMI_OK && tb) rc = grow(s.d_codes, s.have.codes, sl.max_codes());
        if (rc == SWMI_OK && tb) rc = grow(s.d_moves, s.have.moves, sl.max_moves());
        if (rc == SWMI_OK && t.plan) rc = grow(s.d_work, s.have.work, slice * slot_bytes);
        if (rc == SWMI_OK && t.carry_words) rc = grow(s.d_carry, s.have.carry, slice * t.carry_words);
        if (rc != SWMI_OK) return rc;
    }
    // results of the slice a set holds -> host; only as many move words per alignment as the slice's longest walk needs (a
    // ragged slice: its alignments' move words, one run in the caller's layout)
    auto drain = [&](int which) -> hipError_t {
        HostSet &s = sets[which];
        hipStream_t st = streams[which];
        if (s.m == 0) return hipSuccess;
        hipError_t r = hipMemcpyAsync(scores + s.off, s.d_scores, s.m * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess) r = hipMemcpyAsync(ends + t.ends * s.off, s.d_ends, s.m * t.ends * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess && tb) r = hipMemcpyAsync(counts + s.off, s.d_counts, s.m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (r == hipSuccess && tb && t.plan) {
            const size_t w0 = sl.moves(s.off), words = sl.moves(s.off + s.m) - w0;
            if (words) r = hipMemcpyAsync(moves + w0, s.d_moves, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        }
        if (r == hipSuccess) r = hipStreamSynchronize(st);
        if (r == hipSuccess && tb && !t.plan) {
            uint32_t longest = 0;
            for (size_t k = 0; k < s.m; ++k) longest = counts[s.off + k] > longest ? counts[s.off + k] : longest;
            if (longest > t.count_offset) {
                const size_t pitch = mw * sizeof(uint64_t), words = (longest - t.count_offset + 31) / 32;
                r = hipMemcpy2DAsync(moves + s.off * mw, pitch, s.d_moves, pitch, words * sizeof(uint64_t), s.m, hipMemcpyDeviceToHost, st);
                if (r == hipSuccess) r = hipStreamSynchronize(st);
            }
        }
        s.m = 0;
        return r;
    };
    hipError_t e = hipSuccess;
    int turn = 0;
    for (size_t sc = 0; e == hipSuccess && sc < sl.count(); ++sc, turn ^= 1) {
        const int which = n_sets == 2 ? turn : 0;
        HostSet &s = sets[which];
        hipStream_t st = streams[which];
        e = drain(which);                                   // (two slices ago; normally already empty)
        if (e != hipSuccess) break;
        const size_t off = sl.first(sc);
        s.off = off;
        s.m = sl.size(sc);
        const size_t seq1_bytes = sl.seq1(off + s.m) - sl.seq1(off);     // (0 for a ragged slice of empty seq1s only)
        if (seq1_bytes)
            e = hipMemcpyAsync(s.d1, seq1s + sl.seq1(off), seq1_bytes, hipMemcpyHostToDevice, st);
        const size_t seq2_bytes = sl.seq2(off + s.m) - sl.seq2(off);     // (0 for a ragged slice of empty seq2s only)
        if (e == hipSuccess && seq2_bytes) e = hipMemcpyAsync(s.d2, seq2s + sl.seq2(off), seq2_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && t.plan)
            e = hipMemcpyAsync(s.d_work, static_cast<const unsigned char *>(t.plan->slots) + off * slot_bytes, s.m * slot_bytes,
                               hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = launch_table(t, sc, s.d1, s.d2, s.d_work, s.m, s.d_scores, s.d_ends, tb ? s.d_codes : nullptr, tb ? s.d_moves : nullptr,
                             tb ? s.d_counts : nullptr, s.d_carry, st);
        if (e == hipSuccess && n_sets == 2) e = drain(turn ^ 1);         // the previous slice, while this one computes
    }
    for (int k = 0; k < n_sets; ++k) {
        if (e == hipSuccess) e = drain(k);
        if (e != hipSuccess) (void)hipStreamSynchronize(streams[k]);
        sets[k].m = 0;
    }
    if (e != hipSuccess) return fail(SWMI_ERR_HIP, "%s: %s", entry, hipGetErrorString(e));
    return SWMI_OK;
}

// one untimed device call first (it grows the workspace, which synchronises the stream), then HIP events around `iters`
int table_time_device(const Table &t, const char *entry, const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores,
                      void *d_ends, void *d_moves, void *d_counts, void *stream, int iters, float *avg_ms)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = table_device(t, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_counts, stream);
    if (rc != SWMI_OK) return rc;
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t he = hipEventCreate(&ev[0]);
    if (he == hipSuccess) he = hipEventCreate(&ev[1]);
    if (he == hipSuccess) he = hipEventRecord(ev[0], st);
    for (int k = 0; k < iters && he == hipSuccess && rc == SWMI_OK; ++k)
        rc = table_device(t, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_counts, stream);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventRecord(ev[1], st);
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventSynchronize(ev[1]);
    float ms = 0.f;
    if (he == hipSuccess && rc == SWMI_OK) he = hipEventElapsedTime(&ms, ev[0], ev[1]);
    for (auto &x : ev)
        if (x) (void)hipEventDestroy(x);
    if (he != hipSuccess) return fail(SWMI_ERR_HIP, "%s: %s", entry, hipGetErrorString(he));
    if (rc == SWMI_OK) *avg_ms = ms / iters;
    return rc;
}

int table_release_workspaces(TableFamily family)
{
    Context *ctx = current();
    if (!ctx) return last_status();
    SWMI_HIP_TRY(hipDeviceSynchronize());
    TableState &ts = state(*ctx, family);
    std::lock_guard<std::mutex> host_lock(ctx->mu);
    std::lock_guard<std::mutex> lock(ts.mu);
    ts.release();
    return SWMI_OK;
}

}  // namespace host
}  // namespace swmi
