// fake_hip.cpp -- TEST INFRASTRUCTURE ONLY: a recording stand-in for the HIP runtime and for the kernel launchers, so that the
// product's HOST code (swmi_api.cpp, swmi_multi.cpp, swmi_table.cpp, table_api.cpp; with a driver's own stand-ins for the
// ragged launchers also local_ragged_api.cpp and tile_ragged_api.cpp) can run on a machine with no GPU at all:
// FAKE_HIP_DEVICES "gfx950" devices whose memory is host memory, copies that happen at once -- EXCEPT device-to-host copies on
// a stream (hipMemcpyAsync and hipMemcpy2DAsync), which are held back until that stream (or the device, or an event) is
// synchronised and read the device buffer
// THEN: a host pipeline that lets later kernels overwrite a score buffer before its copy-back has drained hands back wrong
// scores here, as it would on hardware -- streams and events that only carry an id, and swmi::launch_* stand-ins that write, as the "score" of a pair, the 32-bit number found in the first four
// bytes of its seq1 -- tests/native/multi_fake.cpp stores the global pair index there, so a gathered score vector must read
// 0, 1, 2, ... whatever the sharding, the gather backend and the order of the calls.  Nothing here is linked into libswmi.so.
// Every hipMalloc / hipHostMalloc block is registered, and the DEVICE side of every copy and every launcher stand-in's reads
// and writes must lie inside ONE live block, or the process aborts with the call, the range and the block it started in:
// malloc'ed "device" memory under ASan alone can hide a large overflow that lands inside a neighbouring allocation.
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../smith-waterman-simd_amd/csrc/swmi_internal.h"

namespace {
std::mutex g_mu;
std::vector<std::string> g_log;
thread_local int t_device = 0;
int g_next_id = 1;
struct Pending { void *dst; const void *src; size_t n; };
struct Handle { int id; int device; std::vector<Pending> pending; };       // a stream (with its held-back D2H copies) or an event
std::vector<Handle *> g_streams;
void log(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void log(const char *fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> l(g_mu);
    g_log.emplace_back(buf);
}
int stream_id(hipStream_t s) { return s ? reinterpret_cast<Handle *>(s)->id : 0; }
void drain(Handle *h)                        // callers hold no lock; a stream is driven by one thread at a time
{
    for (auto &p : h->pending) memmove(p.dst, p.src, p.n);
    h->pending.clear();
}
void drain_all()
{
    std::vector<Handle *> all;
    { std::lock_guard<std::mutex> l(g_mu); all = g_streams; }
    for (Handle *h : all) drain(h);
}
// live device blocks (hipMalloc, and hipHostMalloc's mapped pinned blocks): base -> bytes
std::mutex g_blocks_mu;
std::map<uintptr_t, size_t> g_blocks;
void *add_block(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (p) {
        std::lock_guard<std::mutex> l(g_blocks_mu);
        g_blocks[reinterpret_cast<uintptr_t>(p)] = n;
    }
    return p;
}
void drop_block(const char *call, void *p)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> l(g_blocks_mu);
        if (g_blocks.erase(reinterpret_cast<uintptr_t>(p)) == 0) {
            fprintf(stderr, "fake_hip: %s(%p): not a live block\n", call, p);
            abort();
        }
    }
    free(p);
}
// [p, p + n) must lie inside one live block; `what` names the call and the operand
void check_range(const char *what, const void *p, size_t n)
{
    if (n == 0) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> l(g_blocks_mu);
    auto it = g_blocks.upper_bound(a);
    if (it != g_blocks.begin()) {
        --it;
        if (a - it->first < it->second && n <= it->second - (a - it->first)) return;
        if (a - it->first < it->second) {
            fprintf(stderr, "fake_hip: BOUNDS %s: [%p, +%zu) ends %zu bytes past its block [%p, +%zu)\n", what, p, n,
                    n - (it->second - (a - it->first)), reinterpret_cast<void *>(it->first), it->second);
            abort();
        }
    }
    fprintf(stderr, "fake_hip: BOUNDS %s: [%p, +%zu) starts in no live device block\n", what, p, n);
    abort();
}
// the device side(s) of a copy of this kind
void check_copy(const char *call, void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    char what[96];
    if (kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice) {
        snprintf(what, sizeof what, "%s destination (kind %d)", call, (int)kind);
        check_range(what, dst, n);
    }
    if (kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice) {
        snprintf(what, sizeof what, "%s source (kind %d)", call, (int)kind);
        check_range(what, src, n);
    }
    if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToDevice && kind != hipMemcpyDeviceToHost) {
        fprintf(stderr, "fake_hip: %s with kind %d: the fake knows no device side for it\n", call, (int)kind);
        abort();
    }
}
int device_count()
{
    const char *e = getenv("FAKE_HIP_DEVICES");
    return e ? atoi(e) : 3;
}
}  // namespace

// the test driver reads and clears the call log through these
extern "C" size_t fake_hip_log_size() { std::lock_guard<std::mutex> l(g_mu); return g_log.size(); }
extern "C" const char *fake_hip_log_at(size_t k) { std::lock_guard<std::mutex> l(g_mu); return k < g_log.size() ? g_log[k].c_str() : ""; }
extern "C" void fake_hip_log_clear() { std::lock_guard<std::mutex> l(g_mu); g_log.clear(); }

extern "C" {
hipError_t hipGetDeviceCount(int *count) { *count = device_count(); return *count > 0 ? hipSuccess : hipErrorNoDevice; }
hipError_t hipSetDevice(int d) { if (d < 0 || d >= device_count()) return hipErrorInvalidDevice; t_device = d; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *p, int d)
{
    memset(p, 0, sizeof *p);
    snprintf(p->gcnArchName, sizeof p->gcnArchName, "gfx950:sramecc+:xnack-");
    snprintf(p->name, sizeof p->name, "fake MI355X #%d", d);
    p->multiProcessorCount = 256; p->warpSize = 64; p->clockRate = 2400000; p->totalGlobalMem = size_t(288) << 30;
    return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake HIP error"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t n)
{
    *p = add_block(n);
    log("dev%d malloc bytes%zu", t_device, n);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p) { drop_block("hipFree", p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = add_block(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { drop_block("hipHostFree", p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    std::lock_guard<std::mutex> l(g_mu);
    Handle *h = new Handle{g_next_id++, t_device, {}};
    g_streams.push_back(h);
    *s = reinterpret_cast<hipStream_t>(h);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    Handle *h = reinterpret_cast<Handle *>(s);
    drain(h);
    {
        std::lock_guard<std::mutex> l(g_mu);
        for (size_t k = 0; k < g_streams.size(); ++k)
            if (g_streams[k] == h) { g_streams.erase(g_streams.begin() + k); break; }
    }
    delete h;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    log("dev%d stream_sync stream%d", t_device, stream_id(s));
    if (s) drain(reinterpret_cast<Handle *>(s));
    return hipSuccess;
}
hipError_t hipDeviceSynchronize() { drain_all(); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e)
{
    std::lock_guard<std::mutex> l(g_mu);
    *e = reinterpret_cast<hipEvent_t>(new Handle{g_next_id++, t_device, {}});
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<Handle *>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { log("dev%d event_record ev%d stream%d", t_device, reinterpret_cast<Handle *>(e)->id, stream_id(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { drain_all(); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 1.0f; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { log("dev%d stream_wait stream%d ev%d", t_device, stream_id(s), reinterpret_cast<Handle *>(e)->id); return hipSuccess; }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    log("dev%d memcpy kind%d bytes%zu stream%d", t_device, (int)kind, n, stream_id(s));
    check_copy(s ? "hipMemcpyAsync" : "hipMemcpy", dst, src, n, kind);
    if (kind == hipMemcpyDeviceToHost && s) reinterpret_cast<Handle *>(s)->pending.push_back(Pending{dst, src, n});
    else memmove(dst, src, n);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) { return hipMemcpyAsync(dst, src, n, kind, nullptr); }
hipError_t hipMemcpyPeerAsync(void *dst, int dst_dev, const void *src, int src_dev, size_t n, hipStream_t s)
{
    check_range("hipMemcpyPeerAsync destination", dst, n);
    check_range("hipMemcpyPeerAsync source", src, n);
    memmove(dst, src, n);
    log("dev%d memcpy_peer dst_dev%d src_dev%d bytes%zu stream%d", t_device, dst_dev, src_dev, n, stream_id(s));
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t s)
{
    log("dev%d memcpy2d kind%d width%zu height%zu stream%d", t_device, (int)kind, width, height, stream_id(s));
    if (height) {   // each side spans (height - 1) pitches + one row
        const size_t dst_n = (height - 1) * dpitch + width, src_n = (height - 1) * spitch + width;
        if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToDevice && kind != hipMemcpyDeviceToHost) check_copy("hipMemcpy2DAsync", dst, src, 0, kind);
        if (kind != hipMemcpyDeviceToHost) check_range("hipMemcpy2DAsync destination", dst, dst_n);
        if (kind != hipMemcpyHostToDevice) check_range("hipMemcpy2DAsync source", src, src_n);
    }
    for (size_t r = 0; r < height; ++r) {          // (held back like hipMemcpyAsync's device-to-host copies, row by row)
        char *d = static_cast<char *>(dst) + r * dpitch;
        const char *from = static_cast<const char *>(src) + r * spitch;
        if (kind == hipMemcpyDeviceToHost && s) reinterpret_cast<Handle *>(s)->pending.push_back(Pending{d, from, width});
        else memmove(d, from, width);
    }
    return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int *can, int a, int b) { *can = a != b; return hipSuccess; }
hipError_t hipDeviceEnablePeerAccess(int peer, unsigned) { log("dev%d enable_peer dev%d", t_device, peer); return hipSuccess; }
}  // extern "C"

// ---- stand-ins for the kernel launchers (sw_kernels.hip, sg_kernels.hip and the fourteen fixed-shape table aligners') -------
namespace swmi {
bool schedule_supported(int L) { return L == 64 || L == 32 || L == 16 || L == 8 || L == 4 || L == 2; }
static void fake_scores(const uint8_t *s1, size_t stride, int32_t *out, size_t n)
{
    for (size_t k = 0; k < n; ++k) memcpy(&out[k], s1 + k * stride, 4);       // "score" = the number in the pair's first four bytes
}
hipError_t launch_score(const LaunchConfig &cfg, const uint8_t *s1, const uint8_t *s2, int32_t *out, size_t n, const SmRows &, int,
                        bool packed, hipStream_t st)
{
    log("dev%d launch_score n%zu lanes%d stream%d", t_device, n, cfg.lanes_per_alignment, stream_id(st));
    const size_t stride = packed ? 32 : 128;
    check_range("launch_score seq1 reads", s1, n * stride);
    check_range("launch_score seq2 reads", s2, n * stride);
    check_range("launch_score score writes", out, n * sizeof(int32_t));
    fake_scores(s1, stride, out, n);
    return hipSuccess;
}
hipError_t launch_score_one_vs_many(const LaunchConfig &, const uint8_t *s1, const uint8_t *s2, int32_t *out, size_t n, const SmRows &, int, hipStream_t st)
{
    log("dev%d launch_one_vs_many n%zu stream%d", t_device, n, stream_id(st));
    check_range("launch_score_one_vs_many seq1 reads", s1, n * 128);
    check_range("launch_score_one_vs_many seq2 reads", s2, n ? 128 : 0);
    check_range("launch_score_one_vs_many score writes", out, n * sizeof(int32_t));
    fake_scores(s1, 128, out, n);
    return hipSuccess;
}
hipError_t launch_generate(uint8_t *s1, uint8_t *s2, size_t n, uint64_t, uint64_t first_pair, hipStream_t st)
{
    log("dev%d launch_generate n%zu first%llu stream%d", t_device, n, (unsigned long long)first_pair, stream_id(st));
    check_range("launch_generate seq1 writes", s1, n * 128);
    check_range("launch_generate seq2 writes", s2, n * 128);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t id = (uint32_t)(first_pair + k);
        memset(s1 + 128 * k, 0, 128); memset(s2 + 128 * k, 0, 128);
        memcpy(s1 + 128 * k, &id, 4);
    }
    return hipSuccess;
}
hipError_t launch_banded_affine(const uint8_t *, const uint8_t *, int32_t *, size_t, int, const SmRows &, int, int, hipStream_t, bool, bool) { return hipSuccess; }
int banded_affine_kernel_choice(int, const SmRows &, int, int, bool, bool) { return 0; }
hipError_t launch_unpack(const uint8_t *, uint8_t *, size_t, hipStream_t) { return hipSuccess; }
hipError_t launch_pk_max3_selftest(unsigned long long *, hipStream_t) { return hipSuccess; }
size_t semiglobal_workspace_bytes(size_t n) { return 64 * (n + 1); }
hipError_t launch_semiglobal(const uint8_t *, const uint8_t *, size_t, void *, int32_t *, int32_t *, size_t, uint32_t *, hipStream_t, hipEvent_t, int, SgTuning, unsigned long long *) { return hipSuccess; }
size_t semiglobal_move_words() { return 1040; }
void semiglobal_kernel_names(size_t, int, char *a, size_t an, char *b, size_t bn, SgTuning) { if (a && an) a[0] = 0; if (b && bn) b[0] = 0; }

// The fourteen fixed-shape table aligners (table_api.cpp names their launchers), all through fake_table.  Their code workspaces take
// a constant kFakeCodeWords dwords (half as many qwords with affine gaps) per alignment, not the kernels' formula: a slice is then
// a few thousand alignments at a small shape and the real 256 at 16384 x 16384, and the buffers stay small -- except while
// fake_hip_real_code_sizes(1) holds, for slice sizes worked out by hand (nothing may launch then: fake_table checks its codes
// against the constant).  Alignment k of a launch reads its index `id` from the first (up to) four bytes of its seq1 and writes
// score 2 id + 1, ends[e] = 8 id + e + 3, and with a traceback (id >> 20) % (32 move_words + 1) moves, reported as that +
// count_offset (steps: 0, the semi-global lengths: 1), and move word w = 0xC0DE << 48 | id << 16 | w in EVERY word of its row.
// Every operand must lie inside one live device block, the carry of a striped launch (carry_words dwords per alignment, 8-byte
// aligned) included; the carry's first and last dword are written.  One log line per launch states what the launcher was
// handed: tests/native/table_host_fake.cpp reads it back.
constexpr size_t kFakeCodeWords = 1024;
static bool g_real_code_sizes = false;
extern "C" void fake_hip_real_code_sizes(int on) { g_real_code_sizes = on != 0; }
// the kernels' own sizes: local_kernels.hip / local_affine_kernels.hip (16 lanes, trips of 8 steps) and tile_sweep.h
static size_t local_words(int len1, size_t per_step) { return size_t((len1 + 15 + 7) / 8) * 8 * per_step; }
static size_t tile_words(int len1, int len2) { return size_t((len2 + 1023) / 1024) * size_t((len1 + 63 + 31) / 32 * 8) * 256; }
static size_t tile_or_fake(int len1, int len2, size_t fake) { return g_real_code_sizes ? tile_words(len1, len2) : fake; }
extern "C" unsigned fake_hip_matrix_sum(const int8_t *sm)        // what a launch line prints for its matrix
{
    unsigned h = 0;
    for (int x = 0; x < 16; ++x) h = h * 31 + uint8_t(sm[x]);
    return h;
}

struct TableArgs {
    const char *name;
    const uint8_t *s1, *s2;
    int len1, len2;
    size_t n;
    const int8_t *sm;
    int gap, extend;
    unsigned mask;
    int32_t *scores, *ends;
    size_t n_ends;
    void *codes;
    unsigned long long *moves;
    uint32_t *counts;
    uint32_t count_offset;
    size_t move_words;
    int32_t *carry;
    size_t carry_words;         // dwords per alignment that the launch needs at `carry`
    hipStream_t st;
};
static hipError_t fake_table(const TableArgs &a)
{
    log("dev%d %s n%zu stream%d len%dx%d tb%d mask%u gap%d extend%d sm%u mw%zu carry%p", t_device, a.name, a.n, stream_id(a.st), a.len1,
        a.len2, a.moves != nullptr, a.mask, a.gap, a.extend, a.sm ? fake_hip_matrix_sum(a.sm) : 0u, a.move_words,
        static_cast<void *>(a.carry));
    char what[96];
    const auto check = [&](const char *operand, const void *p, size_t bytes) {
        snprintf(what, sizeof what, "%s %s", a.name, operand);
        check_range(what, p, bytes);
    };
    const size_t n = a.n, len1 = size_t(a.len1), len2 = size_t(a.len2);
    check("seq1 reads", a.s1, n * len1);
    check("seq2 reads", a.s2, n * len2);
    check("score writes", a.scores, n * sizeof(int32_t));
    check("end writes", a.ends, n * a.n_ends * sizeof(int32_t));
    if (a.moves) {
        check("code writes", a.codes, n * kFakeCodeWords * sizeof(uint32_t));
        check("move writes", a.moves, n * a.move_words * sizeof(uint64_t));
        check("count writes", a.counts, n * sizeof(uint32_t));
    }
    if (a.carry_words && n) {
        if (!a.carry || (reinterpret_cast<uintptr_t>(a.carry) & 7)) {
            fprintf(stderr, "fake_hip: %s: carry %p is NULL or not 8-byte aligned\n", a.name, static_cast<void *>(a.carry));
            abort();
        }
        check("carry writes", a.carry, n * a.carry_words * sizeof(int32_t));
        a.carry[0] = a.carry[n * a.carry_words - 1] = 1;
    }
    for (size_t k = 0; k < n; ++k) {
        uint32_t id = 0;
        memcpy(&id, a.s1 + k * len1, len1 < 4 ? len1 : 4);
        a.scores[k] = int32_t(2 * id + 1);
        for (size_t e = 0; e < a.n_ends; ++e) a.ends[k * a.n_ends + e] = int32_t(8 * id + e + 3);
        if (!a.moves) continue;
        a.counts[k] = uint32_t((id >> 20) % (32 * a.move_words + 1)) + a.count_offset;
        for (size_t w = 0; w < a.move_words; ++w) a.moves[k * a.move_words + w] = 0xC0DEull << 48 | uint64_t(id) << 16 | w;
    }
    return hipSuccess;
}
size_t local_code_words(int len1) { return g_real_code_sizes ? local_words(len1, 8) : kFakeCodeWords; }
size_t local_affine_code_words(int len1) { return g_real_code_sizes ? local_words(len1, 16) : kFakeCodeWords; }
size_t sgfull_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t local_full_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t global_full_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t global_long_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t local_long_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t sgfull_long_code_words(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords); }
size_t sgfull_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }
size_t local_full_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }
size_t global_full_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }
size_t global_long_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }
size_t local_long_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }
size_t sgfull_long_affine_code_qwords(int len1, int len2) { return tile_or_fake(len1, len2, kFakeCodeWords / 2); }

hipError_t launch_local(const uint8_t *s1, const uint8_t *s2, int len1, size_t n, const int8_t *sm, int gap, int32_t *scores, int32_t *ends,
                        uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw, hipStream_t st)
{
    return fake_table({"launch_local", s1, s2, len1, 128, n, sm, gap, 0, 0, scores, ends, 4, codes, moves, steps, 0, mw, nullptr, 0, st});
}
hipError_t launch_local_affine(const uint8_t *s1, const uint8_t *s2, int len1, size_t n, const int8_t *sm, int go, int ge, int32_t *scores,
                               int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw, hipStream_t st)
{
    return fake_table({"launch_local_affine", s1, s2, len1, 128, n, sm, go, ge, 0, scores, ends, 4, codes, moves, steps, 0, mw, nullptr, 0, st});
}
hipError_t launch_sgfull(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, int32_t *scores,
                         int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *lengths, size_t mw, hipStream_t st)
{
    return fake_table({"launch_sgfull", s1, s2, len1, len2, n, sm, gap, 0, 0, scores, ends, 2, codes, moves, lengths, 1, mw, nullptr, 0, st});
}
hipError_t launch_sgfull_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves, uint32_t *lengths,
                                size_t mw, hipStream_t st)
{
    return fake_table({"launch_sgfull_affine", s1, s2, len1, len2, n, sm, go, ge, 0, scores, ends, 2, codes, moves, lengths, 1, mw, nullptr,
                       0, st});
}
hipError_t launch_local_full(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, int32_t *scores,
                             int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw, hipStream_t st)
{
    return fake_table({"launch_local_full", s1, s2, len1, len2, n, sm, gap, 0, 0, scores, ends, 4, codes, moves, steps, 0, mw, nullptr, 0, st});
}
hipError_t launch_local_full_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                    int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves, uint32_t *steps,
                                    size_t mw, hipStream_t st)
{
    return fake_table({"launch_local_full_affine", s1, s2, len1, len2, n, sm, go, ge, 0, scores, ends, 4, codes, moves, steps, 0, mw,
                       nullptr, 0, st});
}
hipError_t launch_global_full(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, unsigned fe,
                              int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw,
                              hipStream_t st)
{
    return fake_table({"launch_global_full", s1, s2, len1, len2, n, sm, gap, 0, fe, scores, ends, 4, codes, moves, steps, 0, mw, nullptr, 0,
                       st});
}
hipError_t launch_global_full_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                     unsigned fe, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                                     uint32_t *steps, size_t mw, hipStream_t st)
{
    return fake_table({"launch_global_full_affine", s1, s2, len1, len2, n, sm, go, ge, fe, scores, ends, 4, codes, moves, steps, 0, mw,
                       nullptr, 0, st});
}
hipError_t launch_global_long(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, unsigned fe,
                              int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw,
                              int32_t *carry, hipStream_t st)
{
    return fake_table({"launch_global_long", s1, s2, len1, len2, n, sm, gap, 0, fe, scores, ends, 4, codes, moves, steps, 0, mw, carry,
                       len2 > 16384 ? size_t(len1) : 0, st});
}
hipError_t launch_global_long_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                     unsigned fe, int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                                     uint32_t *steps, size_t mw, int32_t *carry, hipStream_t st)
{
    return fake_table({"launch_global_long_affine", s1, s2, len1, len2, n, sm, go, ge, fe, scores, ends, 4, codes, moves, steps, 0, mw,
                       carry, len2 > 16384 ? 2 * size_t(len1) : 0, st});
}
hipError_t launch_local_long(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, int32_t *scores,
                             int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *steps, size_t mw, int32_t *carry,
                             hipStream_t st)
{
    return fake_table({"launch_local_long", s1, s2, len1, len2, n, sm, gap, 0, 0, scores, ends, 4, codes, moves, steps, 0, mw, carry,
                       len2 > 16384 ? size_t(len1) : 0, st});
}
hipError_t launch_local_long_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                    int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves, uint32_t *steps,
                                    size_t mw, int32_t *carry, hipStream_t st)
{
    return fake_table({"launch_local_long_affine", s1, s2, len1, len2, n, sm, go, ge, 0, scores, ends, 4, codes, moves, steps, 0, mw,
                       carry, len2 > 16384 ? 2 * size_t(len1) : 0, st});
}
hipError_t launch_sgfull_long(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, int32_t *scores,
                              int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *lengths, size_t mw, int32_t *carry,
                              hipStream_t st)
{
    return fake_table({"launch_sgfull_long", s1, s2, len1, len2, n, sm, gap, 0, 0, scores, ends, 2, codes, moves, lengths, 1, mw, carry,
                       len2 > 16384 ? size_t(len1) : 0, st});
}
hipError_t launch_sgfull_long_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                     int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves,
                                     uint32_t *lengths, size_t mw, int32_t *carry, hipStream_t st)
{
    return fake_table({"launch_sgfull_long_affine", s1, s2, len1, len2, n, sm, go, ge, 0, scores, ends, 2, codes, moves, lengths, 1, mw,
                       carry, len2 > 16384 ? 2 * size_t(len1) : 0, st});
}
}  // namespace swmi
