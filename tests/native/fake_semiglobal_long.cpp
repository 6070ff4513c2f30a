// fake_semiglobal_long.cpp -- TEST INFRASTRUCTURE ONLY: stand-ins for the two striped semi-global launchers and their code-size
// functions (csrc/sgfull_long_kernels.hip, sgfull_long_affine_kernels.hip), linked beside fake_hip.cpp, which holds the fake HIP runtime and
// the other launchers.  They follow fake_hip.cpp's fake_table: alignment k of a launch reads its index `id` from the first (up
// to) four bytes of its seq1 and writes score 2 id + 1, ends[e] = 8 id + e + 3 (two per alignment), and with a traceback (id >> 20)
// % (32 move_words + 1) moves, reported as lengths = that + 1, and move word w = 0xC0DE << 48 | id << 16 | w in every word of its row.  fake_hip.cpp's block checker is local to
// that file, so these check by touching: the first and the last element of every operand is read or written -- the carry's n *
// carry_words dwords included, where len2 > 16384 -- so that ASan reports a block that is too small.  A carry that is needed
// must be non-NULL and 8-byte aligned.  One log line per launch, in fake_table's format, read back through
// fake_semiglobal_long_log_*.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../smith-waterman-simd_amd/csrc/swmi_internal.h"

extern "C" unsigned fake_hip_matrix_sum(const int8_t *sm);

namespace {
constexpr size_t kFakeCodeWords = 1024;     // fake_hip.cpp's: dwords of codes per alignment (512 qwords with affine gaps)
std::mutex g_mu;
std::vector<std::string> g_log;
volatile unsigned char g_sink;

// a stream of fake_hip.cpp begins with its id
int stream_id(hipStream_t s) { return s ? *reinterpret_cast<const int *>(s) : 0; }

template <class T> void touch_read(const T *p, size_t count)
{
    if (!count) return;
    g_sink = static_cast<unsigned char>(reinterpret_cast<const volatile unsigned char *>(p)[0] +
                                        reinterpret_cast<const volatile unsigned char *>(p + count)[-1]);
}
template <class T> void touch_write(T *p, size_t count)
{
    if (!count) return;
    p[0] = T{};
    p[count - 1] = T{};
}

hipError_t fake_long(const char *name, const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap,
                     int extend, int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *lengths, size_t mw,
                     int32_t *carry, size_t carry_words, hipStream_t st)
{
    char buf[256];
    snprintf(buf, sizeof buf, "dev0 %s n%zu stream%d len%dx%d tb%d mask%u gap%d extend%d sm%u mw%zu carry%p", name, n, stream_id(st), len1,
             len2, moves != nullptr, 0u, gap, extend, sm ? fake_hip_matrix_sum(sm) : 0u, mw, static_cast<void *>(carry));
    {
        std::lock_guard<std::mutex> l(g_mu);
        g_log.emplace_back(buf);
    }
    touch_read(s1, n * size_t(len1));
    touch_read(s2, n * size_t(len2));
    touch_write(scores, n);
    touch_write(ends, 2 * n);
    if (moves) {
        touch_write(codes, n * kFakeCodeWords);
        touch_write(moves, n * mw);
        touch_write(lengths, n);
    }
    if (carry_words && n) {
        if (!carry || (reinterpret_cast<uintptr_t>(carry) & 7)) {
            fprintf(stderr, "fake_semiglobal_long: %s: carry %p is NULL or not 8-byte aligned\n", name, static_cast<void *>(carry));
            abort();
        }
        touch_write(carry, n * carry_words);
    }
    for (size_t k = 0; k < n; ++k) {
        uint32_t id = 0;
        memcpy(&id, s1 + k * size_t(len1), len1 < 4 ? size_t(len1) : 4);
        scores[k] = int32_t(2 * id + 1);
        for (size_t e = 0; e < 2; ++e) ends[2 * k + e] = int32_t(8 * id + e + 3);
        if (!moves) continue;
        lengths[k] = uint32_t((id >> 20) % (32 * mw + 1)) + 1;
        for (size_t w = 0; w < mw; ++w) moves[k * mw + w] = 0xC0DEull << 48 | uint64_t(id) << 16 | w;
    }
    return hipSuccess;
}
}  // namespace

extern "C" size_t fake_semiglobal_long_log_size() { std::lock_guard<std::mutex> l(g_mu); return g_log.size(); }
extern "C" const char *fake_semiglobal_long_log_at(size_t k) { std::lock_guard<std::mutex> l(g_mu); return k < g_log.size() ? g_log[k].c_str() : ""; }
extern "C" void fake_semiglobal_long_log_clear() { std::lock_guard<std::mutex> l(g_mu); g_log.clear(); }

namespace swmi {
size_t sgfull_long_code_words(int, int) { return kFakeCodeWords; }
size_t sgfull_long_affine_code_qwords(int, int) { return kFakeCodeWords / 2; }

hipError_t launch_sgfull_long(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int gap, int32_t *scores,
                             int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *lengths, size_t mw, int32_t *carry,
                             hipStream_t st)
{
    return fake_long("launch_sgfull_long", s1, s2, len1, len2, n, sm, gap, 0, scores, ends, codes, moves, lengths, mw, carry,
                     len2 > 16384 ? size_t(len1) : 0, st);
}
hipError_t launch_sgfull_long_affine(const uint8_t *s1, const uint8_t *s2, int len1, int len2, size_t n, const int8_t *sm, int go, int ge,
                                    int32_t *scores, int32_t *ends, unsigned long long *codes, unsigned long long *moves, uint32_t *lengths,
                                    size_t mw, int32_t *carry, hipStream_t st)
{
    return fake_long("launch_sgfull_long_affine", s1, s2, len1, len2, n, sm, go, ge, scores, ends, reinterpret_cast<uint32_t *>(codes), moves,
                     lengths, mw, carry, len2 > 16384 ? 2 * size_t(len1) : 0, st);
}
}  // namespace swmi
