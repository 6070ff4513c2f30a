// banded_long_host_fake.cpp -- TEST ONLY: what is new in the host side of libswmi_banded_long.so (csrc/banded_ragged_api.cpp
// with -DSWMI_BANDED_LONG_LIBRARY) on the fake GPU of fake_hip.cpp, as a stand-alone program under ASan +
// UBSan; everything the three builds share is driven by banded_ragged_host_fake.cpp.  This file holds the stand-in for the
// launcher and hipGetDevice.  Its cases: the length bound (65536 accepted, 65537 refused, the tenth export's values by hand);
// the planner's key by hand for 65536-long pairs; and one traceback call of 131 alignments of 65536 x 65536 at band 1024, which
// the byte budget cuts into 129 + 2: per launch every slot's code offset is the running sum of the code sizes written out by
// hand, aligned to a lane's whole stores and, late in the first slice, beyond 2^32 bytes -- held as arithmetic: of the 4.3 GB of
// codes only the first and the last byte are touched --, its move offset the running sum of the move words, its diagonal the
// caller's where that is within +-131072 (65536 + 511, which a clamp at 65536 would move) and +-131072 beyond, the slots in the
// order of the key, and the results at caller positions with sentinels behind them.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/swmi_banded_long.h"
#include "../../smith-waterman-simd_amd/csrc/banded_internal.h"

using swmi::banded::RaggedSlot;

extern "C" hipError_t hipGetDevice(int *d)
{
    *d = 0;
    return hipSuccess;
}

namespace {

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (g_failed < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

int g_failed = 0;
constexpr size_t kLen = 65536, kN = 131, kFirstSlice = 129;
constexpr size_t kCodeBytes = 8 * 256 * 16400;        // band 1024: 8 bytes per lane and iteration, ceil((65536 + 64) / 4) trips
constexpr size_t kMoveWords = 4096;                   // ((65536 + 65536 + 31) / 32 + 1) & ~1
std::vector<int32_t> g_diag;                          // the caller's diagonals
size_t g_base = 0, g_launches = 0;
uint64_t g_top_code = 0;                              // the largest code offset seen, bytes

int32_t clamped(int32_t d) { return std::max(-131072, std::min(131072, d)); }

// the key, by hand, of a 65536 x 65536 pair of the global kind at band 1024: rows 0 .. 65536 are swept around the main
// diagonal; a band whose lowest diagonal d - 512 is above 0 ends at row 65536 + 512 - d, one whose highest diagonal d + 511 is
// below 0 begins at row 1 - 512 - d
int rows_by_hand(int32_t d)
{
    const long long lo = std::max(0ll, 1ll - 512 - d), hi = std::min(65536ll, 65536ll + 512 - d);
    return lo > hi ? 0 : int(hi - lo);
}

void touch(const void *p)
{
    if (hipMemcpy(const_cast<void *>(p), p, 1, hipMemcpyDeviceToDevice) != hipSuccess) abort();       // (aborts outside a live block)
}

}  // namespace

hipError_t swmi::banded::launch_banded_long(int kind, int band, const uint8_t *s1, const uint8_t *s2, const RaggedSlot *slots, size_t n,
                                            const int8_t *, int, int, unsigned free_ends, int32_t *scores, int32_t *ends, unsigned char *codes,
                                            unsigned long long *moves, uint32_t *steps, hipStream_t)
{
    const size_t base = g_base;
    ++g_launches;
    EXPECT(kind == SWMI_BANDED_LONG_GLOBAL && band == 1024 && free_ends == 5u && codes && moves && steps);
    EXPECT(n == (base == 0 ? kFirstSlice : kN - kFirstSlice));
    if (base + n > kN || !codes) abort();
    EXPECT((reinterpret_cast<uintptr_t>(codes) & 15) == 0);
    touch(codes);
    touch(codes + n * kCodeBytes - 1);                                            // the slice's codes end inside the block
    touch(s1 + n * kLen - 1);
    touch(s2 + n * kLen - 1);
    touch(reinterpret_cast<const unsigned char *>(moves + n * kMoveWords) - 1);
    std::vector<char> seen(n, 0);
    uint64_t code_at = 0;                                                        // dwords
    int last_rows = INT_MAX;
    uint32_t last_index = 0;
    for (size_t x = 0; x < n; ++x) {
        const RaggedSlot &q = slots[x];
        EXPECT(q.index < n && !seen[q.index < n ? q.index : 0]);
        if (q.index >= n) break;
        seen[q.index] = 1;
        const size_t c = base + q.index;
        EXPECT(q.len1 == int32_t(kLen) && q.len2 == int32_t(kLen));
        EXPECT(q.off1 == q.index * kLen && q.off2 == q.index * kLen);
        EXPECT(s1[q.off1] == uint8_t(c) && s2[q.off2] == uint8_t(c + 1));
        EXPECT(q.d0 == clamped(g_diag[c]));
        EXPECT(q.move_off == q.index * kMoveWords);
        EXPECT(q.code_off == code_at && q.code_off % 32 == 0);                   // a running sum: disjoint; a lane's trip is two 16-byte stores
        code_at += kCodeBytes / 4;
        g_top_code = std::max<uint64_t>(g_top_code, q.code_off * 4);
        // the planner's order: the key descending, ties in caller order; the key by hand
        const int rows = swmi::banded::width_swept_rows(kind, q.len1, q.len2, q.d0, band);
        EXPECT(rows == rows_by_hand(q.d0) && rows <= last_rows);
        if (x && rows == last_rows) EXPECT(q.index > last_index);
        last_rows = rows;
        last_index = q.index;
        scores[q.index] = 1000 + int32_t(c);
        for (int e = 0; e < 4; ++e) ends[4 * q.index + e] = q.d0 + e;
        steps[q.index] = uint32_t(c % 7);
        moves[q.move_off] = 0xC0DEull << 48 | c;
        moves[q.move_off + kMoveWords - 1] = 0xBEEFull << 48 | c;
    }
    EXPECT(code_at * 4 == n * kCodeBytes);
    g_base += n;
    return hipSuccess;
}

namespace {

void the_length_bound()
{
    const uint64_t ok[3] = {0, 65536, 65536 + 16385}, zero[3] = {0, 0, 65536}, over[3] = {0, 8, 8 + 65537};
    size_t sizes[4] = {0, 0, 0, 0};
    for (int band : {128, 256, 512, 1024})
        for (int kind : {SWMI_BANDED_LONG_LOCAL, SWMI_BANDED_LONG_GLOBAL}) {
            EXPECT(swmi_banded_long_slices_for(kind, band, ok, zero, 2, 1, sizes, 4) == 1 && sizes[0] == 2);
            EXPECT(swmi_banded_long_slices_for(kind, band, over, zero, 2, 1, sizes, 4) == 0);
            EXPECT(std::strstr(swmi_banded_long_last_error(), "alignment 1: a length above 65536"));
            EXPECT(swmi_banded_long_slices_for(kind, band, zero, over, 2, 0, sizes, 4) == 0);
        }
    // the tenth export: ((len1 + len2 + 31) / 32 + 1) & ~1 words each -- (65536, 0): (2048 + 1) & ~1 = 2048; (16385, 65536):
    // 81952 / 32 = 2561, (2561 + 1) & ~1 = 2562
    uint64_t mo[3] = {7, 7, 7};
    EXPECT(swmi_banded_long_move_offsets(ok, zero, 2, mo) == SWMI_OK && mo[0] == 0 && mo[1] == 2048 && mo[2] == 2048 + 2562);
    EXPECT(swmi_banded_long_move_offsets(ok, over, 2, mo) == SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(std::strstr(swmi_banded_long_last_error(), "a length above 65536"));
    EXPECT(swmi_banded_long_move_offsets(ok, zero, 2, nullptr) == SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(swmi_banded_long_move_offsets(nullptr, zero, 2, mo) == SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(swmi_banded_long_move_offsets(ok, zero, 0, mo) == SWMI_OK && mo[0] == 0);
    // an aligning entry refuses the length before it touches a device, behind the band
    const int8_t sm[16] = {0};
    std::vector<uint8_t> bytes(8 + 65537, 1);
    int32_t out[16];
    EXPECT(swmi_banded_long_local(bytes.data(), over, bytes.data(), zero, 2, nullptr, 512, sm, 1, 1, out, out + 2, nullptr, nullptr) ==
           SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(std::strstr(swmi_banded_long_last_error(), "a length above 65536"));
    EXPECT(swmi_banded_long_local(bytes.data(), over, bytes.data(), zero, 2, nullptr, 192, sm, 1, 1, out, out + 2, nullptr, nullptr) ==
           SWMI_ERR_INVALID_ARGUMENT);
    EXPECT(std::strstr(swmi_banded_long_last_error(), "band 192"));
    EXPECT(g_launches == 0);
    std::printf("the length bound: %s\n", g_failed ? "FAILED" : "ok");
}

void the_key_by_hand()
{
    using swmi::banded::width_swept_rows;
    // global kind, 65536 x 65536, band 1024: worked out in rows_by_hand's comment
    EXPECT(width_swept_rows(1, 65536, 65536, 0, 1024) == 65536 && width_swept_rows(1, 65536, 65536, 300, 1024) == 65536);
    EXPECT(width_swept_rows(1, 65536, 65536, -1000, 1024) == 65536 - 489);       // rows 489 .. 65536
    EXPECT(width_swept_rows(1, 65536, 65536, 1000, 1024) == 65048);              // rows 0 .. 65536 + 512 - 1000
    EXPECT(width_swept_rows(1, 65536, 65536, 65536 + 511, 1024) == 1);           // rows 0 and 1: cell (0, 65535) ..
    EXPECT(width_swept_rows(1, 65536, 65536, 65536 + 512, 1024) == 0);           // row 0 alone: cell (0, 65536)
    EXPECT(width_swept_rows(1, 65536, 65536, 131072, 1024) == 0 && width_swept_rows(1, 65536, 65536, -131072, 1024) == 0);
    // local kind: interior rows 1 .. 65536; band 128 around diagonal 50: rows 1 .. 65536 + 64 - 50 capped at len1
    EXPECT(width_swept_rows(0, 65536, 65536, 0, 1024) == 65535 && width_swept_rows(0, 65536, 65536, 50, 128) == 65535);
    EXPECT(width_swept_rows(0, 65536, 100, -65436, 128) == 65536 - (2 - 64 + 65436));     // rows 65374 .. 65536
    EXPECT(width_swept_rows(0, 100, 65536, 65436, 128) == 99);
    std::printf("the key by hand: %s\n", g_failed ? "FAILED" : "ok");
}

void two_slices_by_the_byte_budget()
{
    std::vector<uint64_t> off(kN + 1);
    for (size_t k = 0; k <= kN; ++k) off[k] = k * kLen;
    std::vector<uint8_t> a(kN * kLen, 3), b(kN * kLen, 2);
    g_diag.assign(kN, 0);
    for (size_t c = 0; c < kN; ++c) {
        a[c * kLen] = uint8_t(c);
        b[c * kLen] = uint8_t(c + 1);
        g_diag[c] = int32_t(c % 11) * 97 - 400;
    }
    g_diag[3] = 65536 + 511;                  // reaches the launcher as it is
    g_diag[4] = -(65536 + 511);
    g_diag[5] = INT_MAX;                      // clamped to 131072
    g_diag[6] = INT_MIN;
    g_diag[7] = 131072;
    g_diag[8] = 131073;
    g_diag[130] = 65536 + 1;
    size_t sizes[4] = {0, 0, 0, 0};
    EXPECT(swmi_banded_long_slices_for(SWMI_BANDED_LONG_GLOBAL, 1024, off.data(), off.data(), kN, 1, sizes, 4) == 2);
    EXPECT(sizes[0] == kFirstSlice && sizes[1] == kN - kFirstSlice);
    constexpr size_t kGuard = 8;
    std::vector<int32_t> scores(kN + kGuard, -7), ends(4 * kN + kGuard, -7);
    std::vector<uint32_t> steps(kN + kGuard, 77u);
    std::vector<uint64_t> moves(kN * kMoveWords + kGuard, 0x5A5Aull);
    const int8_t sm[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    g_base = g_launches = 0;
    EXPECT(swmi_banded_long_global(a.data(), off.data(), b.data(), off.data(), kN, g_diag.data(), 1024, sm, 3, 1, 5u, scores.data(), ends.data(),
                                   moves.data(), steps.data()) == SWMI_OK);
    EXPECT(g_launches == 2 && g_base == kN);
    EXPECT(g_top_code == (kFirstSlice - 1) * kCodeBytes && g_top_code > (1ull << 32));        // 128 * 33 587 200 = 4 299 161 600
    for (size_t c = 0; c < kN; ++c) {
        EXPECT(scores[c] == 1000 + int32_t(c) && steps[c] == c % 7);
        for (int e = 0; e < 4; ++e) EXPECT(ends[4 * c + e] == clamped(g_diag[c]) + e);
        EXPECT(moves[c * kMoveWords] == (0xC0DEull << 48 | c) && moves[(c + 1) * kMoveWords - 1] == (0xBEEFull << 48 | c));
    }
    EXPECT(ends[4 * 3] == 66047 && ends[4 * 4] == -66047 && ends[4 * 5] == 131072 && ends[4 * 6] == -131072 && ends[4 * 8] == 131072);
    for (size_t g = 0; g < kGuard; ++g)
        EXPECT(scores[kN + g] == -7 && ends[4 * kN + g] == -7 && steps[kN + g] == 77u && moves[kN * kMoveWords + g] == 0x5A5Aull);
    std::printf("two slices by the byte budget: %s\n", g_failed ? "FAILED" : "ok");
}

}  // namespace

int main()
{
    the_length_bound();
    the_key_by_hand();
    two_slices_by_the_byte_budget();
    EXPECT(swmi_banded_long_release_workspaces() == SWMI_OK);
    if (g_failed) return 1;
    std::printf("banded long host fake ok\n");
    return 0;
}
