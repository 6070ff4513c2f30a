// tile_ragged_plan.h -- the plan of a batch of mixed (len1, len2) for the any-length aligners on the wavefront-tiled sweep:
// what local_full_ragged_api.cpp, global_full_ragged_api.cpp (section 22) and sgfull_ragged_api.cpp
// (section 27) share.  A batch becomes a
// TilePlan: a RaggedPlan (swmi_host.h) whose slices are cut in caller order within the fixed-length aligner's budget, with one
// TileWork per alignment and, per slice, where each wave count's slots start.  Inside a slice the slots are ordered by wave
// count descending (one launch serves one wave count), then len1 descending (the hardware starts workgroups in order, and
// longest first evens out the tail), then caller order.  The plan then runs through the slice pipeline of swmi_table.cpp.
//
// A header and not a source file on purpose: the fake-GPU tests link an exact list of sources, and this one names no
// launcher.  What differs between the three families -- the launchers, the wave count of a slot, the code words of an
// alignment and the slice budget -- reaches the planner as a TileFamily of function pointers that each family's file fills.
#pragma once
#include "swmi_host.h"

#include <algorithm>
#include <array>

namespace swmi {
namespace host {
namespace tile_plan {

constexpr int kMaxWaves = 16;            // wave counts of a slot: 1 .. 16
constexpr size_t kMaxLen = 16384;        // the largest length of either sequence
static_assert(kMaxLen == SWMI_LOCAL_FULL_MAX_LEN && kMaxLen == SWMI_GLOBAL_FULL_MAX_LEN && kMaxLen == SWMI_SGFULL_MAX_LEN);
static_assert(SWMI_GLOBAL_FULL_MOVE_WORDS(5, 70) == SWMI_LOCAL_FULL_MOVE_WORDS(5, 70));   // one move layout for all three families
static_assert(SWMI_SGFULL_MOVE_WORDS(5, 70) == SWMI_LOCAL_FULL_MOVE_WORDS(5, 70));

struct TileFamily {
    RaggedLaunch launch;                                         // the launches of one slice
    int (*waves)(int len1, int len2);                            // the wave count of a slot, 1 .. kMaxWaves
    size_t (*code_words)(bool affine, int len1, int len2);       // of two non-zero lengths, in the kernel's unit (dwords; affine: qwords)
    size_t (*tb_slice_bytes)(bool affine);                       // the fixed-length aligner's budget for a traceback slice
};

struct TilePlan : RaggedPlan {
    bool affine = false;
    std::vector<TileWork> tiles;                                 // [n]: slice s's slots at [first[s], first[s + 1])
    // per slice: the slots of wave count W lie at [start[kMaxWaves - W], start[kMaxWaves - W + 1]) of the slice's slots
    std::vector<std::array<uint32_t, kMaxWaves + 1>> start;
};

// Calls fire(slots, count, waves) once per wave count present in slice `slice`, in descending wave count; the first error ends it
template <class Fire>
hipError_t for_each_wave_count(const TilePlan &p, size_t slice, const void *work, size_t n, Fire fire)
{
    const TileWork *slots = static_cast<const TileWork *>(work);
    const auto &start = p.start[slice];
    if (start[kMaxWaves] != n) return hipErrorInvalidValue;
    for (int waves = kMaxWaves; waves >= 1; --waves) {
        const uint32_t a = start[kMaxWaves - waves], b = start[kMaxWaves - waves + 1];
        if (a == b) continue;
        const hipError_t e = fire(slots + a, size_t(b - a), waves);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// code words of one alignment in the kernel's unit; none when a length is 0 (nothing is swept)
inline size_t code_words(const TileFamily &f, bool affine, size_t len1, size_t len2)
{
    return len1 && len2 ? f.code_words(affine, (int)len1, (int)len2) : 0;
}

// device bytes one alignment of a ragged slice takes: inputs, its slot, results, and with a traceback codes, moves and count
inline size_t ragged_bytes(const TileFamily &f, bool affine, bool tb, size_t len1, size_t len2)
{
    size_t b = len1 + len2 + sizeof(TileWork) + 5 * sizeof(int32_t);
    if (tb)
        b += code_words(f, affine, len1, len2) * (affine ? sizeof(uint64_t) : sizeof(uint32_t)) +
             SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

// the fixed-length aligner's budget for one slice's device buffers
inline size_t budget(const TileFamily &f, bool affine, bool tb) { return tb ? f.tb_slice_bytes(affine) : kTableSliceBytes; }

inline int check_offsets(const char *name, const uint64_t *off, size_t n)
{
    if (!off) return fail(SWMI_ERR_INVALID_ARGUMENT, "%s is NULL", name);
    for (size_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return fail(SWMI_ERR_INVALID_ARGUMENT, "%s decrease at %zu", name, k);
        if (off[k + 1] - off[k] > kMaxLen)
            return fail(SWMI_ERR_INVALID_ARGUMENT, "%s: sequence %zu has length %llu > %zu", name, k,
                        (unsigned long long)(off[k + 1] - off[k]), kMaxLen);
    }
    return SWMI_OK;
}

inline int check_both(const uint64_t *off1, const uint64_t *off2, size_t n)
{
    const int rc = check_offsets("seq1_offsets", off1, n);
    return rc != SWMI_OK ? rc : check_offsets("seq2_offsets", off2, n);
}

inline int check_affine_gaps(const int8_t *sm, int gap_open, int gap_extend)
{
    if (!sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (gap_open < 0 || gap_open > 127 || gap_extend < 0 || gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", gap_open, gap_extend);
    return SWMI_OK;
}

// Slices of checked offsets: each the longest run from where the last one ended whose ragged_bytes fit the budget, at most
// kTableMaxSlice alignments and at least one.  first = {0, ..., n}.
inline std::vector<size_t> cut(const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb)
{
    const size_t cap = budget(f, affine, tb);
    std::vector<size_t> first{0};
    size_t bytes = 0, m = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t b = ragged_bytes(f, affine, tb, size_t(off1[k + 1] - off1[k]), size_t(off2[k + 1] - off2[k]));
        if (m && (bytes + b > cap || m == kTableMaxSlice)) {
            first.push_back(k);
            bytes = m = 0;
        }
        bytes += b;
        ++m;
    }
    if (n) first.push_back(n);
    return first;
}

// the body of a family's *_slices_for entry
inline size_t slices_for(const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb, size_t *sizes,
                         size_t cap)
{
    if (check_both(off1, off2, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(f, off1, off2, n, affine, tb);
    for (size_t s = 0; sizes && s + 1 < first.size() && s < cap; ++s) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

inline void fill_move_offsets(const uint64_t *off1, const uint64_t *off2, size_t n, uint64_t *out)
{
    out[0] = 0;
    for (size_t k = 0; k < n; ++k) out[k + 1] = out[k] + SWMI_LOCAL_FULL_MOVE_WORDS(off1[k + 1] - off1[k], off2[k + 1] - off2[k]);
}

// The plan of a checked batch.  Every TileWork offset and base is a 64-bit running sum relative to its slice (swmi_internal.h
// says why 32 bits would not do); code bases run in caller order, so a slice's codes are one block of code_words[s] dwords.
inline void make_plan(TilePlan &p, const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb)
{
    p.launch = f.launch;
    p.affine = affine;
    p.seq1_offsets = off1;
    p.seq2_offsets = off2;
    p.move_offsets.resize(n + 1);
    fill_move_offsets(off1, off2, n, p.move_offsets.data());
    p.first = cut(f, off1, off2, n, affine, tb);
    p.tiles.resize(n);
    p.slots = p.tiles.data();
    p.slot_bytes = sizeof(TileWork);
    const size_t slices = p.first.size() - 1;
    p.code_words.assign(slices, 0);
    p.start.resize(slices);
    // counting sort on (wave count, len1), both descending, equal keys in caller order: bucket = (16 - W) * 16385 + (16384 - len1)
    constexpr size_t kLens = kMaxLen + 1;
    std::vector<uint32_t> at(kMaxWaves * kLens + 1);
    for (size_t s = 0; s < slices; ++s) {
        const size_t a = p.first[s], b = p.first[s + 1];
        auto bucket = [&](size_t k) {
            const int len1 = int(off1[k + 1] - off1[k]), len2 = int(off2[k + 1] - off2[k]);
            return size_t(kMaxWaves - f.waves(len1, len2)) * kLens + (kMaxLen - size_t(len1));
        };
        std::fill(at.begin(), at.end(), 0u);
        for (size_t k = a; k < b; ++k) ++at[bucket(k) + 1];
        for (size_t x = 1; x < at.size(); ++x) at[x] += at[x - 1];
        for (int j = 0; j <= kMaxWaves; ++j) p.start[s][j] = at[size_t(j) * kLens];
        uint64_t codes = 0;
        for (size_t k = a; k < b; ++k) {
            const uint32_t len1 = uint32_t(off1[k + 1] - off1[k]), len2 = uint32_t(off2[k + 1] - off2[k]);
            p.tiles[a + at[bucket(k)]++] = {off1[k] - off1[a], off2[k] - off2[a], codes, p.move_offsets[k] - p.move_offsets[a],
                                            uint32_t(k - a), len1, len2, 0};
            if (tb) codes += code_words(f, affine, len1, len2);
        }
        p.code_words[s] = size_t(codes) * (affine ? 2 : 1);
        p.max_m = std::max(p.max_m, b - a);
        p.max_seq1 = std::max(p.max_seq1, size_t(off1[b] - off1[a]));
        p.max_seq2 = std::max(p.max_seq2, size_t(off2[b] - off2[a]));
        p.max_codes = std::max(p.max_codes, p.code_words[s]);
        p.max_moves = std::max(p.max_moves, size_t(p.move_offsets[b] - p.move_offsets[a]));
    }
}

// The plan alone, for a test of its arithmetic at sizes no test can allocate: per slice its alignments and device bytes, and
// whether every code base equals the 64-bit running sum of the code words before it.
inline bool plan_check(const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb,
                       std::vector<size_t> *slice_sizes, std::vector<size_t> *slice_bytes)
{
    TilePlan p;
    make_plan(p, f, off1, off2, n, affine, tb);
    bool ok = true;
    for (size_t s = 0; s + 1 < p.first.size(); ++s) {
        const size_t a = p.first[s], b = p.first[s + 1];
        std::vector<uint64_t> base(b - a);
        size_t bytes = 0;
        uint64_t codes = 0;
        for (size_t k = a; k < b; ++k) {
            const size_t len1 = size_t(off1[k + 1] - off1[k]), len2 = size_t(off2[k + 1] - off2[k]);
            base[k - a] = codes;
            if (tb) codes += code_words(f, affine, len1, len2);
            bytes += ragged_bytes(f, affine, tb, len1, len2);
        }
        for (size_t x = a; x < b; ++x) ok = ok && p.tiles[x].k < b - a && p.tiles[x].code_base == base[p.tiles[x].k];
        ok = ok && p.code_words[s] == codes * (affine ? 2 : 1);
        slice_sizes->push_back(b - a);
        slice_bytes->push_back(bytes);
    }
    return ok;
}

}  // namespace tile_plan
}  // namespace host
}  // namespace swmi
