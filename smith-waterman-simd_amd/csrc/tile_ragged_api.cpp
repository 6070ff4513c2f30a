// tile_ragged_api.cpp -- C entries of the three kinds of any-length aligner on the wavefront-tiled sweep, on a batch of mixed
// (len1, len2): local (swmi_local_full[_affine]_ragged*), global / fit / overlap
// (swmi_global_full[_affine]_ragged*, section 22) and exact semi-global (swmi_semiglobal_full[_affine]_ragged*, section 27);
// include/swmi.h.  One row of data per kind (kKinds), one planner, one body for the checks and the call, and one explicit
// extern "C" definition per exported name.
//
// A batch becomes a TilePlan: a RaggedPlan (swmi_host.h) whose slices are cut in caller order within the fixed-length aligner's
// budget, with one TileWork per alignment and, per slice, where each wave count's slots start.  Inside a slice the slots are
// ordered by wave count descending (one launch serves one wave count), then len1 descending (the hardware starts workgroups
// in order, and longest first evens out the tail), then caller order.  The plan then runs through the slice pipeline of
// swmi_table.cpp, on the fixed-length entries' Table (table_api.cpp): their workspaces, their slice budgets, their ends per
// alignment and their count.  This file's name lies outside csrc/swmi_*.cpp for the reason table_api.cpp gives.
#include "swmi_host.h"

#include <algorithm>
#include <array>

namespace swmi {
namespace host {
namespace {

constexpr int kMaxWaves = 16;            // wave counts of a slot: 1 .. 16
constexpr size_t kMaxLen = 16384;        // the largest length of either sequence
static_assert(kMaxLen == SWMI_LOCAL_FULL_MAX_LEN && kMaxLen == SWMI_GLOBAL_FULL_MAX_LEN && kMaxLen == SWMI_SGFULL_MAX_LEN);
static_assert(SWMI_GLOBAL_FULL_MOVE_WORDS(5, 70) == SWMI_LOCAL_FULL_MOVE_WORDS(5, 70));   // one move layout for all three kinds
static_assert(SWMI_SGFULL_MOVE_WORDS(5, 70) == SWMI_LOCAL_FULL_MOVE_WORDS(5, 70));

struct TilePlan : RaggedPlan {
    bool affine = false;
    std::vector<TileWork> tiles;                                 // [n]: slice s's slots at [first[s], first[s + 1])
    // per slice: the slots of wave count W lie at [start[kMaxWaves - W], start[kMaxWaves - W + 1]) of the slice's slots
    std::vector<std::array<uint32_t, kMaxWaves + 1>> start;
};

// Calls fire(slots, count, waves) once per wave count present in slice `slice`, in descending wave count; the first error ends it
template <class Fire>
hipError_t for_each_wave_count(const Table &t, size_t slice, const void *work, size_t n, Fire fire)
{
    const TilePlan &p = *static_cast<const TilePlan *>(t.plan);
    const TileWork *slots = static_cast<const TileWork *>(work);
    const auto &start = p.start[slice];
    if (start[kMaxWaves] != n) return hipErrorInvalidValue;
    for (int waves = kMaxWaves; waves >= 1; --waves) {
        const uint32_t a = start[kMaxWaves - waves], b = start[kMaxWaves - waves + 1];
        if (a == b) continue;
        const hipError_t e = fire(p.affine, slots + a, size_t(b - a), waves);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- the launches of one slice, per kind: one per wave count present, on the one stream (the global kind: one mask for all) ----
#define SLICE_ARGS const Table &t, size_t slice, const uint8_t *s1, const uint8_t *s2, const void *work, size_t n, int32_t *scores, \
                   int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st

unsigned long long *qwords(uint32_t *codes) { return reinterpret_cast<unsigned long long *>(codes); }   // the affine launchers' unit

hipError_t launch_local_tiles(SLICE_ARGS)
{
    return for_each_wave_count(t, slice, work, n, [&](bool affine, const TileWork *slots, size_t m, int waves) {
        return affine ? swmi::launch_local_full_affine_ragged(s1, s2, slots, m, waves, t.sm, t.gap, t.gap_extend, scores, ends,
                                                              qwords(codes), moves, counts, st)
                      : swmi::launch_local_full_ragged(s1, s2, slots, m, waves, t.sm, t.gap, scores, ends, codes, moves, counts, st);
    });
}
hipError_t launch_global_tiles(SLICE_ARGS)
{
    return for_each_wave_count(t, slice, work, n, [&](bool affine, const TileWork *slots, size_t m, int waves) {
        return affine ? swmi::launch_global_full_affine_ragged(s1, s2, slots, m, waves, t.sm, t.gap, t.gap_extend, t.free_ends, scores,
                                                               ends, qwords(codes), moves, counts, st)
                      : swmi::launch_global_full_ragged(s1, s2, slots, m, waves, t.sm, t.gap, t.free_ends, scores, ends, codes, moves,
                                                        counts, st);
    });
}
hipError_t launch_semiglobal_tiles(SLICE_ARGS)
{
    return for_each_wave_count(t, slice, work, n, [&](bool affine, const TileWork *slots, size_t m, int waves) {
        return affine ? swmi::launch_sgfull_affine_ragged(s1, s2, slots, m, waves, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                                          moves, counts, st)
                      : swmi::launch_sgfull_ragged(s1, s2, slots, m, waves, t.sm, t.gap, scores, ends, codes, moves, counts, st);
    });
}
#undef SLICE_ARGS

// ---- the kinds ----
struct TileFamily {
    RaggedLaunch launch;                        // the launches of one slice
    int (*waves)(int len1, int len2);           // the wave count of a slot, 1 .. kMaxWaves
    size_t (*code_words[2])(int len1, int len2);    // of two non-zero lengths, in the kernel's unit: [0] linear, dwords; [1] affine, qwords
    TableFamily fixed[2];                       // the fixed-length family whose Table, workspaces and budget a batch takes: linear, affine
    bool mask;                                  // free_ends is read (and checked before everything else)
    const char *count;                          // the count array's name in the error text
};
constexpr TileFamily kKinds[kTileKinds] = {
    /* kTileLocal */
    {launch_local_tiles, swmi::local_full_ragged_waves, {swmi::local_full_code_words, swmi::local_full_affine_code_qwords},
     {kTableLocalFull, kTableLocalFullAffine}, false, "steps"},
    /* kTileGlobal */
    {launch_global_tiles, swmi::global_full_ragged_waves, {swmi::global_full_code_words, swmi::global_full_affine_code_qwords},
     {kTableGlobalFull, kTableGlobalFullAffine}, true, "steps"},
    /* kTileSemiglobal */
    {launch_semiglobal_tiles, swmi::sgfull_ragged_waves, {swmi::sgfull_code_words, swmi::sgfull_affine_code_qwords},
     {kTableSgfull, kTableSgfullAffine}, false, "lengths"},
};

// ---- the planner ----
// code words of one alignment in the kernel's unit; none when a length is 0 (nothing is swept)
size_t code_words(const TileFamily &f, bool affine, size_t len1, size_t len2)
{
    return len1 && len2 ? f.code_words[affine]((int)len1, (int)len2) : 0;
}

// device bytes one alignment of a ragged slice takes: inputs, its slot, results, and with a traceback codes, moves and count
// (five result dwords, where the semi-global kind writes three and with a traceback four: an upper bound, so a slice never
// outgrows the budget)
size_t ragged_bytes(const TileFamily &f, bool affine, bool tb, size_t len1, size_t len2)
{
    size_t b = len1 + len2 + sizeof(TileWork) + 5 * sizeof(int32_t);
    if (tb)
        b += code_words(f, affine, len1, len2) * (affine ? sizeof(uint64_t) : sizeof(uint32_t)) +
             SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

// the fixed-length aligner's budget for one slice's device buffers
size_t budget(const TileFamily &f, bool affine, bool tb)
{
    return tb ? family_table(f.fixed[affine], 1, 1, nullptr, 0, 0, 0).tb_slice_bytes : kTableSliceBytes;
}

int check_offsets(const char *name, const uint64_t *off, size_t n)
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

int check_both(const uint64_t *off1, const uint64_t *off2, size_t n)
{
    const int rc = check_offsets("seq1_offsets", off1, n);
    return rc != SWMI_OK ? rc : check_offsets("seq2_offsets", off2, n);
}

int check_affine_gaps(const int8_t *sm, int gap_open, int gap_extend)
{
    if (!sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (gap_open < 0 || gap_open > 127 || gap_extend < 0 || gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", gap_open, gap_extend);
    return SWMI_OK;
}

// Slices of checked offsets: each the longest run from where the last one ended whose ragged_bytes fit the budget, at most
// kTableMaxSlice alignments and at least one.  first = {0, ..., n}.
std::vector<size_t> cut(const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb)
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

// the body of a kind's *_slices_for entry
size_t slices_for(TileKind kind, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb, size_t *sizes, size_t cap)
{
    if (check_both(off1, off2, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(kKinds[kind], off1, off2, n, affine, tb);
    for (size_t s = 0; sizes && s + 1 < first.size() && s < cap; ++s) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

void fill_move_offsets(const uint64_t *off1, const uint64_t *off2, size_t n, uint64_t *out)
{
    out[0] = 0;
    for (size_t k = 0; k < n; ++k) out[k + 1] = out[k] + SWMI_LOCAL_FULL_MOVE_WORDS(off1[k + 1] - off1[k], off2[k + 1] - off2[k]);
}

// The plan of a checked batch.  Every TileWork offset and base is a 64-bit running sum relative to its slice (swmi_internal.h
// says why 32 bits would not do); code bases run in caller order, so a slice's codes are one block of code_words[s] dwords.
void make_plan(TilePlan &p, const TileFamily &f, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb)
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

// ---- one body for the host and the device entries of every kind ----
struct Params {
    const int8_t *sm;
    int gap, gap_extend;        // gap_extend 0 from the linear entries
    unsigned free_ends;         // 0 from the kinds without a mask
};

// The checks in the order of the fixed-length entries -- the mask, the matrix and the gaps, the moves / count pair; then n = 0,
// the buffers and the lengths, which here lie in the offsets -- and the call.
int ragged(TileKind kind, bool affine, bool device, const char *entry, const void *seq1s, const uint64_t *off1, const void *seq2s,
           const uint64_t *off2, size_t n, const Params &c, void *scores, void *ends, void *moves, void *counts, void *stream)
{
    const TileFamily &f = kKinds[kind];
    if (f.mask && c.free_ends > SWMI_ENDS_OVERLAP)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", c.free_ends, SWMI_ENDS_OVERLAP);
    int rc = affine ? check_affine_gaps(c.sm, c.gap, c.gap_extend) : check_params(c.sm, c.gap);
    if (rc != SWMI_OK) return rc;
    if (!moves != !counts)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and %s must both be given (traceback) or both be NULL (ends-only)", f.count);
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    rc = check_both(off1, off2, n);
    if (rc != SWMI_OK) return rc;
    TilePlan plan;
    make_plan(plan, f, off1, off2, n, affine, moves != nullptr);
    Table t = family_table(f.fixed[affine], 1, 1, c.sm, c.gap, c.gap_extend, c.free_ends);
    t.plan = &plan;
    if (device) return table_device(t, seq1s, seq2s, n, scores, ends, moves, counts, stream);
    return table_host(t, entry, static_cast<const uint8_t *>(seq1s), static_cast<const uint8_t *>(seq2s), n,
                      static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(counts));
}

}  // namespace

// The plan alone, for a test of its arithmetic at sizes no test can allocate: per slice its alignments and device bytes, and
// whether every code base equals the 64-bit running sum of the code words before it.  Not part of the C ABI.
bool tile_ragged_plan_check(TileKind kind, const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb,
                            std::vector<size_t> *slice_sizes, std::vector<size_t> *slice_bytes)
{
    const TileFamily &f = kKinds[kind];
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

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

// ---- local, mixed shapes (section 19) ----
int swmi_local_full_ragged_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, uint64_t *move_offsets)
{
    if (!move_offsets) return fail(SWMI_ERR_INVALID_ARGUMENT, "move_offsets is NULL");
    const int rc = check_both(seq1_offsets, seq2_offsets, n);
    if (rc != SWMI_OK) return rc;
    fill_move_offsets(seq1_offsets, seq2_offsets, n, move_offsets);
    return SWMI_OK;
}

size_t swmi_local_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                         int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTileLocal, seq1_offsets, seq2_offsets, n, affine != 0, traceback != 0, sizes, cap);
}

int swmi_local_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                           size_t n, const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                           uint64_t *moves, uint32_t *steps)
{
    return ragged(kTileLocal, false, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, {score_matrix, gap_penalty, 0, 0},
                  scores, ends, moves, steps, nullptr);
}

int swmi_local_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                                  size_t n, const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                  void *d_moves, void *d_steps, void *stream)
{
    return ragged(kTileLocal, false, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, {score_matrix, gap_penalty, 0, 0},
                  d_scores, d_ends, d_moves, d_steps, stream);
}

int swmi_local_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                  const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                  int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return ragged(kTileLocal, true, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, {score_matrix, gap_open, gap_extend, 0},
                  scores, ends, moves, steps, nullptr);
}

int swmi_local_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                         const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                         int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return ragged(kTileLocal, true, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                  {score_matrix, gap_open, gap_extend, 0}, d_scores, d_ends, d_moves, d_steps, stream);
}

// ---- global / fit / overlap, mixed shapes (section 22) ----
size_t swmi_global_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                          int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTileGlobal, seq1_offsets, seq2_offsets, n, affine != 0, traceback != 0, sizes, cap);
}

int swmi_global_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                            size_t n, const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, int32_t *scores,
                            int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return ragged(kTileGlobal, false, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n,
                  {score_matrix, gap_penalty, 0, free_ends}, scores, ends, moves, steps, nullptr);
}

int swmi_global_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, const uint64_t *seq2_offsets,
                                   size_t n, const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores,
                                   void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return ragged(kTileGlobal, false, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                  {score_matrix, gap_penalty, 0, free_ends}, d_scores, d_ends, d_moves, d_steps, stream);
}

int swmi_global_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                   const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                   unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return ragged(kTileGlobal, true, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n,
                  {score_matrix, gap_open, gap_extend, free_ends}, scores, ends, moves, steps, nullptr);
}

int swmi_global_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                          const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                          int gap_extend, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves,
                                          void *d_steps, void *stream)
{
    return ragged(kTileGlobal, true, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                  {score_matrix, gap_open, gap_extend, free_ends}, d_scores, d_ends, d_moves, d_steps, stream);
}

// ---- exact semi-global, mixed shapes (section 27) ----
size_t swmi_semiglobal_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                              int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTileSemiglobal, seq1_offsets, seq2_offsets, n, affine != 0, traceback != 0, sizes, cap);
}

int swmi_semiglobal_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                size_t n, const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return ragged(kTileSemiglobal, false, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, {score_matrix, gap_penalty, 0, 0},
                  scores, ends, moves, lengths, nullptr);
}

int swmi_semiglobal_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                       const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                                       void *d_scores, void *d_ends, void *d_moves, void *d_lengths, void *stream)
{
    return ragged(kTileSemiglobal, false, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                  {score_matrix, gap_penalty, 0, 0}, d_scores, d_ends, d_moves, d_lengths, stream);
}

int swmi_semiglobal_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                       const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                       int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths)
{
    return ragged(kTileSemiglobal, true, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n,
                  {score_matrix, gap_open, gap_extend, 0}, scores, ends, moves, lengths, nullptr);
}

int swmi_semiglobal_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                              const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                              int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_lengths,
                                              void *stream)
{
    return ragged(kTileSemiglobal, true, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n,
                  {score_matrix, gap_open, gap_extend, 0}, d_scores, d_ends, d_moves, d_lengths, stream);
}

}  // extern "C"
