// table_api.cpp -- C entries of the fourteen fixed-shape aligners that run through the slice pipeline of swmi_table.cpp (struct
// Table, swmi_host.h; include/swmi.h, DESIGN.md sections 12 to 14, 16 to 18, 20, 21, 23, 25 and 26): one row of data per family
// (kRows, in the order of TableFamily), one body for the argument check, the Table and each of the five kinds of entry, and
// one explicit extern "C" definition per exported name.  Everything but family_table, which the mixed-shape entries
// (local_ragged_api.cpp, tile_ragged_api.cpp) call for a fixed-length family's Table, is private to this file.  Its name lies
// outside csrc/swmi_*.cpp, so that the host-only builds of swmi_api.cpp + swmi_multi.cpp stay free of the table kernels.
#include "swmi_host.h"

#include <algorithm>
#include <cstdlib>

namespace swmi {
namespace host {
namespace {

// columns of one stripe = what the fixed-length kernels of all three striped kinds reach
constexpr size_t kStripe = SWMI_GLOBAL_FULL_MAX_LEN;
static_assert(kStripe == SWMI_LOCAL_FULL_MAX_LEN && kStripe == SWMI_SGFULL_MAX_LEN);

// ---- how a slice of each family launches ----
#define SLICE_ARGS const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends, uint32_t *codes, \
                   unsigned long long *moves, uint32_t *counts, hipStream_t st

unsigned long long *qwords(uint32_t *codes) { return reinterpret_cast<unsigned long long *>(codes); }   // the affine launchers' unit

hipError_t launch_local_slice(SLICE_ARGS)
{
    return swmi::launch_local(s1, s2, (int)t.len1, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words, st);
}
hipError_t launch_sgfull_slice(SLICE_ARGS)
{
    return swmi::launch_sgfull(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words, st);
}
hipError_t launch_local_affine_slice(SLICE_ARGS)
{
    return swmi::launch_local_affine(s1, s2, (int)t.len1, n, t.sm, t.gap, t.gap_extend, scores, ends, codes, moves, counts,
                                     t.move_words, st);
}
hipError_t launch_sgfull_affine_slice(SLICE_ARGS)
{
    return swmi::launch_sgfull_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                      moves, counts, t.move_words, st);
}
hipError_t launch_local_full_slice(SLICE_ARGS)
{
    return swmi::launch_local_full(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                   st);
}
hipError_t launch_local_full_affine_slice(SLICE_ARGS)
{
    return swmi::launch_local_full_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                          moves, counts, t.move_words, st);
}
hipError_t launch_global_full_slice(SLICE_ARGS)
{
    return swmi::launch_global_full(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.free_ends, scores, ends, codes, moves, counts,
                                    t.move_words, st);
}
hipError_t launch_global_full_affine_slice(SLICE_ARGS)
{
    return swmi::launch_global_full_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, t.free_ends, scores, ends,
                                           qwords(codes), moves, counts, t.move_words, st);
}
// The six striped families: a shape that the fixed-length kernel reaches goes to it, and every field is then the fixed-length
// entry's by construction.
bool fits_stripe(const Table &t) { return t.len1 <= kStripe && t.len2 <= kStripe; }
hipError_t launch_global_long_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_global_full_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_global_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.free_ends, scores, ends, codes, moves, counts,
                                    t.move_words, t.carry, st);
}
hipError_t launch_global_long_affine_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_global_full_affine_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_global_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, t.free_ends, scores, ends,
                                           qwords(codes), moves, counts, t.move_words, t.carry, st);
}
hipError_t launch_local_long_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_local_full_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_local_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                   t.carry, st);
}
hipError_t launch_local_long_affine_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_local_full_affine_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_local_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                          moves, counts, t.move_words, t.carry, st);
}
hipError_t launch_semiglobal_long_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_sgfull_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_sgfull_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                    t.carry, st);
}
hipError_t launch_semiglobal_long_affine_slice(SLICE_ARGS)
{
    if (fits_stripe(t)) return launch_sgfull_affine_slice(t, s1, s2, n, scores, ends, codes, moves, counts, st);
    return swmi::launch_sgfull_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                           moves, counts, t.move_words, t.carry, st);
}
#undef SLICE_ARGS

// ---- the families ----
// What differs between the aligners.  Code sizes are in the Table's unit, dwords: twice the affine launchers' qwords.
struct FamilyRow {
    TableLaunch launch;
    TableFamily family;         // Table::state: whose device buffers a call uses; the row's own index in kRows
    size_t max_len;             // per axis
    bool fixed_len2;            // len2 is SWMI_LOCAL_SEQ2_LEN, whatever the caller's
    const char *count;          // Table::count, and
    uint32_t count_offset;      //   Table::count_offset
    size_t ends;                // int32 of `ends` per alignment
    size_t (*code_words)(size_t len1, size_t len2);
    size_t (*move_words)(size_t len1, size_t len2);
    // A traceback slice holds as many alignments as `budget` of `budget_as`'s maximum shape (0: kTableSliceBytes).  256 of
    // 16384 x 16384 (16.1 GiB of 2-bit codes, 32.1 GiB of 4-bit ones) are one workgroup per alignment for every CU of an
    // MI355X; 4096 of len1 = 16384 (4.1 GiB) give every CU a workgroup of 16 alignments.  A striped pair takes its
    // fixed-length pair's budget, and counts its carry in a slice: on a shape that both reach the code sizes are equal
    // (tile::code_words), so the slices are the fixed-length entries'.
    size_t budget;
    TableFamily budget_as;
    bool affine;                // gap_extend is read; gaps within [0, 127] instead of check_params
    bool mask;                  // free_ends is read
    bool carry;                 // column stripes: a carry of len1 dwords (affine: 2 len1) per alignment where len2 > 16384
    bool domain;                // the unfloored striped aligners' domain rule, P (len1 + len2) <= 2^23 (include/swmi.h); the long
                                //   local pair has none: 0 <= H < 2^23 whatever the parameters (local_long_kernels.hip)
    bool timer_first;           // the timer checks its own arguments (and binds the context) before the call's
    bool timer_pair;            // the timer refuses a traceback given by half where the host and device entries do: behind the
                                //   call's check and before a device is looked for (the others leave it to table_time_device)
};
constexpr FamilyRow kRows[] = {
    /* kTableLocal */
    {launch_local_slice, kTableLocal, SWMI_LOCAL_MAX_LEN, true, "steps", 0, 4, [](size_t a, size_t) { return swmi::local_code_words((int)a); },
     [](size_t a, size_t) { return size_t(SWMI_LOCAL_MOVE_WORDS(a)); }, 0, kTableLocal, false, false, false, false, true, false},
    /* kTableSgfull */
    {launch_sgfull_slice, kTableSgfull, SWMI_SGFULL_MAX_LEN, false, "lengths", 1, 2,
     [](size_t a, size_t b) { return swmi::sgfull_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_SGFULL_MOVE_WORDS(a, b)); }, 256, kTableSgfull, false, false, false, false, true, false},
    /* kTableLocalAffine */
    {launch_local_affine_slice, kTableLocalAffine, SWMI_LOCAL_MAX_LEN, true, "steps", 0, 4,
     [](size_t a, size_t) { return swmi::local_affine_code_words((int)a); },
     [](size_t a, size_t) { return size_t(SWMI_LOCAL_MOVE_WORDS(a)); }, 4096, kTableLocalAffine, true, false, false, false, true, false},
    /* kTableSgfullAffine */
    {launch_sgfull_affine_slice, kTableSgfullAffine, SWMI_SGFULL_MAX_LEN, false, "lengths", 1, 2,
     [](size_t a, size_t b) { return 2 * swmi::sgfull_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_SGFULL_MOVE_WORDS(a, b)); }, 256, kTableSgfullAffine, true, false, false, false, false,
     false},
    /* kTableLocalFull */
    {launch_local_full_slice, kTableLocalFull, SWMI_LOCAL_FULL_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return swmi::local_full_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_LOCAL_FULL_MOVE_WORDS(a, b)); }, 256, kTableLocalFull, false, false, false, false, false,
     false},
    /* kTableLocalFullAffine */
    {launch_local_full_affine_slice, kTableLocalFullAffine, SWMI_LOCAL_FULL_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return 2 * swmi::local_full_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_LOCAL_FULL_MOVE_WORDS(a, b)); }, 256, kTableLocalFullAffine, true, false, false, false,
     false, false},
    /* kTableGlobalFull */
    {launch_global_full_slice, kTableGlobalFull, SWMI_GLOBAL_FULL_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return swmi::global_full_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_GLOBAL_FULL_MOVE_WORDS(a, b)); }, 256, kTableGlobalFull, false, true, false, false, false,
     false},
    /* kTableGlobalFullAffine */
    {launch_global_full_affine_slice, kTableGlobalFullAffine, SWMI_GLOBAL_FULL_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return 2 * swmi::global_full_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_GLOBAL_FULL_MOVE_WORDS(a, b)); }, 256, kTableGlobalFullAffine, true, true, false, false,
     false, false},
    /* kTableGlobalLong */
    {launch_global_long_slice, kTableGlobalLong, SWMI_GLOBAL_LONG_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return swmi::global_long_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_GLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableGlobalFull, false, true, true, true, false,
     false},
    /* kTableGlobalLongAffine */
    {launch_global_long_affine_slice, kTableGlobalLongAffine, SWMI_GLOBAL_LONG_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return 2 * swmi::global_long_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_GLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableGlobalFullAffine, true, true, true, true,
     false, false},
    /* kTableLocalLong */
    {launch_local_long_slice, kTableLocalLong, SWMI_LOCAL_LONG_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return swmi::local_long_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_LOCAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableLocalFull, false, false, true, false, false,
     false},
    /* kTableLocalLongAffine */
    {launch_local_long_affine_slice, kTableLocalLongAffine, SWMI_LOCAL_LONG_MAX_LEN, false, "steps", 0, 4,
     [](size_t a, size_t b) { return 2 * swmi::local_long_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_LOCAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableLocalFullAffine, true, false, true, false,
     false, false},
    /* kTableSemiglobalLong */
    {launch_semiglobal_long_slice, kTableSemiglobalLong, SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, "lengths", 1, 2,
     [](size_t a, size_t b) { return swmi::sgfull_long_code_words((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableSgfull, false, false, true, true, false,
     true},
    /* kTableSemiglobalLongAffine */
    {launch_semiglobal_long_affine_slice, kTableSemiglobalLongAffine, SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, "lengths", 1, 2,
     [](size_t a, size_t b) { return 2 * swmi::sgfull_long_affine_code_qwords((int)a, (int)b); },
     [](size_t a, size_t b) { return size_t(SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableSgfullAffine, true, false, true, true,
     false, true},
};
constexpr bool rows_in_enum_order()
{
    for (int f = 0; f < kTableFamilies; ++f)
        if (kRows[f].family != f) return false;
    return true;
}
static_assert(sizeof kRows / sizeof kRows[0] == kTableFamilies && rows_in_enum_order(), "kRows[f] is the row of TableFamily f");

// the arguments of one call that the families read
struct Call {
    size_t len1, len2;          // len2 = SWMI_LOCAL_SEQ2_LEN from the two local families' entries
    const int8_t *sm;
    int gap, gap_extend;        // gap_extend 0 from the linear families' entries
    unsigned free_ends;         // 0 from the families without a mask
};

// ---- one body each ----
bool lens_ok(const FamilyRow &r, size_t len1, size_t len2)
{
    return len1 >= 1 && len1 <= r.max_len && (r.fixed_len2 || (len2 >= 1 && len2 <= r.max_len));
}

// the striped aligners' domain rule (include/swmi.h): P (len1 + len2) <= 2^23 with P = max(1, max |sm|, gaps...)
bool domain_ok(const Call &c)
{
    size_t p = 1;
    for (int x = 0; x < 16; ++x) p = std::max(p, (size_t)std::abs((int)c.sm[x]));
    p = std::max(p, (size_t)std::abs(c.gap));
    p = std::max(p, (size_t)std::abs(c.gap_extend));
    return p * (c.len1 + c.len2) <= (size_t(1) << 23);
}

// in the order include/swmi.h gives: the lengths, the mask, the matrix and the gaps, the domain rule
int check(const FamilyRow &r, const Call &c)
{
    if (!lens_ok(r, c.len1, c.len2)) {
        if (r.fixed_len2) return fail(SWMI_ERR_INVALID_ARGUMENT, "len1 %zu outside [1, %zu]", c.len1, r.max_len);
        return fail(SWMI_ERR_INVALID_ARGUMENT, "lengths (%zu, %zu) outside [1, %zu]", c.len1, c.len2, r.max_len);
    }
    if (r.mask && c.free_ends > SWMI_ENDS_OVERLAP)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", c.free_ends, SWMI_ENDS_OVERLAP);
    if (!r.affine) {
        const int rc = check_params(c.sm, c.gap);
        if (rc != SWMI_OK) return rc;
    } else {
        if (!c.sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
        if (c.gap < 0 || c.gap > 127 || c.gap_extend < 0 || c.gap_extend > 127)
            return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", c.gap, c.gap_extend);
    }
    if (r.domain && !domain_ok(c)) {
        if (r.affine)
            return fail(SWMI_ERR_INVALID_ARGUMENT, "max(1, |score|, gap_open, gap_extend) * (len1 + len2) = P * %zu above 2^23",
                        c.len1 + c.len2);
        return fail(SWMI_ERR_INVALID_ARGUMENT, "max(1, |score|, gap) * (len1 + len2) = P * %zu above 2^23", c.len1 + c.len2);
    }
    return SWMI_OK;
}

Table call_table(TableFamily f, const Call &c) { return family_table(f, c.len1, c.len2, c.sm, c.gap, c.gap_extend, c.free_ends); }

size_t slices_for(TableFamily f, size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!lens_ok(kRows[f], len1, len2)) return 0;
    return table_slices_for(family_table(f, len1, len2, nullptr, 0, 0, 0), n, traceback != 0, sizes, cap);
}

int device(TableFamily f, const Call &c, const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores, void *d_ends, void *d_moves,
           void *d_counts, void *stream)
{
    const int rc = check(kRows[f], c);
    if (rc != SWMI_OK) return rc;
    return table_device(call_table(f, c), d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_counts, stream);
}

int host(TableFamily f, const char *entry, const Call &c, const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int32_t *scores,
         int32_t *ends, uint64_t *moves, uint32_t *counts)
{
    const int rc = check(kRows[f], c);
    if (rc != SWMI_OK) return rc;
    return table_host(call_table(f, c), entry, seq1s, seq2s, n, scores, ends, moves, counts);
}

int time_device(TableFamily f, const char *entry, const Call &c, const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores,
                void *d_ends, void *d_moves, void *d_counts, void *stream, int iters, float *avg_ms)
{
    const FamilyRow &r = kRows[f];
    int rc = r.timer_first ? table_check_timer(n, iters, avg_ms) : SWMI_OK;       // (its last check makes the context current)
    if (rc == SWMI_OK) rc = check(r, c);
    if (rc == SWMI_OK && r.timer_pair && !d_moves != !d_counts)
        rc = fail(SWMI_ERR_INVALID_ARGUMENT, "moves and %s must both be given (traceback) or both be NULL (ends-only)", r.count);
    if (rc == SWMI_OK && !r.timer_first) rc = table_check_timer(n, iters, avg_ms);
    if (rc != SWMI_OK) return rc;
    return table_time_device(call_table(f, c), entry, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_counts, stream, iters, avg_ms);
}

// The reference's list (source.cpp:1571-1572: from the start cell to the end cell) from the walk's moves, for end cells up to
// (max_i, max_j): the start cell is the end cell less the moves' row / column steps, and the list applies the moves last to first.
int expand_moves(int32_t max_i, int32_t max_j, const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                 size_t cap)
{
    if ((!moves && steps) || (!positions && cap)) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (end_i < 0 || end_j < 0 || end_i > max_i || end_j > max_j)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "end cell (%d, %d) outside the matrix", end_i, end_j);
    if (steps > (uint32_t)end_i + (uint32_t)end_j)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "%u steps cannot start inside the matrix from (%d, %d)", steps, end_i, end_j);
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

}  // namespace

// The Table of one call of a family, from its row (swmi_host.h)
Table family_table(TableFamily f, size_t len1, size_t len2, const int8_t *sm, int gap, int gap_extend, unsigned free_ends)
{
    const FamilyRow &r = kRows[f], &b = kRows[r.budget_as];
    Table t{r.launch, r.family, kTableSliceBytes, r.count, len1, len2, r.ends, r.code_words(len1, len2), r.move_words(len1, len2),
            r.count_offset, sm, gap, gap_extend};
    t.free_ends = free_ends;
    if (r.budget) {
        Table full = t;
        full.len1 = b.max_len;
        full.len2 = b.fixed_len2 ? len2 : b.max_len;
        full.code_words = b.code_words(full.len1, full.len2);
        full.move_words = b.move_words(full.len1, full.len2);
        t.tb_slice_bytes = r.budget * table_slice_bytes(full, true);
    }
    if (r.carry && len2 > kStripe) t.carry_words = r.affine ? 2 * len1 : len1;       // a row of H, or of (H, F)
    return t;
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

// ---- local (section 12) ----
size_t swmi_local_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocal, n, len1, SWMI_LOCAL_SEQ2_LEN, traceback, sizes, cap);
}

int swmi_local_align_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                            int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return device(kTableLocal, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                  d_steps, stream);
}

int swmi_local_align(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocal, __func__, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves,
                steps);
}

int swmi_local_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                           int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                           float *avg_ms)
{
    return time_device(kTableLocal, __func__, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores,
                       d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

int swmi_local_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return expand_moves(SWMI_LOCAL_MAX_LEN, SWMI_LOCAL_SEQ2_LEN, moves, steps, end_i, end_j, positions, cap);
}

// ---- exact semi-global (section 13) ----
size_t swmi_semiglobal_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableSgfull, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_lengths, void *stream)
{
    return device(kTableSgfull, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_lengths,
                  stream);
}

int swmi_semiglobal_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                         const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves,
                         uint32_t *lengths)
{
    return host(kTableSgfull, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves, lengths);
}

int swmi_semiglobal_full_release_workspaces(void) { return table_release_workspaces(kTableSgfull); }

int swmi_semiglobal_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                     void *d_lengths, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableSgfull, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                       d_moves, d_lengths, stream, iters, avg_ms);
}

// ---- local with affine gaps (section 14) ----
size_t swmi_local_affine_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocalAffine, n, len1, SWMI_LOCAL_SEQ2_LEN, traceback, sizes, cap);
}

int swmi_local_align_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                                   int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                   void *stream)
{
    return device(kTableLocalAffine, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores,
                  d_ends, d_moves, d_steps, stream);
}

int swmi_local_align_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                            int gap_open, int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocalAffine, __func__, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores,
                ends, moves, steps);
}

int swmi_local_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                                  int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                  void *stream, int iters, float *avg_ms)
{
    return time_device(kTableLocalAffine, __func__, {len1, SWMI_LOCAL_SEQ2_LEN, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s,
                       n, d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- exact semi-global with affine gaps (section 16) ----
size_t swmi_semiglobal_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableSgfullAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_lengths, void *stream)
{
    return device(kTableSgfullAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                  d_moves, d_lengths, stream);
}

int swmi_semiglobal_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return host(kTableSgfullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores, ends, moves,
                lengths);
}

int swmi_semiglobal_full_affine_release_workspaces(void) { return table_release_workspaces(kTableSgfullAffine); }

int swmi_semiglobal_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                            void *d_ends, void *d_moves, void *d_lengths, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableSgfullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores,
                       d_ends, d_moves, d_lengths, stream, iters, avg_ms);
}

// ---- local, any two lengths (section 17) ----
size_t swmi_local_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocalFull, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                           const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                           void *d_steps, void *stream)
{
    return device(kTableLocalFull, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_steps,
                  stream);
}

int swmi_local_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                    int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocalFull, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves, steps);
}

int swmi_local_full_release_workspaces(void) { return table_release_workspaces(kTableLocalFull); }

int swmi_local_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableLocalFull, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                       d_moves, d_steps, stream, iters, avg_ms);
}

int swmi_local_full_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return expand_moves(SWMI_LOCAL_FULL_MAX_LEN, SWMI_LOCAL_FULL_MAX_LEN, moves, steps, end_i, end_j, positions, cap);
}

// ---- local with affine gaps, any two lengths (section 18) ----
size_t swmi_local_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocalFullAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                  const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                  void *d_moves, void *d_steps, void *stream)
{
    return device(kTableLocalFullAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                  d_moves, d_steps, stream);
}

int swmi_local_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                           const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                           uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocalFullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores, ends,
                moves, steps);
}

int swmi_local_full_affine_release_workspaces(void) { return table_release_workspaces(kTableLocalFullAffine); }

int swmi_local_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableLocalFullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n,
                       d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- global / fit / overlap, any two lengths (section 20) ----
size_t swmi_global_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableGlobalFull, n, len1, len2, traceback, sizes, cap);
}

int swmi_global_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                            void *d_moves, void *d_steps, void *stream)
{
    return device(kTableGlobalFull, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                  d_steps, stream);
}

int swmi_global_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableGlobalFull, __func__, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, seq1s, seq2s, n, scores, ends, moves,
                steps);
}

int swmi_global_full_release_workspaces(void) { return table_release_workspaces(kTableGlobalFull); }

int swmi_global_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                 const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                                 void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableGlobalFull, __func__, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, d_seq1s, d_seq2s, n, d_scores,
                       d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- global / fit / overlap with affine gaps, any two lengths (section 21) ----
size_t swmi_global_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableGlobalFullAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_global_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                   const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                   void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return device(kTableGlobalFullAffine, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, d_seq1s, d_seq2s, n, d_scores,
                  d_ends, d_moves, d_steps, stream);
}

int swmi_global_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, int32_t *scores,
                            int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableGlobalFullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, seq1s, seq2s, n, scores,
                ends, moves, steps);
}

int swmi_global_full_affine_release_workspaces(void) { return table_release_workspaces(kTableGlobalFullAffine); }

int swmi_global_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                        const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                        void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                        float *avg_ms)
{
    return time_device(kTableGlobalFullAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, d_seq1s, d_seq2s,
                       n, d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- global / fit / overlap up to 65536 x 65536 (section 23) ----
size_t swmi_global_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableGlobalLong, n, len1, len2, traceback, sizes, cap);
}

int swmi_global_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                            void *d_moves, void *d_steps, void *stream)
{
    return device(kTableGlobalLong, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                  d_steps, stream);
}

int swmi_global_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableGlobalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, seq1s, seq2s, n, scores, ends, moves,
                steps);
}

int swmi_global_long_release_workspaces(void) { return table_release_workspaces(kTableGlobalLong); }

int swmi_global_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                 const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                                 void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableGlobalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, free_ends}, d_seq1s, d_seq2s, n, d_scores,
                       d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

int swmi_global_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return expand_moves(SWMI_GLOBAL_LONG_MAX_LEN, SWMI_GLOBAL_LONG_MAX_LEN, moves, steps, end_i, end_j, positions, cap);
}

// ---- the same with affine gaps (section 23) ----
size_t swmi_global_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableGlobalLongAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_global_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                   const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                   void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return device(kTableGlobalLongAffine, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, d_seq1s, d_seq2s, n, d_scores,
                  d_ends, d_moves, d_steps, stream);
}

int swmi_global_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, int32_t *scores,
                            int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableGlobalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, seq1s, seq2s, n, scores,
                ends, moves, steps);
}

int swmi_global_long_affine_release_workspaces(void) { return table_release_workspaces(kTableGlobalLongAffine); }

int swmi_global_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                        const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                        void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                        float *avg_ms)
{
    return time_device(kTableGlobalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, free_ends}, d_seq1s, d_seq2s,
                       n, d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- local up to 65536 x 65536 (section 25) ----
size_t swmi_local_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocalLong, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                           int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return device(kTableLocalLong, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                  d_steps, stream);
}

int swmi_local_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                    int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves, steps);
}

int swmi_local_long_release_workspaces(void) { return table_release_workspaces(kTableLocalLong); }

int swmi_local_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableLocalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                       d_moves, d_steps, stream, iters, avg_ms);
}

int swmi_local_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return expand_moves(SWMI_LOCAL_LONG_MAX_LEN, SWMI_LOCAL_LONG_MAX_LEN, moves, steps, end_i, end_j, positions, cap);
}

// ---- the same with affine gaps (section 25) ----
size_t swmi_local_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableLocalLongAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                  const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                  void *d_moves, void *d_steps, void *stream)
{
    return device(kTableLocalLongAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                  d_moves, d_steps, stream);
}

int swmi_local_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                           const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                           uint64_t *moves, uint32_t *steps)
{
    return host(kTableLocalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores, ends,
                moves, steps);
}

int swmi_local_long_affine_release_workspaces(void) { return table_release_workspaces(kTableLocalLongAffine); }

int swmi_local_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableLocalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n,
                       d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// ---- exact semi-global up to 65536 x 65536 (section 26) ----
size_t swmi_semiglobal_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableSemiglobalLong, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                                int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_lengths, void *stream)
{
    return device(kTableSemiglobalLong, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                  d_lengths, stream);
}

int swmi_semiglobal_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                         int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths)
{
    return host(kTableSemiglobalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves,
                lengths);
}

int swmi_semiglobal_long_release_workspaces(void) { return table_release_workspaces(kTableSemiglobalLong); }

int swmi_semiglobal_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                     void *d_lengths, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableSemiglobalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores,
                       d_ends, d_moves, d_lengths, stream, iters, avg_ms);
}

int swmi_semiglobal_long_expand_moves(const uint64_t *moves, uint32_t length, int32_t *traceback, size_t cap)
{
    return semiglobal_expand_moves(SWMI_SEMIGLOBAL_LONG_MAX_TRACEBACK, moves, length, traceback, cap);
}

// ---- the same with affine gaps (section 26) ----
size_t swmi_semiglobal_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kTableSemiglobalLongAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_lengths, void *stream)
{
    return device(kTableSemiglobalLongAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores,
                  d_ends, d_moves, d_lengths, stream);
}

int swmi_semiglobal_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return host(kTableSemiglobalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores,
                ends, moves, lengths);
}

int swmi_semiglobal_long_affine_release_workspaces(void) { return table_release_workspaces(kTableSemiglobalLongAffine); }

int swmi_semiglobal_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                            void *d_moves, void *d_lengths, void *stream, int iters, float *avg_ms)
{
    return time_device(kTableSemiglobalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n,
                       d_scores, d_ends, d_moves, d_lengths, stream, iters, avg_ms);
}

}  // extern "C"
