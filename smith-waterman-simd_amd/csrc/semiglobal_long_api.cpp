// semiglobal_long_api.cpp -- C entries of the exact semi-global aligners for sequences up to 65536 long (include/swmi.h, DESIGN.md
// section 26): the two families' slice launchers, their rows and one explicit extern "C" definition per exported name.  The check, the
// Table and every kind of entry are table_api.cpp's one body each (swmi_host.h: family_*).  The two families live beside
// table_api.cpp, as local_long_api.cpp does: this is the only host source that names launch_sgfull_long*, so a program
// that links table_api.cpp without the long semi-global kernels still links.
#include "swmi_host.h"

namespace swmi {
namespace host {
namespace {

constexpr size_t kStripe = SWMI_SGFULL_MAX_LEN;       // columns of one stripe = what the fixed-length semi-global kernels reach

#define SLICE_ARGS const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends, uint32_t *codes, \
                   unsigned long long *moves, uint32_t *counts, hipStream_t st

unsigned long long *qwords(uint32_t *codes) { return reinterpret_cast<unsigned long long *>(codes); }   // the affine launchers' unit

// A shape that the fixed-length kernel reaches goes to it: every field is then swmi_semiglobal_full's by construction.
hipError_t launch_semiglobal_long_slice(SLICE_ARGS)
{
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_sgfull(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words, st);
    return swmi::launch_sgfull_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                    t.carry, st);
}
hipError_t launch_semiglobal_long_affine_slice(SLICE_ARGS)
{
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_sgfull_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                          moves, counts, t.move_words, st);
    return swmi::launch_sgfull_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                           moves, counts, t.move_words, t.carry, st);
}
#undef SLICE_ARGS

// The fixed-length semi-global pair's budget (256 alignments of 16384 x 16384), count ("lengths": the moves + 1),
// ends[2] and move words; a carry where len2 > 16384; and the domain rule, because H is not floored
// (sgfull_long_kernels.hip).  On a shape that both families reach the code sizes are equal (tile::code_words), so the slices
// are the fixed entries'.
constexpr FamilyRow kSemiglobalLong = {
    launch_semiglobal_long_slice, kTableSemiglobalLong, SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, "lengths", 1, 2,
    [](size_t a, size_t b) { return swmi::sgfull_long_code_words((int)a, (int)b); },
    [](size_t a, size_t b) { return size_t(SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableSgfull,
    /* affine */ false, /* mask */ false, /* carry */ true, /* domain */ true, /* timer_first */ false};
constexpr FamilyRow kSemiglobalLongAffine = {
    launch_semiglobal_long_affine_slice, kTableSemiglobalLongAffine, SWMI_SEMIGLOBAL_LONG_MAX_LEN, false, "lengths", 1, 2,
    [](size_t a, size_t b) { return 2 * swmi::sgfull_long_affine_code_qwords((int)a, (int)b); },
    [](size_t a, size_t b) { return size_t(SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableSgfullAffine,
    /* affine */ true, /* mask */ false, /* carry */ true, /* domain */ true, /* timer_first */ false};
static_assert(kSemiglobalLong.budget_as < kTableApiFamilies && kSemiglobalLongAffine.budget_as < kTableApiFamilies);

// The shared timer body looks for a device before its first call looks at moves / lengths; these two timers refuse a traceback
// given by half where the host and device entries do, behind the call's own check and before any device is touched.
int timer_check(const FamilyRow &r, const Call &c, const void *d_moves, const void *d_lengths)
{
    const int rc = family_check(r, c);
    if (rc != SWMI_OK) return rc;
    if (!d_moves != !d_lengths)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and %s must both be given (traceback) or both be NULL (ends-only)", r.count);
    return SWMI_OK;
}

}  // namespace
}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

// ---- exact semi-global up to 65536 x 65536 (section 26) ----
size_t swmi_semiglobal_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return family_slices_for(kSemiglobalLong, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                                int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_lengths, void *stream)
{
    return family_device(kSemiglobalLong, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                         d_lengths, stream);
}

int swmi_semiglobal_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                         int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths)
{
    return family_host(kSemiglobalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves,
                       lengths);
}

int swmi_semiglobal_long_release_workspaces(void) { return table_release_workspaces(kTableSemiglobalLong); }

int swmi_semiglobal_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                     void *d_lengths, void *stream, int iters, float *avg_ms)
{
    const Call c{len1, len2, score_matrix, gap_penalty, 0, 0};
    const int rc = timer_check(kSemiglobalLong, c, d_moves, d_lengths);
    if (rc != SWMI_OK) return rc;
    return family_time_device(kSemiglobalLong, __func__, c, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_lengths, stream, iters,
                              avg_ms);
}

int swmi_semiglobal_long_expand_moves(const uint64_t *moves, uint32_t length, int32_t *traceback, size_t cap)
{
    return semiglobal_expand_moves(SWMI_SEMIGLOBAL_LONG_MAX_TRACEBACK, moves, length, traceback, cap);
}

// ---- the same with affine gaps (section 26) ----
size_t swmi_semiglobal_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return family_slices_for(kSemiglobalLongAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_semiglobal_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_lengths, void *stream)
{
    return family_device(kSemiglobalLongAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                         d_moves, d_lengths, stream);
}

int swmi_semiglobal_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return family_host(kSemiglobalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores, ends,
                       moves, lengths);
}

int swmi_semiglobal_long_affine_release_workspaces(void) { return table_release_workspaces(kTableSemiglobalLongAffine); }

int swmi_semiglobal_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                            void *d_moves, void *d_lengths, void *stream, int iters, float *avg_ms)
{
    const Call c{len1, len2, score_matrix, gap_open, gap_extend, 0};
    const int rc = timer_check(kSemiglobalLongAffine, c, d_moves, d_lengths);
    if (rc != SWMI_OK) return rc;
    return family_time_device(kSemiglobalLongAffine, __func__, c, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves, d_lengths, stream,
                              iters, avg_ms);
}

}  // extern "C"
