// global_long_affine_api.cpp -- C entries of the global and free-end-gap aligner with affine gaps for two sequences of up to
// 65536 bases, with end cell, start cell and traceback (swmi_global_long_affine*, include/swmi.h).  They
// run through the slice pipeline of swmi_table.cpp (struct Table, swmi_host.h); this file is the only host source that names
// launch_global_long_affine, and its name lies outside csrc/swmi_*.cpp, which tests/test_table_host_fake.py links against a
// fake GPU that does not know this launcher.
#include "swmi_host.h"

namespace swmi {
namespace host {
namespace {

constexpr size_t kStripe = SWMI_GLOBAL_FULL_MAX_LEN;      // columns of one stripe = what the fixed-length kernels reach

// A shape that the fixed-length kernel reaches goes to it: every field is then swmi_global_full_affine's by construction.
hipError_t launch_global_long_affine_slice(const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores,
                                           int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    unsigned long long *qcodes = reinterpret_cast<unsigned long long *>(codes);
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_global_full_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, t.free_ends, scores, ends,
                                               qcodes, moves, counts, t.move_words, st);
    return swmi::launch_global_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, t.free_ends, scores, ends,
                                           qcodes, moves, counts, t.move_words, t.carry, st);
}

bool len_ok(size_t len) { return len >= 1 && len <= SWMI_GLOBAL_LONG_MAX_LEN; }

int check_global_long_affine(size_t len1, size_t len2, const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends)
{
    if (!len_ok(len1) || !len_ok(len2))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "lengths (%zu, %zu) outside [1, %d]", len1, len2, SWMI_GLOBAL_LONG_MAX_LEN);
    if (free_ends > SWMI_ENDS_OVERLAP) return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", free_ends, SWMI_ENDS_OVERLAP);
    if (!sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (gap_open < 0 || gap_open > 127 || gap_extend < 0 || gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", gap_open, gap_extend);
    if (!global_long_domain_ok(len1, len2, sm, gap_open, gap_extend))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "max(1, |score|, gap_open, gap_extend) * (len1 + len2) = P * %zu above 2^23", len1 + len2);
    return SWMI_OK;
}

}  // namespace

Table global_long_affine_table(size_t len1, size_t len2, const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends)
{
    // the budgets are swmi_global_full_affine's (256 alignments of 16384 x 16384 with a traceback); the carry is counted in a slice
    Table t = global_full_affine_table(kStripe, kStripe, sm, gap_open, gap_extend, free_ends);
    t.launch = launch_global_long_affine_slice;
    t.state = &Context::global_long_affine_state;
    t.len1 = len1;
    t.len2 = len2;
    t.code_words = 2 * swmi::global_long_affine_code_qwords((int)len1, (int)len2);   // the Table's unit is dwords
    t.move_words = SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2);
    t.carry_words = len2 > kStripe ? 2 * len1 : 0;                                    // (H, F) per row
    return t;
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

size_t swmi_global_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!len_ok(len1) || !len_ok(len2)) return 0;
    return table_slices_for(global_long_affine_table(len1, len2, nullptr, 0, 0, 0), n, traceback != 0, sizes, cap);
}

int swmi_global_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                   const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                   void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    const int rc = check_global_long_affine(len1, len2, score_matrix, gap_open, gap_extend, free_ends);
    if (rc != SWMI_OK) return rc;
    return table_device(global_long_affine_table(len1, len2, score_matrix, gap_open, gap_extend, free_ends), d_seq1s, d_seq2s, n,
                        d_scores, d_ends, d_moves, d_steps, stream);
}

int swmi_global_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends, int32_t *scores,
                            int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    const int rc = check_global_long_affine(len1, len2, score_matrix, gap_open, gap_extend, free_ends);
    if (rc != SWMI_OK) return rc;
    return table_host(global_long_affine_table(len1, len2, score_matrix, gap_open, gap_extend, free_ends), __func__, seq1s, seq2s, n,
                      scores, ends, moves, steps);
}

int swmi_global_long_affine_release_workspaces(void) { return table_release_workspaces(&Context::global_long_affine_state); }

int swmi_global_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                        const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                        void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                        float *avg_ms)
{
    int rc = check_global_long_affine(len1, len2, score_matrix, gap_open, gap_extend, free_ends);
    if (rc == SWMI_OK) rc = table_check_timer(n, iters, avg_ms);       // (its last check makes the context current)
    if (rc != SWMI_OK) return rc;
    return table_time_device(global_long_affine_table(len1, len2, score_matrix, gap_open, gap_extend, free_ends), __func__, d_seq1s,
                             d_seq2s, n, d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

}  // extern "C"
