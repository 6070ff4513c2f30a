// local_affine_api.cpp -- C entries of the affine-gap local aligner with end cell, start cell and traceback
// (swmi_local_align_affine*, include/swmi.h).  They run through the slice pipeline of swmi_table.cpp
// (struct Table, swmi_host.h); this file is the only host source that names launch_local_affine, and its name lies outside
// csrc/swmi_*.cpp, which tests/test_table_host_fake.py links against a fake GPU that knows the other two launchers only.
#include "swmi_host.h"

namespace swmi {
namespace host {
namespace {

// A traceback slice holds as many alignments as 4096 of len1 = 16384 (about 4.1 GiB: 1.0 MiB of codes each): a full-length
// slice gives every CU of an MI355X a workgroup of 16 alignments.
constexpr size_t kAffineSliceAlignments = 4096;

hipError_t launch_affine_slice(const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends,
                               uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    return swmi::launch_local_affine(s1, s2, (int)t.len1, n, t.sm, t.gap, t.gap_extend, scores, ends, codes, moves, counts,
                                     t.move_words, st);
}


bool len1_ok(size_t len1) { return len1 >= 1 && len1 <= SWMI_LOCAL_MAX_LEN; }

int check_affine(size_t len1, const int8_t *sm, int gap_open, int gap_extend)
{
    if (!len1_ok(len1)) return fail(SWMI_ERR_INVALID_ARGUMENT, "len1 %zu outside [1, %d]", len1, SWMI_LOCAL_MAX_LEN);
    if (!sm) return fail(SWMI_ERR_INVALID_ARGUMENT, "score_matrix is NULL");
    if (gap_open < 0 || gap_open > 127 || gap_extend < 0 || gap_extend > 127)
        return fail(SWMI_ERR_DOMAIN, "gap_open %d / gap_extend %d outside [0,127]", gap_open, gap_extend);
    return SWMI_OK;
}

}  // namespace

Table affine_table(size_t len1, const int8_t *sm, int gap_open, int gap_extend)
{
    Table t{launch_affine_slice, &Context::local_affine_state, 0, "steps", len1, SWMI_LOCAL_SEQ2_LEN, 4,
            swmi::local_affine_code_words((int)len1), SWMI_LOCAL_MOVE_WORDS(len1), 0, sm, gap_open, gap_extend};
    Table full = t;
    full.len1 = SWMI_LOCAL_MAX_LEN;
    full.code_words = swmi::local_affine_code_words(SWMI_LOCAL_MAX_LEN);
    full.move_words = SWMI_LOCAL_MOVE_WORDS(SWMI_LOCAL_MAX_LEN);
    t.tb_slice_bytes = kAffineSliceAlignments * table_slice_bytes(full, true);
    return t;
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

size_t swmi_local_affine_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap)
{
    return len1_ok(len1) ? table_slices_for(affine_table(len1, nullptr, 0, 0), n, traceback != 0, sizes, cap) : 0;
}

int swmi_local_align_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                                   int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                   void *stream)
{
    const int rc = check_affine(len1, score_matrix, gap_open, gap_extend);
    if (rc != SWMI_OK) return rc;
    return table_device(affine_table(len1, score_matrix, gap_open, gap_extend), d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                        d_steps, stream);
}

int swmi_local_align_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                            int gap_open, int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    const int rc = check_affine(len1, score_matrix, gap_open, gap_extend);
    if (rc != SWMI_OK) return rc;
    return table_host(affine_table(len1, score_matrix, gap_open, gap_extend), __func__, seq1s, seq2s, n, scores, ends, moves, steps);
}

int swmi_local_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n, const int8_t score_matrix[16],
                                  int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                  void *stream, int iters, float *avg_ms)
{
    int rc = table_check_timer(n, iters, avg_ms);
    if (rc == SWMI_OK) rc = check_affine(len1, score_matrix, gap_open, gap_extend);
    if (rc != SWMI_OK) return rc;
    return table_time_device(affine_table(len1, score_matrix, gap_open, gap_extend), __func__, d_seq1s, d_seq2s, n, d_scores,
                             d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

}  // extern "C"
