// local_full_api.cpp -- C entries of the local aligner for two sequences of any length, with end cell, start cell and
// traceback (swmi_local_full*, include/swmi.h).  They run through the slice pipeline of swmi_table.cpp
// (struct Table, swmi_host.h); this file is the only host source that names launch_local_full, and its name lies outside
// csrc/swmi_*.cpp, which tests/test_table_host_fake.py links against a fake GPU that does not know this launcher.
#include "swmi_host.h"

namespace swmi {
namespace host {
namespace {

// A traceback slice holds as many alignments as 256 of 16384 x 16384 (about 16.1 GiB: 64.25 MiB of codes each, 2 bits per
// cell): one workgroup per alignment, so that a full-size slice gives every CU of an MI355X a workgroup.
constexpr size_t kLocalFullSliceAlignments = 256;

hipError_t launch_local_full_slice(const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends,
                                   uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    return swmi::launch_local_full(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                   st);
}

bool len_ok(size_t len) { return len >= 1 && len <= SWMI_LOCAL_FULL_MAX_LEN; }

int check_local_full(size_t len1, size_t len2, const int8_t *sm, int gap)
{
    if (!len_ok(len1) || !len_ok(len2))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "lengths (%zu, %zu) outside [1, %d]", len1, len2, SWMI_LOCAL_FULL_MAX_LEN);
    return check_params(sm, gap);
}

}  // namespace

Table local_full_table(size_t len1, size_t len2, const int8_t *sm, int gap)
{
    Table t{launch_local_full_slice, &Context::local_full_state, 0, "steps", len1, len2, 4,
            swmi::local_full_code_words((int)len1, (int)len2), SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2), 0, sm, gap, 0};
    Table full = t;
    full.len1 = full.len2 = SWMI_LOCAL_FULL_MAX_LEN;
    full.code_words = swmi::local_full_code_words(SWMI_LOCAL_FULL_MAX_LEN, SWMI_LOCAL_FULL_MAX_LEN);
    full.move_words = SWMI_LOCAL_FULL_MOVE_WORDS(SWMI_LOCAL_FULL_MAX_LEN, SWMI_LOCAL_FULL_MAX_LEN);
    t.tb_slice_bytes = kLocalFullSliceAlignments * table_slice_bytes(full, true);
    return t;
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

size_t swmi_local_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!len_ok(len1) || !len_ok(len2)) return 0;
    return table_slices_for(local_full_table(len1, len2, nullptr, 0), n, traceback != 0, sizes, cap);
}

int swmi_local_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                           const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                           void *d_steps, void *stream)
{
    const int rc = check_local_full(len1, len2, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    return table_device(local_full_table(len1, len2, score_matrix, gap_penalty), d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                        d_steps, stream);
}

int swmi_local_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                    int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    const int rc = check_local_full(len1, len2, score_matrix, gap_penalty);
    if (rc != SWMI_OK) return rc;
    return table_host(local_full_table(len1, len2, score_matrix, gap_penalty), __func__, seq1s, seq2s, n, scores, ends, moves, steps);
}

int swmi_local_full_release_workspaces(void) { return table_release_workspaces(&Context::local_full_state); }

int swmi_local_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_steps, void *stream, int iters, float *avg_ms)
{
    int rc = check_local_full(len1, len2, score_matrix, gap_penalty);
    if (rc == SWMI_OK) rc = table_check_timer(n, iters, avg_ms);       // (its last check makes the context current)
    if (rc != SWMI_OK) return rc;
    return table_time_device(local_full_table(len1, len2, score_matrix, gap_penalty), __func__, d_seq1s, d_seq2s, n, d_scores,
                             d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// swmi_local_expand_moves with both axes up to SWMI_LOCAL_FULL_MAX_LEN: the reference's list from the start cell to the end
// cell.  The start cell is the end cell less the moves' row / column steps, and the list applies the moves last to first.
int swmi_local_full_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    if ((!moves && steps) || (!positions && cap)) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (end_i < 0 || end_j < 0 || end_i > SWMI_LOCAL_FULL_MAX_LEN || end_j > SWMI_LOCAL_FULL_MAX_LEN)
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

}  // extern "C"
