// global_long_api.cpp -- C entries of the global and free-end-gap aligner for two sequences of up to 65536 bases, with end cell,
// start cell and traceback (swmi_global_long*, include/swmi.h).  They run through the slice pipeline of
// swmi_table.cpp (struct Table, swmi_host.h); this file is the only host source that names launch_global_long, and its name
// lies outside csrc/swmi_*.cpp, which tests/test_table_host_fake.py links against a fake GPU that does not know this launcher.
#include "swmi_host.h"

#include <algorithm>
#include <cstdlib>

namespace swmi {
namespace host {
namespace {

constexpr size_t kStripe = SWMI_GLOBAL_FULL_MAX_LEN;      // columns of one stripe = what the fixed-length kernels reach

// A shape that the fixed-length kernel reaches goes to it: every field is then swmi_global_full's by construction.
hipError_t launch_global_long_slice(const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends,
                                    uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_global_full(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.free_ends, scores, ends, codes, moves, counts,
                                        t.move_words, st);
    return swmi::launch_global_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.free_ends, scores, ends, codes, moves, counts,
                                    t.move_words, t.carry, st);
}

bool len_ok(size_t len) { return len >= 1 && len <= SWMI_GLOBAL_LONG_MAX_LEN; }

int check_global_long(size_t len1, size_t len2, const int8_t *sm, int gap, unsigned free_ends)
{
    if (!len_ok(len1) || !len_ok(len2))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "lengths (%zu, %zu) outside [1, %d]", len1, len2, SWMI_GLOBAL_LONG_MAX_LEN);
    if (free_ends > SWMI_ENDS_OVERLAP) return fail(SWMI_ERR_INVALID_ARGUMENT, "free_ends %u above %u", free_ends, SWMI_ENDS_OVERLAP);
    const int rc = check_params(sm, gap);
    if (rc != SWMI_OK) return rc;
    if (!global_long_domain_ok(len1, len2, sm, gap, 0))
        return fail(SWMI_ERR_INVALID_ARGUMENT, "max(1, |score|, gap) * (len1 + len2) = P * %zu above 2^23", len1 + len2);
    return SWMI_OK;
}

}  // namespace

bool global_long_domain_ok(size_t len1, size_t len2, const int8_t *sm, int gap_a, int gap_b)
{
    size_t p = 1;
    for (int x = 0; x < 16; ++x) p = std::max(p, (size_t)std::abs((int)sm[x]));
    p = std::max(p, (size_t)std::abs(gap_a));
    p = std::max(p, (size_t)std::abs(gap_b));
    return p * (len1 + len2) <= (size_t(1) << 23);
}

Table global_long_table(size_t len1, size_t len2, const int8_t *sm, int gap, unsigned free_ends)
{
    // the budgets are swmi_global_full's (256 alignments of 16384 x 16384 with a traceback); the carry is counted in a slice
    Table t = global_full_table(kStripe, kStripe, sm, gap, free_ends);
    t.launch = launch_global_long_slice;
    t.state = &Context::global_long_state;
    t.len1 = len1;
    t.len2 = len2;
    t.code_words = swmi::global_long_code_words((int)len1, (int)len2);
    t.move_words = SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2);
    t.carry_words = len2 > kStripe ? len1 : 0;
    return t;
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

size_t swmi_global_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    if (!len_ok(len1) || !len_ok(len2)) return 0;
    return table_slices_for(global_long_table(len1, len2, nullptr, 0, 0), n, traceback != 0, sizes, cap);
}

int swmi_global_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                            const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                            void *d_moves, void *d_steps, void *stream)
{
    const int rc = check_global_long(len1, len2, score_matrix, gap_penalty, free_ends);
    if (rc != SWMI_OK) return rc;
    return table_device(global_long_table(len1, len2, score_matrix, gap_penalty, free_ends), d_seq1s, d_seq2s, n, d_scores, d_ends,
                        d_moves, d_steps, stream);
}

int swmi_global_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    const int rc = check_global_long(len1, len2, score_matrix, gap_penalty, free_ends);
    if (rc != SWMI_OK) return rc;
    return table_host(global_long_table(len1, len2, score_matrix, gap_penalty, free_ends), __func__, seq1s, seq2s, n, scores, ends,
                      moves, steps);
}

int swmi_global_long_release_workspaces(void) { return table_release_workspaces(&Context::global_long_state); }

int swmi_global_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                 const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends,
                                 void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    int rc = check_global_long(len1, len2, score_matrix, gap_penalty, free_ends);
    if (rc == SWMI_OK) rc = table_check_timer(n, iters, avg_ms);       // (its last check makes the context current)
    if (rc != SWMI_OK) return rc;
    return table_time_device(global_long_table(len1, len2, score_matrix, gap_penalty, free_ends), __func__, d_seq1s, d_seq2s, n,
                             d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

// swmi_local_full_expand_moves with the striped aligners' bounds on the end cell
int swmi_global_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    if ((!moves && steps) || (!positions && cap)) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (end_i < 0 || end_j < 0 || end_i > SWMI_GLOBAL_LONG_MAX_LEN || end_j > SWMI_GLOBAL_LONG_MAX_LEN)
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
