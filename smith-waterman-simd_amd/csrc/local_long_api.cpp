// local_long_api.cpp -- C entries of the local aligners for sequences up to 65536 long (include/swmi.h):
// the two families' slice launchers, their rows and one explicit extern "C" definition per exported name.  The check, the
// Table and every kind of entry are table_api.cpp's one body each (swmi_host.h: family_*).  The two families live beside
// table_api.cpp, as the ragged *_api.cpp files do: this is the only host source that names launch_local_long*, so a program
// that links table_api.cpp without the long local kernels still links.
#include "swmi_host.h"

namespace swmi {
namespace host {
namespace {

constexpr size_t kStripe = SWMI_LOCAL_FULL_MAX_LEN;       // columns of one stripe = what the fixed-length local kernels reach

#define SLICE_ARGS const Table &t, const uint8_t *s1, const uint8_t *s2, size_t n, int32_t *scores, int32_t *ends, uint32_t *codes, \
                   unsigned long long *moves, uint32_t *counts, hipStream_t st

unsigned long long *qwords(uint32_t *codes) { return reinterpret_cast<unsigned long long *>(codes); }   // the affine launchers' unit

// A shape that the fixed-length kernel reaches goes to it: every field is then swmi_local_full's by construction.
hipError_t launch_local_long_slice(SLICE_ARGS)
{
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_local_full(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                       st);
    return swmi::launch_local_long(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, scores, ends, codes, moves, counts, t.move_words,
                                   t.carry, st);
}
hipError_t launch_local_long_affine_slice(SLICE_ARGS)
{
    if (t.len1 <= kStripe && t.len2 <= kStripe)
        return swmi::launch_local_full_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                              moves, counts, t.move_words, st);
    return swmi::launch_local_long_affine(s1, s2, (int)t.len1, (int)t.len2, n, t.sm, t.gap, t.gap_extend, scores, ends, qwords(codes),
                                          moves, counts, t.move_words, t.carry, st);
}
#undef SLICE_ARGS

// The fixed-length local pair's budget (256 alignments of 16384 x 16384), a carry where len2 > 16384, and no domain rule:
// 0 <= H < 2^23 whatever the parameters (local_long_kernels.hip).  On a shape that both families reach the code sizes are
// equal (tile::code_words), so the slices are the fixed entries'.
constexpr FamilyRow kLocalLong = {launch_local_long_slice, kTableLocalLong, SWMI_LOCAL_LONG_MAX_LEN, false, "steps", 0, 4,
                                  [](size_t a, size_t b) { return swmi::local_long_code_words((int)a, (int)b); },
                                  [](size_t a, size_t b) { return size_t(SWMI_LOCAL_LONG_MOVE_WORDS(a, b)); }, 256, kTableLocalFull,
                                  /* affine */ false, /* mask */ false, /* carry */ true, /* domain */ false, /* timer_first */ false};
constexpr FamilyRow kLocalLongAffine = {launch_local_long_affine_slice, kTableLocalLongAffine, SWMI_LOCAL_LONG_MAX_LEN, false, "steps", 0, 4,
                                        [](size_t a, size_t b) { return 2 * swmi::local_long_affine_code_qwords((int)a, (int)b); },
                                        [](size_t a, size_t b) { return size_t(SWMI_LOCAL_LONG_MOVE_WORDS(a, b)); }, 256,
                                        kTableLocalFullAffine, /* affine */ true, /* mask */ false, /* carry */ true,
                                        /* domain */ false, /* timer_first */ false};
static_assert(kLocalLong.budget_as < kTableApiFamilies && kLocalLongAffine.budget_as < kTableApiFamilies);

}  // namespace
}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

// ---- local up to 65536 x 65536 (section 25) ----
size_t swmi_local_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return family_slices_for(kLocalLong, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                           int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream)
{
    return family_device(kLocalLong, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends, d_moves,
                         d_steps, stream);
}

int swmi_local_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                    int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return family_host(kLocalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, seq1s, seq2s, n, scores, ends, moves, steps);
}

int swmi_local_long_release_workspaces(void) { return table_release_workspaces(kTableLocalLong); }

int swmi_local_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                void *d_steps, void *stream, int iters, float *avg_ms)
{
    return family_time_device(kLocalLong, __func__, {len1, len2, score_matrix, gap_penalty, 0, 0}, d_seq1s, d_seq2s, n, d_scores,
                              d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

int swmi_local_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return family_expand_moves(SWMI_LOCAL_LONG_MAX_LEN, SWMI_LOCAL_LONG_MAX_LEN, moves, steps, end_i, end_j, positions, cap);
}

// ---- the same with affine gaps (section 25) ----
size_t swmi_local_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return family_slices_for(kLocalLongAffine, n, len1, len2, traceback, sizes, cap);
}

int swmi_local_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                  const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                  void *d_moves, void *d_steps, void *stream)
{
    return family_device(kLocalLongAffine, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n, d_scores, d_ends,
                         d_moves, d_steps, stream);
}

int swmi_local_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                           const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                           uint64_t *moves, uint32_t *steps)
{
    return family_host(kLocalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, seq1s, seq2s, n, scores, ends,
                       moves, steps);
}

int swmi_local_long_affine_release_workspaces(void) { return table_release_workspaces(kTableLocalLongAffine); }

int swmi_local_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                       const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                       void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms)
{
    return family_time_device(kLocalLongAffine, __func__, {len1, len2, score_matrix, gap_open, gap_extend, 0}, d_seq1s, d_seq2s, n,
                              d_scores, d_ends, d_moves, d_steps, stream, iters, avg_ms);
}

}  // extern "C"
