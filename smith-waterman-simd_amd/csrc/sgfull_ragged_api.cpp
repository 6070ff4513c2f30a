// sgfull_ragged_api.cpp -- C entries of the two exact semi-global aligners on a batch of mixed (len1, len2)
// (swmi_semiglobal_full_ragged*, swmi_semiglobal_full_affine_ragged*, include/swmi.h).  A batch becomes a
// TilePlan (tile_ragged_plan.h, shared with the local and the global aligners' ragged entries) and runs through the slice
// pipeline of swmi_table.cpp, on the fixed-length entries' Table (table_api.cpp): their workspaces, their slice budgets, two
// int32 of `ends` per alignment and the count "lengths" = moves + 1.  This file is the only host source that names the ragged
// semi-global launchers, and table_api.cpp does not refer to it, so the fake-GPU build of the fixed-length entries links
// without them.
#include "tile_ragged_plan.h"

namespace swmi {
namespace host {
namespace {

using namespace tile_plan;

// The launches of one slice: one per wave count present, in descending wave count, on the one stream
hipError_t launch_tiles(const Table &t, size_t slice, const uint8_t *s1, const uint8_t *s2, const void *work, size_t n, int32_t *scores,
                        int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts, hipStream_t st)
{
    const TilePlan &p = *static_cast<const TilePlan *>(t.plan);
    return for_each_wave_count(p, slice, work, n, [&](const TileWork *slots, size_t m, int waves) {
        return p.affine ? swmi::launch_sgfull_affine_ragged(s1, s2, slots, m, waves, t.sm, t.gap, t.gap_extend, scores, ends,
                                                            reinterpret_cast<unsigned long long *>(codes), moves, counts, st)
                        : swmi::launch_sgfull_ragged(s1, s2, slots, m, waves, t.sm, t.gap, scores, ends, codes, moves, counts, st);
    });
}

size_t family_code_words(bool affine, int len1, int len2)
{
    return affine ? swmi::sgfull_affine_code_qwords(len1, len2) : swmi::sgfull_code_words(len1, len2);
}

size_t family_tb_slice_bytes(bool affine)
{
    return family_table(affine ? kTableSgfullAffine : kTableSgfull, 1, 1, nullptr, 0, 0, 0).tb_slice_bytes;
}

// what the planner of tile_ragged_plan.h takes from this family (its ragged_bytes counts five result dwords per alignment,
// where this family writes three and with a traceback four: an upper bound, so a slice never outgrows the budget)
constexpr TileFamily kSemiglobal{launch_tiles, swmi::sgfull_ragged_waves, family_code_words, family_tb_slice_bytes};

// checks shared by the host and the device entries, in the order of the global mixed entries without the mask (the lengths,
// which here lie in the offsets, after n = 0 has returned); then the call
int ragged(bool affine, bool device, const char *entry, const void *seq1s, const uint64_t *off1, const void *seq2s, const uint64_t *off2,
           size_t n, const int8_t *sm, int gap, int gap_extend, void *scores, void *ends, void *moves, void *lengths, void *stream)
{
    int rc = affine ? check_affine_gaps(sm, gap, gap_extend) : check_params(sm, gap);
    if (rc != SWMI_OK) return rc;
    if (!moves != !lengths)
        return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and lengths must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    rc = check_both(off1, off2, n);
    if (rc != SWMI_OK) return rc;
    TilePlan plan;
    make_plan(plan, kSemiglobal, off1, off2, n, affine, moves != nullptr);
    Table t = family_table(affine ? kTableSgfullAffine : kTableSgfull, 1, 1, sm, gap, gap_extend, 0);
    t.plan = &plan;
    if (device) return table_device(t, seq1s, seq2s, n, scores, ends, moves, lengths, stream);
    return table_host(t, entry, static_cast<const uint8_t *>(seq1s), static_cast<const uint8_t *>(seq2s), n,
                      static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(lengths));
}

}  // namespace

// The plan alone, for a test of its arithmetic at sizes no test can allocate (tile_ragged_plan.h).  Not part of the C ABI.
bool semiglobal_full_ragged_plan_check(const uint64_t *off1, const uint64_t *off2, size_t n, bool affine, bool tb,
                                       std::vector<size_t> *slice_sizes, std::vector<size_t> *slice_bytes)
{
    return plan_check(kSemiglobal, off1, off2, n, affine, tb, slice_sizes, slice_bytes);
}

}  // namespace host
}  // namespace swmi

using namespace swmi::host;
using namespace swmi::host::tile_plan;

extern "C" {

size_t swmi_semiglobal_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                              int traceback, size_t *sizes, size_t cap)
{
    return slices_for(kSemiglobal, seq1_offsets, seq2_offsets, n, affine != 0, traceback != 0, sizes, cap);
}

int swmi_semiglobal_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, const uint64_t *seq2_offsets,
                                size_t n, const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return ragged(false, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, score_matrix, gap_penalty, 0, scores, ends,
                  moves, lengths, nullptr);
}

int swmi_semiglobal_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                       const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                                       void *d_scores, void *d_ends, void *d_moves, void *d_lengths, void *stream)
{
    return ragged(false, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, score_matrix, gap_penalty, 0, d_scores,
                  d_ends, d_moves, d_lengths, stream);
}

int swmi_semiglobal_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                       const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                       int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths)
{
    return ragged(true, false, __func__, seq1s, seq1_offsets, seq2s, seq2_offsets, n, score_matrix, gap_open, gap_extend, scores,
                  ends, moves, lengths, nullptr);
}

int swmi_semiglobal_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                              const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                              int gap_extend, void *d_scores, void *d_ends, void *d_moves, void *d_lengths,
                                              void *stream)
{
    return ragged(true, true, __func__, d_seq1s, seq1_offsets, d_seq2s, seq2_offsets, n, score_matrix, gap_open, gap_extend, d_scores,
                  d_ends, d_moves, d_lengths, stream);
}

}  // extern "C"
