// local_ragged_api.cpp -- C entries of the two local aligners on a batch of mixed seq1 lengths (swmi_local_align_ragged*,
// swmi_local_align_affine_ragged*, include/swmi.h).  A batch becomes a RaggedPlan (swmi_host.h): slices
// cut in caller order within the aligner's budget, and per slice one LocalWork per alignment, longest first, so that the 4
// alignments of a wavefront and the 16 of a workgroup have similar lengths.  The plan then runs through the slice pipeline of
// swmi_table.cpp, on the fixed-length entries' Table (table_api.cpp: family_table).  The any-length aligners' mixed-shape
// batches have a planner and slots of their own, tile_ragged_api.cpp.  This file is the only host source that names the two
// ragged 128-column launchers, which tests/native/ragged_host_fake.cpp stands in for.
#include "swmi_host.h"

#include <algorithm>

namespace swmi {
namespace host {
namespace {

hipError_t launch_linear_ragged(const Table &t, size_t, const uint8_t *s1, const uint8_t *s2, const void *work, size_t n,
                                int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts,
                                hipStream_t st)
{
    return swmi::launch_local_ragged(s1, s2, static_cast<const LocalWork *>(work), n, t.sm, t.gap, scores, ends, codes, moves, counts, st);
}

hipError_t launch_affine_ragged(const Table &t, size_t, const uint8_t *s1, const uint8_t *s2, const void *work, size_t n,
                                int32_t *scores, int32_t *ends, uint32_t *codes, unsigned long long *moves, uint32_t *counts,
                                hipStream_t st)
{
    return swmi::launch_local_affine_ragged(s1, s2, static_cast<const LocalWork *>(work), n, t.sm, t.gap, t.gap_extend, scores, ends, codes, moves, counts, st);
}

size_t code_words(bool affine, size_t len1)
{
    return affine ? swmi::local_affine_code_words((int)len1) : swmi::local_code_words((int)len1);
}

// device bytes one alignment of a ragged slice takes: inputs, its slot, results, and with a traceback codes, moves and count
size_t ragged_bytes(bool affine, bool tb, size_t len1)
{
    size_t b = len1 + SWMI_LOCAL_SEQ2_LEN + sizeof(LocalWork) + 5 * sizeof(int32_t);
    if (tb) b += code_words(affine, len1) * sizeof(uint32_t) + SWMI_LOCAL_MOVE_WORDS(len1) * sizeof(uint64_t) + sizeof(uint32_t);
    return b;
}

// the fixed-length aligner's budget for one slice's device buffers
size_t budget(bool affine, bool tb)
{
    if (!tb) return kTableSliceBytes;
    return family_table(affine ? kTableLocalAffine : kTableLocal, 1, SWMI_LOCAL_SEQ2_LEN, nullptr, 0, 0, 0).tb_slice_bytes;
}

int check_offsets(const uint64_t *off, size_t n)
{
    if (!off) return fail(SWMI_ERR_INVALID_ARGUMENT, "seq1_offsets is NULL");
    for (size_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return fail(SWMI_ERR_INVALID_ARGUMENT, "seq1_offsets decrease at %zu", k);
        if (off[k + 1] - off[k] > SWMI_LOCAL_MAX_LEN)
            return fail(SWMI_ERR_INVALID_ARGUMENT, "seq1 %zu has length %llu > %d", k, (unsigned long long)(off[k + 1] - off[k]),
                        SWMI_LOCAL_MAX_LEN);
    }
    return SWMI_OK;
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
std::vector<size_t> cut(const uint64_t *off, size_t n, bool affine, bool tb)
{
    const size_t cap = budget(affine, tb);
    std::vector<size_t> first{0};
    size_t bytes = 0, m = 0;
    for (size_t k = 0; k < n; ++k) {
        const size_t b = ragged_bytes(affine, tb, size_t(off[k + 1] - off[k]));
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

void fill_move_offsets(const uint64_t *off, size_t n, uint64_t *out)
{
    out[0] = 0;
    for (size_t k = 0; k < n; ++k) out[k + 1] = out[k] + SWMI_LOCAL_MOVE_WORDS(off[k + 1] - off[k]);
}

// The plan of a checked batch.  Every LocalWork field is relative to its slice and fits 32 bits: a slice's bytes stay within
// the budget (at most about 4.4 GiB), and its seq1 bytes, code dwords and move words are each under a quarter of them.
void make_plan(RaggedPlan &p, const uint64_t *off, size_t n, bool affine, bool tb)
{
    p.launch = affine ? launch_affine_ragged : launch_linear_ragged;
    p.seq1_offsets = off;
    p.move_offsets.resize(n + 1);
    fill_move_offsets(off, n, p.move_offsets.data());
    p.first = cut(off, n, affine, tb);
    p.work.resize(n);
    p.slots = p.work.data();
    p.slot_bytes = sizeof(LocalWork);
    p.code_words.assign(p.first.size() - 1, 0);
    std::vector<uint32_t> at(SWMI_LOCAL_MAX_LEN + 1);       // per length: the next slot of that length
    for (size_t s = 0; s + 1 < p.first.size(); ++s) {
        const size_t a = p.first[s], b = p.first[s + 1];
        // counting sort, longest first, equal lengths in caller order
        std::fill(at.begin(), at.end(), 0u);
        for (size_t k = a; k < b; ++k) ++at[off[k + 1] - off[k]];
        uint32_t slot = 0;
        for (size_t len = SWMI_LOCAL_MAX_LEN + 1; len-- > 0;) {
            const uint32_t c = at[len];
            at[len] = slot;
            slot += c;
        }
        size_t codes = 0;
        for (size_t k = a; k < b; ++k) {
            const uint32_t len1 = uint32_t(off[k + 1] - off[k]);
            p.work[a + at[len1]++] = {uint32_t(k - a), uint32_t(off[k] - off[a]), len1, uint32_t(codes),
                                      uint32_t(p.move_offsets[k] - p.move_offsets[a])};
            if (tb) codes += code_words(affine, len1);
        }
        p.code_words[s] = codes;
        p.max_m = std::max(p.max_m, b - a);
        p.max_seq1 = std::max(p.max_seq1, size_t(off[b] - off[a]));
        p.max_codes = std::max(p.max_codes, codes);
        p.max_moves = std::max(p.max_moves, size_t(p.move_offsets[b] - p.move_offsets[a]));
    }
}

// checks shared by the host and the device entries, in the order of the fixed-length ones; then the call
int ragged(bool affine, bool device, const char *entry, const void *seq1s, const uint64_t *off, const void *seq2s, size_t n,
           const int8_t *sm, int gap, int gap_extend, void *scores, void *ends, void *moves, void *steps, void *stream)
{
    int rc = affine ? check_affine_gaps(sm, gap, gap_extend) : check_params(sm, gap);
    if (rc != SWMI_OK) return rc;
    if (!moves != !steps) return fail(SWMI_ERR_INVALID_ARGUMENT, "moves and steps must both be given (traceback) or both be NULL (ends-only)");
    if (n == 0) return SWMI_OK;
    if (!seq1s || !seq2s || !scores || !ends) return fail(SWMI_ERR_INVALID_ARGUMENT, "NULL buffer with n = %zu", n);
    rc = check_offsets(off, n);
    if (rc != SWMI_OK) return rc;
    RaggedPlan plan;
    make_plan(plan, off, n, affine, moves != nullptr);
    Table t = family_table(affine ? kTableLocalAffine : kTableLocal, 1, SWMI_LOCAL_SEQ2_LEN, sm, gap, gap_extend, 0);
    t.plan = &plan;
    if (device) return table_device(t, seq1s, seq2s, n, scores, ends, moves, steps, stream);
    return table_host(t, entry, static_cast<const uint8_t *>(seq1s), static_cast<const uint8_t *>(seq2s), n,
                      static_cast<int32_t *>(scores), static_cast<int32_t *>(ends), static_cast<uint64_t *>(moves),
                      static_cast<uint32_t *>(steps));
}

}  // namespace
}  // namespace host
}  // namespace swmi

using namespace swmi::host;

extern "C" {

int swmi_local_ragged_move_offsets(const uint64_t *seq1_offsets, size_t n, uint64_t *move_offsets)
{
    if (!move_offsets) return fail(SWMI_ERR_INVALID_ARGUMENT, "move_offsets is NULL");
    const int rc = check_offsets(seq1_offsets, n);
    if (rc != SWMI_OK) return rc;
    fill_move_offsets(seq1_offsets, n, move_offsets);
    return SWMI_OK;
}

size_t swmi_local_ragged_slices_for(const uint64_t *seq1_offsets, size_t n, int affine, int traceback, size_t *sizes, size_t cap)
{
    if (check_offsets(seq1_offsets, n) != SWMI_OK) return 0;
    const std::vector<size_t> first = cut(seq1_offsets, n, affine != 0, traceback != 0);
    for (size_t s = 0; sizes && s + 1 < first.size() && s < cap; ++s) sizes[s] = first[s + 1] - first[s];
    return first.size() - 1;
}

int swmi_local_align_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n,
                            const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves,
                            uint32_t *steps)
{
    return ragged(false, false, __func__, seq1s, seq1_offsets, seq2s, n, score_matrix, gap_penalty, 0, scores, ends, moves, steps,
                  nullptr);
}

int swmi_local_align_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, size_t n,
                                   const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves,
                                   void *d_steps, void *stream)
{
    return ragged(false, true, __func__, d_seq1s, seq1_offsets, d_seq2s, n, score_matrix, gap_penalty, 0, d_scores, d_ends, d_moves,
                  d_steps, stream);
}

int swmi_local_align_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n,
                                   const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                   uint64_t *moves, uint32_t *steps)
{
    return ragged(true, false, __func__, seq1s, seq1_offsets, seq2s, n, score_matrix, gap_open, gap_extend, scores, ends, moves,
                  steps, nullptr);
}

int swmi_local_align_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, size_t n,
                                          const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores, void *d_ends,
                                          void *d_moves, void *d_steps, void *stream)
{
    return ragged(true, true, __func__, d_seq1s, seq1_offsets, d_seq2s, n, score_matrix, gap_open, gap_extend, d_scores, d_ends,
                  d_moves, d_steps, stream);
}

}  // extern "C"
