// swmi_wide_compat.hpp -- C++ batch overloads of the wide-alphabet aligners (swmi_wide.h, libswmi_wide.so), in the shape of
// their 4-letter namesakes in swmi_compat.hpp, whose piece pipeline, move layout and path expander they use: link both
// libraries.  No swmi_init is needed: the calls run on the calling thread's current HIP device.
#ifndef SWMI_WIDE_COMPAT_HPP
#define SWMI_WIDE_COMPAT_HPP

#include "swmi_compat.hpp"
#include "swmi_wide.h"

namespace swmi {

namespace detail {

// Throws std::runtime_error("<what>: <libswmi_wide.so's last error>") unless rc is SWMI_OK; returns SWMI_OK, for the piece
// pipeline's own check (which would quote the other library's text).
inline int check_wide(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_wide_last_error());
    return SWMI_OK;
}

}  // namespace detail

// Local alignment with affine gaps over 32 letters of seq1s[k] against seq2s[k] (swmi_wide_local): seq1s[k] of any length in
// [0, 16384], seq2s[k] in [0, 4096]; score_matrix[(a & 31) * 32 + (b & 31)].  result[k] = (score, path from the start cell to
// the end cell), and (0, {(0, 0)}) when either is empty.  Pieces, moves and threads as in
// SmithWaterman_long_affine_mi355x_ragged_batch.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_wide_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 1024> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    const char *name = "SmithWaterman_wide_affine_mi355x_ragged_batch";
    return local_full_ragged_batch(name, seq1s, seq2s, piece, threads,
                                   [&, name](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                             int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return detail::check_wide(
                                           swmi_wide_local(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend, sc, e, mv, st), name);
                                   });
}

// Global / fit / overlap alignment with affine gaps over 32 letters (swmi_wide_global), also for an empty sequence, whose table
// is one border (swmi.h has the closed form).  Shapes, pieces, moves and threads as above.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_wide_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 1024> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    const char *name = "NeedlemanWunsch_wide_affine_mi355x_ragged_batch";
    return local_full_ragged_batch(name, seq1s, seq2s, piece, threads,
                                   [&, name](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                             int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return detail::check_wide(swmi_wide_global(a, oa, b, ob, m, score_matrix.data(), gap_open,
                                                                                  gap_extend, free_ends, sc, e, mv, st),
                                                                 name);
                                   });
}

}  // namespace swmi

#endif  // SWMI_WIDE_COMPAT_HPP
