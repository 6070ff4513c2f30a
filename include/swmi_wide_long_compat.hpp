// swmi_wide_long_compat.hpp -- C++ batch overloads of the long wide-alphabet aligners (swmi_wide_long.h, libswmi_wide_long.so:
// both sequences up to 65536 letters), in the shape of swmi_wide_compat.hpp's, on swmi_compat.hpp's piece pipeline
// (detail::run_in_pieces) with this library's move layout (swmi_wide_long_move_offsets) and the long local aligners' path
// expander (swmi_local_long_expand_moves): link -lswmi_wide_long -lswmi.  No swmi_init is needed: the calls run on the calling
// thread's current HIP device.
#ifndef SWMI_WIDE_LONG_COMPAT_HPP
#define SWMI_WIDE_LONG_COMPAT_HPP

#include "swmi_compat.hpp"
#include "swmi_wide_long.h"

namespace swmi {

namespace detail {

// Throws std::runtime_error("<what>: <libswmi_wide_long.so's last error>") unless rc is SWMI_OK.
inline void check_wide_long(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_wide_long_last_error());
}

// full_ragged_batch (swmi_compat.hpp) for lengths up to 65536: the same pieces, staging and threads, with the move layout and
// the expander that reach that far.  call(seq1 bytes, offsets, seq2 bytes, offsets, m, scores, ends, moves, counts) is the C
// entry with its parameters bound.
template <class Call>
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> wide_long_ragged_batch(
    const char *name, const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, size_t piece,
    unsigned threads, Call call)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    if (piece == 0) piece = 4096;
    threads = expander_threads(threads);
    auto stage = [](const std::vector<std::vector<uint8_t>> &seqs, size_t off, size_t m, std::vector<uint8_t> &bytes,
                    std::vector<uint64_t> &offsets) {
        bytes.clear();
        offsets.assign(1, 0);
        for (size_t k = 0; k < m; ++k) {
            bytes.insert(bytes.end(), seqs[off + k].begin(), seqs[off + k].end());
            offsets.push_back(bytes.size());
        }
        if (bytes.empty()) bytes.push_back(0);          // (every sequence of the piece is empty: a pointer that is never read)
    };
    auto align = [&](PieceBuffers &p, size_t off, size_t m) {
        stage(seq1s, off, m, p.seq1s, p.seq1_offsets);
        stage(seq2s, off, m, p.seq2s, p.seq2_offsets);
        p.move_offsets.resize(m + 1);
        check_wide_long(swmi_wide_long_move_offsets(p.seq1_offsets.data(), p.seq2_offsets.data(), m, p.move_offsets.data()), name);
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(p.move_offsets[m] ? p.move_offsets[m] : 1);
        p.counts.resize(m);
        check_wide_long(call(p.seq1s.data(), p.seq1_offsets.data(), p.seq2s.data(), p.seq2_offsets.data(), m, p.scores.data(),
                             p.ends.data(), p.moves.data(), p.counts.data()),
                        name);
    };
    return run_in_pieces(seq1s.size(), piece, threads, align, [=](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], local_long_path(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends.data() + 4 * k)};
    });
}

}  // namespace detail

// Local alignment with affine gaps over 32 letters of seq1s[k] against seq2s[k] (swmi_wide_long_local): each of any length in
// [0, 65536]; score_matrix[(a & 31) * 32 + (b & 31)].  result[k] = (score, path from the start cell to the end cell), and
// (0, {(0, 0)}) when either is empty.  Pieces, moves and threads as in SmithWaterman_wide_affine_mi355x_ragged_batch.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_wide_long_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 1024> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::wide_long_ragged_batch("SmithWaterman_wide_long_affine_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                          [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                              int32_t *e, uint64_t *mv, uint32_t *st) {
                                              return swmi_wide_long_local(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend, sc, e, mv, st);
                                          });
}

// Global / fit / overlap alignment with affine gaps over 32 letters (swmi_wide_long_global; its domain rule applies), also for
// an empty sequence, whose table is one border.  Shapes, pieces, moves and threads as above.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_wide_long_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 1024> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::wide_long_ragged_batch("NeedlemanWunsch_wide_long_affine_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                          [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                              int32_t *e, uint64_t *mv, uint32_t *st) {
                                              return swmi_wide_long_global(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend, free_ends, sc,
                                                                           e, mv, st);
                                          });
}

}  // namespace swmi

#endif  // SWMI_WIDE_LONG_COMPAT_HPP
