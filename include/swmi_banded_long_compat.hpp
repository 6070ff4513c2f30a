// swmi_banded_long_compat.hpp -- C++ batch overloads of the banded aligners on MIXED shapes with the band's width per call for
// sequences up to 65536 long (swmi_banded_long.h, libswmi_banded_long.so) on swmi_compat.hpp's piece pipeline, with this
// library's move layout (swmi_banded_long_move_offsets) and the long local aligners' path expander
// (swmi_local_long_expand_moves): link libswmi_banded_long.so and libswmi.so alone.  No swmi_init is needed: the calls run on
// the calling thread's current HIP device.  The overloads are swmi_banded_width_compat.hpp's over this library's entries; this
// header does not include that one, so that a program which uses only these links only this library.
#ifndef SWMI_BANDED_LONG_COMPAT_HPP
#define SWMI_BANDED_LONG_COMPAT_HPP

#include "swmi_banded_long.h"
#include "swmi_compat.hpp"

namespace swmi {

namespace detail {

// The two overloads' body: pieces of at most `piece` alignments (0 counts as 4096), each one call, piece p expanded on
// `threads` host threads (0 = as many as the machine reports) while piece p + 1 is aligned.  call(seq1 bytes, offsets, seq2
// bytes, offsets, m, the piece's diagonals or NULL, scores, ends, moves, steps) is the C entry with its parameters bound; a
// status other than SWMI_OK throws std::runtime_error("<name>: <libswmi_banded_long.so's last error>").
template <class Call>
inline std::vector<Result> banded_long_batch(const char *name, const std::vector<std::vector<uint8_t>> &seq1s,
                                             const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
                                             size_t piece, unsigned threads, Call call)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    if (!diagonals.empty() && diagonals.size() != seq1s.size())
        throw std::invalid_argument(std::string(name) + ": diagonals must be empty or hold one entry per alignment");
    if (piece == 0) piece = 4096;
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
        if (swmi_banded_long_move_offsets(p.seq1_offsets.data(), p.seq2_offsets.data(), m, p.move_offsets.data()) != SWMI_OK)
            throw std::invalid_argument(std::string(name) + ": " + swmi_banded_long_last_error());
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(p.move_offsets[m] ? p.move_offsets[m] : 1);
        p.counts.resize(m);
        if (call(p.seq1s.data(), p.seq1_offsets.data(), p.seq2s.data(), p.seq2_offsets.data(), m,
                 diagonals.empty() ? nullptr : diagonals.data() + off, p.scores.data(), p.ends.data(), p.moves.data(),
                 p.counts.data()) != SWMI_OK)
            throw std::runtime_error(std::string(name) + ": " + swmi_banded_long_last_error());
    };
    return run_in_pieces(seq1s.size(), piece, expander_threads(threads), align, [](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], local_long_path(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends.data() + 4 * k)};
    });
}

}  // namespace detail

// SmithWaterman_banded_width_affine_mi355x_ragged_batch for sequences of up to 65536 (swmi_banded_long_local).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_banded_long_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
    int band, const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::banded_long_batch("SmithWaterman_banded_long_affine_mi355x_ragged_batch", seq1s, seq2s, diagonals, piece, threads,
                                     [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                         const int32_t *d, int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                         return swmi_banded_long_local(a, oa, b, ob, m, d, band, score_matrix.data(), gap_open, gap_extend,
                                                                       sc, e, mv, st);
                                     });
}

// NeedlemanWunsch_banded_width_affine_mi355x_ragged_batch for sequences of up to 65536 (swmi_banded_long_global).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
    int band, const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL,
    size_t piece = 0, unsigned threads = 0)
{
    return detail::banded_long_batch("NeedlemanWunsch_banded_long_affine_mi355x_ragged_batch", seq1s, seq2s, diagonals, piece, threads,
                                     [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                         const int32_t *d, int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                         return swmi_banded_long_global(a, oa, b, ob, m, d, band, score_matrix.data(), gap_open,
                                                                        gap_extend, free_ends, sc, e, mv, st);
                                     });
}

}  // namespace swmi

#endif  // SWMI_BANDED_LONG_COMPAT_HPP
