// swmi_banded_ragged_compat.hpp -- C++ batch overloads of the banded aligners on MIXED shapes (swmi_banded_ragged.h,
// libswmi_banded_ragged.so) on swmi_compat.hpp's piece pipeline, move layout and path expander: link libswmi_banded_ragged.so
// and libswmi.so.  No swmi_init is needed: the calls run on the calling thread's current HIP device.
#ifndef SWMI_BANDED_RAGGED_COMPAT_HPP
#define SWMI_BANDED_RAGGED_COMPAT_HPP

#include "swmi_banded_ragged.h"
#include "swmi_compat.hpp"

namespace swmi {

namespace detail {

// Throws std::runtime_error("<what>: <libswmi_banded_ragged.so's last error>") unless rc is SWMI_OK.
inline void check_banded_ragged(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_banded_ragged_last_error());
}

// The two overloads' body: pieces of at most `piece` alignments (0 counts as 4096), each one ragged call, piece p expanded on
// `threads` host threads (0 = as many as the machine reports) while piece p + 1 is aligned.  call(seq1 bytes, offsets, seq2
// bytes, offsets, m, the piece's diagonals or NULL, scores, ends, moves, steps) is the C entry with its parameters bound.
template <class Call>
inline std::vector<Result> banded_ragged_batch(const char *name, const std::vector<std::vector<uint8_t>> &seq1s,
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
        if (swmi_local_full_ragged_move_offsets(p.seq1_offsets.data(), p.seq2_offsets.data(), m, p.move_offsets.data()) != SWMI_OK)
            throw std::invalid_argument(std::string(name) + ": " + swmi_last_error());
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(p.move_offsets[m] ? p.move_offsets[m] : 1);
        p.counts.resize(m);
        check_banded_ragged(call(p.seq1s.data(), p.seq1_offsets.data(), p.seq2s.data(), p.seq2_offsets.data(), m,
                                 diagonals.empty() ? nullptr : diagonals.data() + off, p.scores.data(), p.ends.data(), p.moves.data(),
                                 p.counts.data()),
                            name);
    };
    return run_in_pieces(seq1s.size(), piece, expander_threads(threads), align, [](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], local_full_path(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends.data() + 4 * k)};
    });
}

}  // namespace detail

// Banded local alignment with affine gaps of seq1s[k] against seq2s[k] on the 128 diagonals around diagonals[k] (an empty
// vector: the main diagonal for all), every sequence of a length of its own in [0, 16384] (swmi_banded_ragged_local): result[k]
// is what SmithWaterman_banded_affine_mi355x_batch gives for that pair alone, (score, path from the start cell to the end
// cell), and (0, {(0, 0)}) when either sequence is empty.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_banded_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::banded_ragged_batch("SmithWaterman_banded_affine_mi355x_ragged_batch", seq1s, seq2s, diagonals, piece, threads,
                                       [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                           const int32_t *d, int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                           return swmi_banded_ragged_local(a, oa, b, ob, m, d, score_matrix.data(), gap_open, gap_extend, sc, e,
                                                                           mv, st);
                                       });
}

// The same with no zero floor under the mask free_ends (SWMI_FREE_*, or SWMI_BANDED_END_ANYWHERE with the BEGIN bits;
// swmi_banded_ragged_global): result[k] is what NeedlemanWunsch_banded_affine_mi355x_batch gives for that pair alone, and
// (SWMI_BANDED_NO_ALIGNMENT, {(0, 0)}) where the band holds no alignment, as there.  An empty sequence is taken: the table is
// then one border (swmi_banded_ragged.h).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_banded_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::banded_ragged_batch("NeedlemanWunsch_banded_affine_mi355x_ragged_batch", seq1s, seq2s, diagonals, piece, threads,
                                       [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m,
                                           const int32_t *d, int32_t *sc, int32_t *e, uint64_t *mv, uint32_t *st) {
                                           return swmi_banded_ragged_global(a, oa, b, ob, m, d, score_matrix.data(), gap_open, gap_extend,
                                                                            free_ends, sc, e, mv, st);
                                       });
}

}  // namespace swmi

#endif  // SWMI_BANDED_RAGGED_COMPAT_HPP
