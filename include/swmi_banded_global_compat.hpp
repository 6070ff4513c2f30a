// swmi_banded_global_compat.hpp -- C++ batch overload of the banded global / fit / overlap / extension aligner
// (swmi_banded_global.h, libswmi_banded_global.so) on swmi_compat.hpp's piece pipeline, move layout and path expander: link
// libswmi_banded_global.so and libswmi.so.  No swmi_init is needed: the calls run on the calling thread's current HIP device.
#ifndef SWMI_BANDED_GLOBAL_COMPAT_HPP
#define SWMI_BANDED_GLOBAL_COMPAT_HPP

#include "swmi_banded_global.h"
#include "swmi_compat.hpp"

namespace swmi {

namespace detail {

// Throws std::runtime_error("<what>: <libswmi_banded_global.so's last error>") unless rc is SWMI_OK.
inline void check_banded_global(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_banded_global_last_error());
}

}  // namespace detail

// Banded alignment with affine gaps and no zero floor of seq1s[k] against seq2s[k] on the 128 diagonals around diagonals[k] (an
// empty vector: the main diagonal for all) under the mask free_ends (SWMI_FREE_*, or SWMI_BANDED_END_ANYWHERE with the BEGIN
// bits), every seq1 of one length and every seq2 of one length in [1, 16384] (swmi_banded_global).  result[k] = (score, path
// from the start cell to the end cell); (SWMI_BANDED_NO_ALIGNMENT, {(0, 0)}) where the band holds no alignment.  In pieces of
// `piece` alignments, at most one traceback slice (0 = one slice), piece p expanded on `threads` host threads (0 = as many as
// the machine reports) while piece p + 1 is aligned.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_banded_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, const std::vector<int32_t> &diagonals,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    const char *name = "NeedlemanWunsch_banded_affine_mi355x_batch";
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    if (!diagonals.empty() && diagonals.size() != seq1s.size())
        throw std::invalid_argument(std::string(name) + ": diagonals must be empty or hold one entry per alignment");
    const size_t len1 = detail::common_length(seq1s), len2 = detail::common_length(seq2s);
    detail::check_lengths(name, seq1s, len1, "seq1");
    detail::check_lengths(name, seq2s, len2, "seq2");
    if (seq1s.empty()) return {};
    size_t slice = 0;
    if (swmi_banded_global_slices_for(seq1s.size(), len1, len2, 1, &slice, 1) == 0) detail::check_banded_global(SWMI_ERR_INVALID_ARGUMENT, name);
    if (piece == 0 || piece > slice) piece = slice;
    const size_t mw = SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2);
    auto align = [&](detail::PieceBuffers &p, size_t off, size_t m) {
        p.seq1s.resize(m * (len1 + len2));
        uint8_t *s2 = p.seq1s.data() + m * len1;
        for (size_t k = 0; k < m; ++k) {
            std::copy(seq1s[off + k].begin(), seq1s[off + k].end(), p.seq1s.begin() + k * len1);
            std::copy(seq2s[off + k].begin(), seq2s[off + k].end(), s2 + k * len2);
        }
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(m * mw);
        p.counts.resize(m);
        detail::check_banded_global(swmi_banded_global(p.seq1s.data(), len1, s2, len2, m, diagonals.empty() ? nullptr : diagonals.data() + off,
                                                       score_matrix.data(), gap_open, gap_extend, free_ends, p.scores.data(), p.ends.data(),
                                                       p.moves.data(), p.counts.data()),
                                    "swmi_banded_global");
    };
    return detail::run_in_pieces(seq1s.size(), piece, detail::expander_threads(threads), align, [=](const detail::PieceBuffers &p, size_t k) {
        return detail::Result{p.scores[k], detail::local_full_path(p.moves.data() + k * mw, p.counts[k], p.ends.data() + 4 * k)};
    });
}

}  // namespace swmi

#endif  // SWMI_BANDED_GLOBAL_COMPAT_HPP
