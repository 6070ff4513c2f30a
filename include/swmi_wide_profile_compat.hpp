// swmi_wide_profile_compat.hpp -- C++ batch overloads of the profile aligners (swmi_wide_profile.h,
// libswmi_wide_profile.so): a batch of sequences over 32 letters against ONE position-specific profile, on swmi_compat.hpp's
// piece pipeline, move layout and path expander, as swmi_wide_compat.hpp has them: link libswmi_wide_profile.so and
// libswmi.so.  No swmi_init is needed: the calls run on the calling thread's current HIP device.
#ifndef SWMI_WIDE_PROFILE_COMPAT_HPP
#define SWMI_WIDE_PROFILE_COMPAT_HPP

#include "swmi_compat.hpp"
#include "swmi_wide_profile.h"

namespace swmi {

namespace detail {

// Throws std::runtime_error("<what>: <libswmi_wide_profile.so's last error>") unless rc is SWMI_OK.
inline void check_wide_profile(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_wide_profile_last_error());
}

// The sequences in pieces of at most `piece` alignments (0 counts as 4096), each one call of `call`(seq1 bytes, offsets, m,
// scores, ends, moves, steps) -- the C entry with the profile and its parameters bound -- so only two pieces' inputs and moves
// are held at a time; the profile is not staged: every piece's call reads the caller's.  Paths and threads as in
// full_ragged_batch.
template <class Call>
inline std::vector<Result> wide_profile_batch(const char *name, const Sequences &seqs, const std::vector<int8_t> &profile, size_t piece,
                                              unsigned threads, Call call)
{
    if (profile.size() % SWMI_WIDE_LETTERS) throw std::invalid_argument(std::string(name) + ": the profile must hold 32 scores per column");
    const size_t len2 = profile.size() / SWMI_WIDE_LETTERS;
    if (piece == 0) piece = 4096;
    auto align = [&](PieceBuffers &p, size_t off, size_t m) {
        p.seq1s.clear();
        p.seq1_offsets.assign(1, 0);
        for (size_t k = 0; k < m; ++k) {
            p.seq1s.insert(p.seq1s.end(), seqs[off + k].begin(), seqs[off + k].end());
            p.seq1_offsets.push_back(p.seq1s.size());
        }
        if (p.seq1s.empty()) p.seq1s.push_back(0);      // (every sequence of the piece is empty: a pointer that is never read)
        p.move_offsets.resize(m + 1);
        check_wide_profile(swmi_wide_profile_move_offsets(p.seq1_offsets.data(), m, len2, p.move_offsets.data()), name);
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(p.move_offsets[m] ? p.move_offsets[m] : 1);
        p.counts.resize(m);
        check_wide_profile(call(p.seq1s.data(), p.seq1_offsets.data(), m, len2 ? profile.data() : nullptr, len2, p.scores.data(),
                                p.ends.data(), p.moves.data(), p.counts.data()),
                           name);
    };
    return run_in_pieces(seqs.size(), piece, expander_threads(threads), align, [](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], local_full_path(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends.data() + 4 * k)};
    });
}

}  // namespace detail

// Local alignment with affine gaps of every seqs[k] (any length in [0, 16384], 32 letters) against the profile
// (swmi_wide_profile_local): profile[j * 32 + a] is the score of letter a in column j + 1, profile.size() = 32 len2, len2 in
// [0, 4096].  result[k] = (score, path from the start cell to the end cell), and (0, {(0, 0)}) when the sequence or the
// profile is empty.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_wide_profile_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seqs, const std::vector<int8_t> &profile, int gap_open, int gap_extend, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::wide_profile_batch("SmithWaterman_wide_profile_mi355x_batch", seqs, profile, piece, threads,
                                      [&](const uint8_t *a, const uint64_t *oa, size_t m, const int8_t *p, size_t len2, int32_t *sc,
                                          int32_t *e, uint64_t *mv, uint32_t *st) {
                                          return swmi_wide_profile_local(a, oa, m, p, len2, gap_open, gap_extend, sc, e, mv, st);
                                      });
}

// Global / fit / overlap alignment with affine gaps against the profile (swmi_wide_profile_global), also for an empty
// sequence or profile, whose table is one border (swmi.h has the closed form).  Shapes, pieces, moves and threads as above.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_wide_profile_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seqs, const std::vector<int8_t> &profile, int gap_open, int gap_extend,
    unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0, unsigned threads = 0)
{
    return detail::wide_profile_batch("NeedlemanWunsch_wide_profile_mi355x_batch", seqs, profile, piece, threads,
                                      [&](const uint8_t *a, const uint64_t *oa, size_t m, const int8_t *p, size_t len2, int32_t *sc,
                                          int32_t *e, uint64_t *mv, uint32_t *st) {
                                          return swmi_wide_profile_global(a, oa, m, p, len2, gap_open, gap_extend, free_ends, sc, e, mv, st);
                                      });
}

}  // namespace swmi

#endif  // SWMI_WIDE_PROFILE_COMPAT_HPP
