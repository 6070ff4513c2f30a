// swmi_compat.hpp -- header-only C++ mirror of the reference's call signature over the C ABI (swmi.h).
//
// The reference's boundary is the free function (source.cpp:462-466, :758-762, :953-957)
//     int SmithWaterman_simdN(const std::array<uint8_t,128>&, const std::array<uint8_t,128>&,
//                             const std::array<int8_t,16>&, const int8_t);
// A maintainer who wants the reference's own drivers (SpeedTest source.cpp:3032-3147,
// TestSimdSmithWaterman :2943-2982) to run on the GPU includes this header and calls
// SmithWaterman_mi355x(...) where they called SmithWaterman_simd4(...) -- or, to keep the 1M-call loop
// shape AND get batch throughput, submits through swmi::PairQueue (same arguments per call).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "swmi.h"

// Same arguments, same return value as SmithWaterman_simd4 (source.cpp:462-466). One synchronous launch per call.
inline int SmithWaterman_mi355x(const std::array<uint8_t, 128> &seq1, const std::array<uint8_t, 128> &seq2,
                                const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty)
{
    const int r = swmi_score_pair(seq1.data(), seq2.data(), score_matrix.data(), gap_penalty);
    if (r < 0) throw std::runtime_error(std::string("swmi_score_pair: ") + swmi_last_error());
    return r;
}

// Same arguments, same return value as SemiGlobal_AdaptiveBanded_XDrop_111_32_70 and its _simd / _simd_mark2..4 variants
// (source.cpp:1836-1838, :1978, call sites TestSemiGlobal :2774-2778, SpeedtestSemiGlobal :2818-2856): (score, traceback from
// (0, 0) to the best cell).  One synchronous call per alignment -- correct, but ~11 ms of latency each: use the batch below.
inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_AdaptiveBanded_XDrop_mi355x(const std::array<uint8_t, 16384> &seq1,
                                                                                              const std::array<uint8_t, 16384> &seq2);

// Same arguments, same return value as SmithWaterman_111_long (source.cpp:1526-1576): (score, path of (i, j) from the start
// cell to the end cell).  One synchronous call per alignment; SmithWaterman_local_mi355x_batch below is the throughput form.
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_111_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::array<uint8_t, 128> &seq2);
// The same local alignment with any score matrix and gap (swmi_local_align: no reference counterpart beyond (1, -1, 1)).
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_local_mi355x(const std::vector<uint8_t> &seq1,
                                                                                  const std::array<uint8_t, 128> &seq2,
                                                                                  const std::array<int8_t, 16> &score_matrix,
                                                                                  const int8_t gap_penalty);
// The same local alignment with affine gaps, a gap of length k costing gap_open + (k-1) gap_extend (swmi_local_align_affine:
// no reference counterpart; open = extend = 1 with (1, -1) is SmithWaterman_111_long).
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                   const std::array<uint8_t, 128> &seq2,
                                                                                   const std::array<int8_t, 16> &score_matrix,
                                                                                   int gap_open, int gap_extend);

// Same arguments, same return value as SemiGlobal_111 (source.cpp:1776-1834): (score, path of (i, j) from (0,0) to the best
// cell) of the exact semi-global alignment, the full table with no band and no X-drop (swmi_semiglobal_full).  One
// synchronous call per alignment; swmi::SemiGlobal_111_mi355x_batch below is the throughput form.
inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_111_mi355x(const std::array<uint8_t, 16384> &seq1,
                                                                             const std::array<uint8_t, 16384> &seq2);
// The same exact semi-global alignment of any lengths in [1, 16384] with affine gaps, a gap of length k costing gap_open +
// (k-1) gap_extend (swmi_semiglobal_full_affine: no reference counterpart; open = extend = 1 with (1, -1) at 16384 x 16384
// is SemiGlobal_111).  One synchronous call per alignment; swmi::SemiGlobal_affine_mi355x_batch is the throughput form.
inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                const std::vector<uint8_t> &seq2,
                                                                                const std::array<int8_t, 16> &score_matrix,
                                                                                int gap_open, int gap_extend);

// Local alignment of two sequences of any lengths in [1, 16384], any score matrix and gap (swmi_local_full): the return value
// of SmithWaterman_111_long, (score, path of (i, j) from the start cell to the end cell), with a seq2 of any length instead
// of a 128-mer.  One synchronous call per alignment; swmi::SmithWaterman_long_mi355x_batch is the throughput form.  For a
// 128-base seq2 SmithWaterman_local_mi355x gives the same result faster.
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                 const std::vector<uint8_t> &seq2,
                                                                                 const std::array<int8_t, 16> &score_matrix,
                                                                                 const int8_t gap_penalty);
// The same any-length local alignment with affine gaps, a gap of length k costing gap_open + (k-1) gap_extend
// (swmi_local_full_affine: no reference counterpart).  One synchronous call per alignment;
// swmi::SmithWaterman_long_affine_mi355x_batch is the throughput form.  For a 128-base seq2 SmithWaterman_affine_mi355x gives
// the same result faster.  SmithWaterman_long_affine_mi355x(a, b, 111-matrix, 1, 1) == SmithWaterman_long_mi355x(a, b, 111-matrix, 1).
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                        const std::vector<uint8_t> &seq2,
                                                                                        const std::array<int8_t, 16> &score_matrix,
                                                                                        int gap_open, int gap_extend);

// Global (Needleman-Wunsch) and free-end-gap alignment of two sequences of any lengths in [1, 16384], any score matrix and
// gap (swmi_global_full: no reference counterpart): (score, path of (i, j) from the start cell to the end cell), forced steps
// along a border that is not free included.  free_ends is a mask of SWMI_FREE_*: SWMI_ENDS_GLOBAL (end to end, from (0, 0) to
// (len1, len2)), SWMI_ENDS_FIT (all of seq1 against a stretch of seq2), SWMI_ENDS_OVERLAP, or any other of the 16.  The score
// may be negative.  One synchronous call per alignment; swmi::NeedlemanWunsch_mi355x_batch is the throughput form, and
// swmi::NeedlemanWunsch_mi355x_ragged_batch the one for mixed lengths.  An empty sequence is taken too (through the ragged
// entry): the table is then one border, and the result the closed form of include/swmi.h.
inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_mi355x(const std::vector<uint8_t> &seq1,
                                                                              const std::vector<uint8_t> &seq2,
                                                                              const std::array<int8_t, 16> &score_matrix,
                                                                              const int8_t gap_penalty,
                                                                              unsigned free_ends = SWMI_ENDS_GLOBAL);

// The same with affine gaps (swmi_global_full_affine: no reference counterpart), a gap of length k costing
// gap_open + (k-1) gap_extend, both in [0, 127]: Gotoh's global alignment under SWMI_ENDS_GLOBAL, fit and overlap alignment
// under the other masks.  NeedlemanWunsch_affine_mi355x(a, b, m, g, g, mask) == NeedlemanWunsch_mi355x(a, b, m, g, mask).
// One synchronous call per alignment; swmi::NeedlemanWunsch_affine_mi355x_batch is the throughput form.
inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::vector<uint8_t> &seq2,
                                                                                     const std::array<int8_t, 16> &score_matrix,
                                                                                     int gap_open, int gap_extend,
                                                                                     unsigned free_ends = SWMI_ENDS_GLOBAL);

// NeedlemanWunsch_mi355x and NeedlemanWunsch_affine_mi355x for lengths in [1, 65536] (swmi_global_long, swmi_global_long_affine):
// the same results, accepted iff max(1, |score|, gaps) * (len1 + len2) <= 2^23 (include/swmi.h), which holds for every shape
// up to 32768 x 32768.  One synchronous call per alignment; swmi::NeedlemanWunsch_long_mi355x_batch and
// swmi::NeedlemanWunsch_long_affine_mi355x_batch are the throughput forms.
inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                   const std::vector<uint8_t> &seq2,
                                                                                   const std::array<int8_t, 16> &score_matrix,
                                                                                   const int8_t gap_penalty,
                                                                                   unsigned free_ends = SWMI_ENDS_GLOBAL);
inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                          const std::vector<uint8_t> &seq2,
                                                                                          const std::array<int8_t, 16> &score_matrix,
                                                                                          int gap_open, int gap_extend,
                                                                                          unsigned free_ends = SWMI_ENDS_GLOBAL);

// SmithWaterman_long_mi355x and SmithWaterman_long_affine_mi355x for lengths in [1, 65536] (swmi_local_long,
// swmi_local_long_affine): the same results, with every int8 matrix and gap at every shape (no domain rule).  One synchronous
// call per alignment; swmi::SmithWaterman_xlong_mi355x_batch and swmi::SmithWaterman_xlong_affine_mi355x_batch are the
// throughput forms.
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_xlong_mi355x(const std::vector<uint8_t> &seq1,
                                                                                  const std::vector<uint8_t> &seq2,
                                                                                  const std::array<int8_t, 16> &score_matrix,
                                                                                  const int8_t gap_penalty);
inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_xlong_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                         const std::vector<uint8_t> &seq2,
                                                                                         const std::array<int8_t, 16> &score_matrix,
                                                                                         int gap_open, int gap_extend);

// SemiGlobal_111's exact semi-global alignment for lengths in [1, 65536], any score matrix and gap (swmi_semiglobal_long,
// swmi_semiglobal_long_affine): (score, path of (i, j) from (0, 0) to the best cell), the results of swmi_semiglobal_full and
// swmi_semiglobal_full_affine field for field, accepted iff max(1, |score|, gaps) * (len1 + len2) <= 2^23 (include/swmi.h), which
// holds for every shape up to 32768 x 32768.  One synchronous call per alignment; swmi::SemiGlobal_long_mi355x_batch and
// swmi::SemiGlobal_long_affine_mi355x_batch are the throughput forms.
inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                              const std::vector<uint8_t> &seq2,
                                                                              const std::array<int8_t, 16> &score_matrix,
                                                                              const int8_t gap_penalty);
inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::vector<uint8_t> &seq2,
                                                                                     const std::array<int8_t, 16> &score_matrix,
                                                                                     int gap_open, int gap_extend);

namespace swmi {

// match 1, mismatch -1 (source.cpp:1786)
inline const std::array<int8_t, 16> &semiglobal_111_matrix()
{
    static const std::array<int8_t, 16> m = {1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1, -1, -1, -1, -1, 1};
    return m;
}

namespace detail {

using Result = std::pair<int, std::vector<std::pair<int, int>>>;

// Throws std::runtime_error("<what>: <the library's last error>") unless rc is SWMI_OK.
inline void check(int rc, const char *what)
{
    if (rc != SWMI_OK) throw std::runtime_error(std::string(what) + ": " + swmi_last_error());
}

// One piece's inputs and outputs; each batch overload sizes and fills the ones its C entry takes.
struct PieceBuffers {
    std::vector<uint8_t> seq1s;                        // seq1s staged back to back
    std::vector<uint64_t> seq1_offsets, move_offsets;  // a ragged piece's layouts
    std::vector<uint8_t> seq2s;                        // seq2s staged back to back (a piece ragged on both sides)
    std::vector<uint64_t> seq2_offsets;
    std::vector<int32_t> scores, ends;
    std::vector<uint64_t> moves;
    std::vector<uint32_t> counts;                      // steps or lengths
};

// Aligns alignments [0, n) in pieces of at most `piece` (0 counts as 1).  align(buf, off, m) runs the C entry for
// [off, off + m) into piece buffers `buf` and throws on failure; expand(buf, k) returns piece-relative result k of the piece
// that `buf` holds.  threads == 0: each piece is expanded on the calling thread before the next is aligned (one set of
// buffers).  threads >= 1: piece p is expanded on min(threads, m) threads while piece p + 1 is aligned (two sets, taken in
// turn).  The first failure -- of align, of an expander or of creating a thread -- is recorded, no piece starts after it,
// every started thread is joined, and then it is rethrown as it was thrown.
template <class Align, class Expand>
std::vector<Result> run_in_pieces(size_t n, size_t piece, unsigned threads, Align align, Expand expand)
{
    if (piece == 0) piece = 1;
    std::vector<Result> out(n);
    PieceBuffers bufs[2];
    std::vector<std::thread> pool;                     // the expanders of the piece before the one being aligned
    std::mutex mu;
    std::exception_ptr failed;
    auto record = [&] {                                // (called in a handler)
        std::lock_guard<std::mutex> lock(mu);
        if (!failed) failed = std::current_exception();
    };
    auto has_failed = [&] {
        std::lock_guard<std::mutex> lock(mu);
        return bool(failed);
    };
    auto join_all = [&] {
        for (auto &th : pool) th.join();
        pool.clear();
    };
    auto expand_range = [&](int buf, size_t off, size_t lo, size_t hi) {
        try {
            for (size_t k = lo; k < hi; ++k) out[off + k] = expand(bufs[buf], k);
        } catch (...) {
            record();
        }
    };
    int b = 0;
    try {
        for (size_t off = 0; off < n && !has_failed(); off += piece) {
            const size_t m = std::min(piece, n - off);
            align(bufs[b], off, m);
            join_all();                                // (the previous piece's expanders, which read the other buffers)
            if (threads == 0) {
                expand_range(b, off, 0, m);
            } else if (!has_failed()) {
                const unsigned use = threads > m ? unsigned(m) : threads;
                for (unsigned t = 0; t < use; ++t) pool.emplace_back(expand_range, b, off, m * t / use, m * (t + 1) / use);
                b ^= 1;
            }
        }
    } catch (...) {
        record();                                      // (align failed, or a thread could not be created)
    }
    join_all();
    if (failed) std::rethrow_exception(failed);
    return out;
}

// The host threads a batch overload expands paths on: 0 = as many as the machine reports, at most 64.
inline unsigned expander_threads(unsigned threads)
{
    if (threads == 0) threads = std::thread::hardware_concurrency();
    return threads < 1 ? 1 : threads > 64 ? 64 : threads;
}

using Sequences = std::vector<std::vector<uint8_t>>;

// The length every sequence of a batch overload with one shape must have.
inline size_t common_length(const Sequences &seqs) { return seqs.empty() ? 0 : seqs[0].size(); }

// Throws std::invalid_argument unless every sequence has the length `len`; `which` is "seq1" or "seq2".
inline void check_lengths(const char *name, const Sequences &seqs, size_t len, const char *which)
{
    for (const auto &s : seqs)
        if (s.size() != len) throw std::invalid_argument(std::string(name) + ": every " + which + " must have the same length");
}

// The batch overloads of the (len1, 128) aligners (swmi_local_align and its affine twin), every seq1 of one length, named
// `name`: in pieces of at most `piece` alignments, each expanded on the calling thread.  call(seq1s, len1, seq2s, m, scores,
// ends, moves, steps) is the C entry `entry` with its parameters bound.
template <class Call, class Expand>
std::vector<Result> local_batch(const char *name, const char *entry, const Sequences &seq1s,
                                const std::vector<std::array<uint8_t, 128>> &seq2s, size_t piece, Call call, Expand expand)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    const size_t len1 = common_length(seq1s), mw = SWMI_LOCAL_MOVE_WORDS(len1);
    check_lengths(name, seq1s, len1, "seq1");
    auto align = [&](PieceBuffers &p, size_t off, size_t m) {
        p.seq1s.resize(m * len1);
        for (size_t k = 0; k < m; ++k) std::copy(seq1s[off + k].begin(), seq1s[off + k].end(), p.seq1s.begin() + k * len1);
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(m * mw);
        p.counts.resize(m);
        check(call(p.seq1s.data(), len1, seq2s[off].data(), m, p.scores.data(), p.ends.data(), p.moves.data(), p.counts.data()),
              entry);
    };
    return run_in_pieces(seq1s.size(), piece, 0, align, [&](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], expand(p.moves.data() + k * mw, p.counts[k], p.ends.data() + 4 * k)};
    });
}

// The batch overloads of the aligners with one (len1, len2) per call, every seq1 of one length and every seq2 of one length,
// named `name`: in pieces of `piece` alignments, at most one traceback slice of the aligner (0 = one slice), both sides of a
// piece staged in one buffer, piece p expanded on `threads` host threads (expander_threads) while piece p + 1 is aligned.
// slices_for is the aligner's *_slices_for; call(seq1s, len1, seq2s, len2, m, scores, ends, moves, counts) is the C entry
// `entry` with its parameters bound; its rows hold `move_words` words and `ends_width` ends.
template <class SlicesFor, class Call, class Expand>
std::vector<Result> shaped_batch(const char *name, const char *entry, const Sequences &seq1s, const Sequences &seq2s, size_t piece,
                                 unsigned threads, size_t ends_width, size_t move_words, SlicesFor slices_for, Call call, Expand expand)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    const size_t len1 = common_length(seq1s), len2 = common_length(seq2s);
    check_lengths(name, seq1s, len1, "seq1");
    check_lengths(name, seq2s, len2, "seq2");
    if (seq1s.empty()) return {};
    size_t slice = 0;
    if (slices_for(seq1s.size(), len1, len2, 1, &slice, 1) == 0)               // (a length out of range: throws the library's error)
        check(call(nullptr, len1, nullptr, len2, 1, nullptr, nullptr, nullptr, nullptr), entry);
    if (piece == 0 || piece > slice) piece = slice;
    auto align = [&](PieceBuffers &p, size_t off, size_t m) {
        p.seq1s.resize(m * (len1 + len2));
        uint8_t *s2 = p.seq1s.data() + m * len1;
        for (size_t k = 0; k < m; ++k) {
            std::copy(seq1s[off + k].begin(), seq1s[off + k].end(), p.seq1s.begin() + k * len1);
            std::copy(seq2s[off + k].begin(), seq2s[off + k].end(), s2 + k * len2);
        }
        p.scores.resize(m);
        p.ends.resize(ends_width * m);
        p.moves.resize(m * move_words);
        p.counts.resize(m);
        check(call(p.seq1s.data(), len1, s2, len2, m, p.scores.data(), p.ends.data(), p.moves.data(), p.counts.data()), entry);
    };
    return run_in_pieces(seq1s.size(), piece, expander_threads(threads), align, [&](const PieceBuffers &p, size_t k) {
        return Result{p.scores[k], expand(p.moves.data() + k * move_words, p.counts[k], p.ends.data() + k * ends_width)};
    });
}

// One alignment through a C entry: call(score, ends, moves, count) is the entry `entry` with its sequences and parameters
// bound (the semi-global entries fill two of the four ends, the X-drop entry none).
template <class Call, class Expand>
Result one_alignment(const char *entry, size_t move_words, Call call, Expand expand)
{
    int32_t score = 0, ends[4] = {0, 0, 0, 0};
    uint32_t count = 0;
    std::vector<uint64_t> moves(move_words);
    check(call(&score, ends, moves.data(), &count), entry);
    return {score, expand(moves.data(), count, ends)};
}

}  // namespace detail

// One local alignment's moves (swmi_local_align) -> the reference's path vector (source.cpp:1571-1575).
inline std::vector<std::pair<int, int>> expand_local_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j)
{
    static_assert(sizeof(std::pair<int, int>) == 2 * sizeof(int32_t), "std::pair<int,int> must be two packed ints");
    std::vector<std::pair<int, int>> path(size_t(steps) + 1);
    detail::check(swmi_local_expand_moves(moves, steps, end_i, end_j, reinterpret_cast<int32_t *>(path.data()), path.size()),
                  "swmi_local_expand_moves");
    return path;
}

// One alignment's moves (swmi_semiglobal_xdrop_moves) -> the reference's traceback vector (source.cpp:1962-1975).
inline std::vector<std::pair<int, int>> expand_moves(const uint64_t *moves, uint32_t length)
{
    static_assert(sizeof(std::pair<int, int>) == 2 * sizeof(int32_t), "std::pair<int,int> must be two packed ints");
    std::vector<std::pair<int, int>> tb(length);
    detail::check(swmi_semiglobal_expand_moves(moves, length, reinterpret_cast<int32_t *>(tb.data()), length), "swmi_semiglobal_expand_moves");
    return tb;
}

// One any-length local alignment's moves (swmi_local_full) -> the reference's path vector (source.cpp:1571-1575).
inline std::vector<std::pair<int, int>> expand_local_full_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j)
{
    static_assert(sizeof(std::pair<int, int>) == 2 * sizeof(int32_t), "std::pair<int,int> must be two packed ints");
    std::vector<std::pair<int, int>> path(size_t(steps) + 1);
    detail::check(swmi_local_full_expand_moves(moves, steps, end_i, end_j, reinterpret_cast<int32_t *>(path.data()), path.size()),
                  "swmi_local_full_expand_moves");
    return path;
}

namespace detail {

// The three expanders as detail::local_batch, shaped_batch and one_alignment call them: (moves row, count, the alignment's ends).
inline std::vector<std::pair<int, int>> local_path(const uint64_t *moves, uint32_t steps, const int32_t *ends)
{
    return expand_local_moves(moves, steps, ends[0], ends[1]);
}
inline std::vector<std::pair<int, int>> semiglobal_path(const uint64_t *moves, uint32_t length, const int32_t *)
{
    return expand_moves(moves, length);
}
inline std::vector<std::pair<int, int>> local_full_path(const uint64_t *moves, uint32_t steps, const int32_t *ends)
{
    return expand_local_full_moves(moves, steps, ends[0], ends[1]);
}
// ... and the long global aligners' (end cells up to (65536, 65536))
inline std::vector<std::pair<int, int>> global_long_path(const uint64_t *moves, uint32_t steps, const int32_t *ends)
{
    std::vector<std::pair<int, int>> path(size_t(steps) + 1);
    detail::check(swmi_global_long_expand_moves(moves, steps, ends[0], ends[1], reinterpret_cast<int32_t *>(path.data()), path.size()),
                  "swmi_global_long_expand_moves");
    return path;
}

// ... and the long local aligners'
inline std::vector<std::pair<int, int>> local_long_path(const uint64_t *moves, uint32_t steps, const int32_t *ends)
{
    std::vector<std::pair<int, int>> path(size_t(steps) + 1);
    detail::check(swmi_local_long_expand_moves(moves, steps, ends[0], ends[1], reinterpret_cast<int32_t *>(path.data()), path.size()),
                  "swmi_local_long_expand_moves");
    return path;
}

// ... and the long semi-global aligners' (lengths up to 131073)
inline std::vector<std::pair<int, int>> semiglobal_long_path(const uint64_t *moves, uint32_t length, const int32_t *)
{
    std::vector<std::pair<int, int>> tb(length);
    detail::check(swmi_semiglobal_long_expand_moves(moves, length, reinterpret_cast<int32_t *>(tb.data()), length),
                  "swmi_semiglobal_long_expand_moves");
    return tb;
}

}  // namespace detail

// Local alignment of seq1s[k] (every one of the same length) against seq2s[k]: result[k] == SmithWaterman_local_mi355x(seq1s[k],
// seq2s[k], score_matrix, gap_penalty).  The batch goes to the GPU in pieces of at most `piece` alignments, so only one piece's
// inputs and moves are staged at a time (not n rows of moves up front); each piece's paths are built on the host.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_local_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 65536)
{
    return detail::local_batch(
        "SmithWaterman_local_mi355x_batch", "swmi_local_align", seq1s, seq2s, piece,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t m, auto... out) {
            return swmi_local_align(a, len1, b, m, score_matrix.data(), gap_penalty, out...);
        },
        detail::local_path);
}

// Affine local alignment of seq1s[k] (every one of the same length) against seq2s[k]: result[k] ==
// SmithWaterman_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend), in pieces of at most `piece` alignments
// as SmithWaterman_local_mi355x_batch.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 65536)
{
    return detail::local_batch(
        "SmithWaterman_affine_mi355x_batch", "swmi_local_align_affine", seq1s, seq2s, piece,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t m, auto... out) {
            return swmi_local_align_affine(a, len1, b, m, score_matrix.data(), gap_open, gap_extend, out...);
        },
        detail::local_path);
}

// Ragged local alignments (swmi_local_align_ragged and its affine twin): seq1s[k] of any length in [0, 16384] against
// seq2s[k], in pieces of at most `piece` alignments, each one call, so only one piece's inputs and moves are staged at a time.
// call(seq1 bytes, offsets, seq2s, m, scores, ends, moves, steps) is the C entry with its parameters bound.
template <class Call>
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> local_ragged_batch(
    const char *name, const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s,
    size_t piece, Call call)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    auto align = [&](detail::PieceBuffers &p, size_t off, size_t m) {
        p.seq1s.clear();
        p.seq1_offsets.assign(1, 0);
        for (size_t k = 0; k < m; ++k) {
            p.seq1s.insert(p.seq1s.end(), seq1s[off + k].begin(), seq1s[off + k].end());
            p.seq1_offsets.push_back(p.seq1s.size());
        }
        if (p.seq1s.empty()) p.seq1s.push_back(0);      // (every seq1 of the piece is empty: a pointer that is never read)
        p.move_offsets.resize(m + 1);
        if (swmi_local_ragged_move_offsets(p.seq1_offsets.data(), m, p.move_offsets.data()) != SWMI_OK)
            throw std::invalid_argument(std::string(name) + ": " + swmi_last_error());
        p.scores.resize(m);
        p.ends.resize(4 * m);
        p.moves.resize(p.move_offsets[m]);
        p.counts.resize(m);
        detail::check(call(p.seq1s.data(), p.seq1_offsets.data(), seq2s[off].data(), m, p.scores.data(), p.ends.data(), p.moves.data(),
                           p.counts.data()),
                      name);
    };
    return detail::run_in_pieces(seq1s.size(), piece, 0, align, [](const detail::PieceBuffers &p, size_t k) {
        return detail::Result{p.scores[k],
                              expand_local_moves(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends[4 * k], p.ends[4 * k + 1])};
    });
}

// Local alignment of seq1s[k] (any lengths, 0 .. 16384) against seq2s[k]: result[k] == SmithWaterman_local_mi355x(seq1s[k],
// seq2s[k], score_matrix, gap_penalty), in ragged calls of at most `piece` alignments (an empty seq1 gives (0, {(0, 0)})).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_local_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 65536)
{
    return local_ragged_batch("SmithWaterman_local_mi355x_ragged_batch", seq1s, seq2s, piece,
                              [&](const uint8_t *a, const uint64_t *o, const uint8_t *b, size_t m, int32_t *sc, int32_t *e, uint64_t *mv,
                                  uint32_t *st) { return swmi_local_align_ragged(a, o, b, m, score_matrix.data(), gap_penalty, sc, e, mv, st); });
}

// The same with affine gaps: result[k] == SmithWaterman_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 65536)
{
    return local_ragged_batch("SmithWaterman_affine_mi355x_ragged_batch", seq1s, seq2s, piece,
                              [&](const uint8_t *a, const uint64_t *o, const uint8_t *b, size_t m, int32_t *sc, int32_t *e, uint64_t *mv,
                                  uint32_t *st) {
                                  return swmi_local_align_affine_ragged(a, o, b, m, score_matrix.data(), gap_open, gap_extend, sc, e, mv, st);
                              });
}

// The reference's SmithWaterman_111_long (source.cpp:1526-1576) over a batch of any seq1 lengths: result[k] ==
// SmithWaterman_111_long(seq1s[k], seq2s[k]).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_111_long_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::array<uint8_t, 128>> &seq2s, size_t piece = 65536)
{
    return SmithWaterman_local_mi355x_ragged_batch(seq1s, seq2s, semiglobal_111_matrix(), 1, piece);
}

// The reference's SpeedtestSemiGlobal loop (source.cpp:2818-2856) over arrays of pairs: result[k] ==
// SemiGlobal_AdaptiveBanded_XDrop_111_32_70(seq1s[k], seq2s[k]).  The GPU returns 2 bits per traceback step (8 KB per
// alignment over PCIe instead of the 262 KB its positions take).  The batch goes to the GPU in pieces of `piece` alignments
// (65536 = two of the library's internal chunks: its copies and kernels overlap inside a call); only two pieces' moves are
// held at a time, and the positions of one piece are rebuilt on `threads` host threads (0 = as many as the machine reports,
// at most 64) while the GPU aligns the next.  A failure in an expander thread is recorded, every thread is joined, and then
// it is thrown.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_mi355x_batch(
    const std::vector<std::array<uint8_t, 16384>> &seq1s, const std::vector<std::array<uint8_t, 16384>> &seq2s, unsigned threads = 0,
    size_t piece = 65536)
{
    static_assert(sizeof(std::array<uint8_t, 16384>) == 16384, "std::array<uint8_t,16384> must be 16384 contiguous bytes");
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument("SemiGlobal_mi355x_batch: seq1s and seq2s differ in length");
    threads = detail::expander_threads(threads);
    const size_t mw = SWMI_SG_MOVE_WORDS;
    auto align = [&](detail::PieceBuffers &p, size_t off, size_t m) {
        p.scores.resize(m);
        p.moves.resize(m * mw);
        p.counts.resize(m);
        detail::check(swmi_semiglobal_xdrop_moves(seq1s[off].data(), seq2s[off].data(), m, p.scores.data(), p.moves.data(), p.counts.data()),
                      "swmi_semiglobal_xdrop_moves");
    };
    return detail::run_in_pieces(seq1s.size(), piece, threads, align, [&](const detail::PieceBuffers &p, size_t k) {
        return detail::Result{p.scores[k], expand_moves(p.moves.data() + k * mw, p.counts[k])};
    });
}

// The reference's SemiGlobal_111 (source.cpp:1776-1834) over arrays of pairs: result[k] == SemiGlobal_111(seq1s[k], seq2s[k]).
// The batch goes to the GPU in pieces of `piece` alignments (256 = one full-size slice of swmi_semiglobal_full); only two
// pieces' moves are held at a time (8 KiB per alignment), and the paths of one piece are rebuilt on `threads` host threads
// (0 = as many as the machine reports, at most 64) while the GPU aligns the next.  A failure in an expander thread is
// recorded, every thread is joined, and then it is thrown.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_111_mi355x_batch(
    const std::vector<std::array<uint8_t, 16384>> &seq1s, const std::vector<std::array<uint8_t, 16384>> &seq2s,
    unsigned threads = 0, size_t piece = 256)
{
    static_assert(sizeof(std::array<uint8_t, 16384>) == 16384, "std::array<uint8_t,16384> must be 16384 contiguous bytes");
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument("SemiGlobal_111_mi355x_batch: seq1s and seq2s differ in length");
    threads = detail::expander_threads(threads);
    const size_t mw = SWMI_SGFULL_MOVE_WORDS(16384, 16384);
    auto align = [&](detail::PieceBuffers &p, size_t off, size_t m) {
        p.scores.resize(m);
        p.ends.resize(2 * m);
        p.moves.resize(m * mw);
        p.counts.resize(m);
        detail::check(swmi_semiglobal_full(seq1s[off].data(), 16384, seq2s[off].data(), 16384, m, semiglobal_111_matrix().data(), 1,
                                           p.scores.data(), p.ends.data(), p.moves.data(), p.counts.data()),
                      "swmi_semiglobal_full");
    };
    return detail::run_in_pieces(seq1s.size(), piece, threads, align, [&](const detail::PieceBuffers &p, size_t k) {
        return detail::Result{p.scores[k], expand_moves(p.moves.data() + k * mw, p.counts[k])};
    });
}

// Affine exact semi-global alignment of seq1s[k] against seq2s[k], every seq1 of one length and every seq2 of one length:
// result[k] == SemiGlobal_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend).  The batch goes to the GPU
// in pieces of `piece` alignments, at most one traceback slice of swmi_semiglobal_full_affine (0 = one slice: 256 at
// 16384 x 16384); only two pieces' moves are held at a time, and the paths of one piece are rebuilt on `threads` host
// threads (0 = as many as the machine reports, at most 64) while the GPU aligns the next.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned threads = 0, size_t piece = 0)
{
    return detail::shaped_batch(
        "SemiGlobal_affine_mi355x_batch", "swmi_semiglobal_full_affine", seq1s, seq2s, piece, threads, 2,
        SWMI_SGFULL_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_semiglobal_full_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_semiglobal_full_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, out...);
        },
        detail::semiglobal_path);
}

// Any-length local alignment of seq1s[k] against seq2s[k], every seq1 of one length and every seq2 of one length:
// result[k] == SmithWaterman_long_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty).  The batch goes to the GPU in pieces
// of `piece` alignments, at most one traceback slice of swmi_local_full (0 = one slice: 256 at 16384 x 16384); only two
// pieces' moves are held at a time, and the paths of one piece are rebuilt on `threads` host threads (0 = as many as the
// machine reports, at most 64) while the GPU aligns the next.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_long_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SmithWaterman_long_mi355x_batch", "swmi_local_full", seq1s, seq2s, piece, threads, 4,
        SWMI_LOCAL_FULL_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_local_full_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_local_full(a, len1, b, len2, m, score_matrix.data(), gap_penalty, out...);
        },
        detail::local_full_path);
}

// Global / free-end-gap alignment of seq1s[k] against seq2s[k], every seq1 of one length and every seq2 of one length:
// result[k] == NeedlemanWunsch_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty, free_ends).  The batch goes to the GPU in
// pieces of `piece` alignments, at most one traceback slice of swmi_global_full (0 = one slice: 256 at 16384 x 16384); only
// two pieces' moves are held at a time, and the paths of one piece are rebuilt on `threads` host threads (0 = as many as the
// machine reports, at most 64) while the GPU aligns the next.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::shaped_batch(
        "NeedlemanWunsch_mi355x_batch", "swmi_global_full", seq1s, seq2s, piece, threads, 4,
        SWMI_GLOBAL_FULL_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_global_full_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_global_full(a, len1, b, len2, m, score_matrix.data(), gap_penalty, free_ends, out...);
        },
        detail::local_full_path);
}

// Affine global / free-end-gap alignment of seq1s[k] against seq2s[k], every seq1 of one length and every seq2 of one length:
// result[k] == NeedlemanWunsch_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend, free_ends).  The batch goes
// to the GPU in pieces of `piece` alignments, at most one traceback slice of swmi_global_full_affine (0 = one slice: 256 at
// 16384 x 16384); only two pieces' moves are held at a time, and the paths of one piece are rebuilt on `threads` host threads
// (0 = as many as the machine reports, at most 64) while the GPU aligns the next.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::shaped_batch(
        "NeedlemanWunsch_affine_mi355x_batch", "swmi_global_full_affine", seq1s, seq2s, piece, threads, 4,
        SWMI_GLOBAL_FULL_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_global_full_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_global_full_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, free_ends, out...);
        },
        detail::local_full_path);
}

// NeedlemanWunsch_mi355x_batch for lengths in [1, 65536]: result[k] == NeedlemanWunsch_long_mi355x(seq1s[k], seq2s[k], ...).  A
// piece is at most one traceback slice of swmi_global_long (0 = one slice: 16 at 65536 x 65536).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_long_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::shaped_batch(
        "NeedlemanWunsch_long_mi355x_batch", "swmi_global_long", seq1s, seq2s, piece, threads, 4,
        SWMI_GLOBAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_global_long_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_global_long(a, len1, b, len2, m, score_matrix.data(), gap_penalty, free_ends, out...);
        },
        detail::global_long_path);
}

// NeedlemanWunsch_affine_mi355x_batch for lengths in [1, 65536]: result[k] == NeedlemanWunsch_long_affine_mi355x(seq1s[k],
// seq2s[k], ...).  A piece is at most one traceback slice of swmi_global_long_affine.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_long_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return detail::shaped_batch(
        "NeedlemanWunsch_long_affine_mi355x_batch", "swmi_global_long_affine", seq1s, seq2s, piece, threads, 4,
        SWMI_GLOBAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_global_long_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_global_long_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, free_ends, out...);
        },
        detail::global_long_path);
}

// Any-length affine local alignment of seq1s[k] against seq2s[k], every seq1 of one length and every seq2 of one length:
// result[k] == SmithWaterman_long_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend).  The batch goes to the
// GPU in pieces of `piece` alignments, at most one traceback slice of swmi_local_full_affine (0 = one slice: 256 at
// 16384 x 16384); only two pieces' moves are held at a time, and the paths of one piece are rebuilt on `threads` host
// threads (0 = as many as the machine reports, at most 64) while the GPU aligns the next.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_long_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SmithWaterman_long_affine_mi355x_batch", "swmi_local_full_affine", seq1s, seq2s, piece, threads, 4,
        SWMI_LOCAL_FULL_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_local_full_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_local_full_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, out...);
        },
        detail::local_full_path);
}

// SmithWaterman_long_mi355x_batch for lengths in [1, 65536]: result[k] == SmithWaterman_xlong_mi355x(seq1s[k], seq2s[k], ...).  A
// piece is at most one traceback slice of swmi_local_long (0 = one slice: 16 at 65536 x 65536).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_xlong_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SmithWaterman_xlong_mi355x_batch", "swmi_local_long", seq1s, seq2s, piece, threads, 4,
        SWMI_LOCAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_local_long_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_local_long(a, len1, b, len2, m, score_matrix.data(), gap_penalty, out...);
        },
        detail::local_long_path);
}

// SmithWaterman_long_affine_mi355x_batch for lengths in [1, 65536]: result[k] == SmithWaterman_xlong_affine_mi355x(seq1s[k],
// seq2s[k], ...).  A piece is at most one traceback slice of swmi_local_long_affine.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_xlong_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SmithWaterman_xlong_affine_mi355x_batch", "swmi_local_long_affine", seq1s, seq2s, piece, threads, 4,
        SWMI_LOCAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_local_long_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_local_long_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, out...);
        },
        detail::local_long_path);
}

// Exact semi-global alignment of seq1s[k] against seq2s[k] for lengths in [1, 65536], every seq1 of one length and every seq2 of
// one length: result[k] == SemiGlobal_long_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty).  A piece is at most one
// traceback slice of swmi_semiglobal_long (0 = one slice: 16 at 65536 x 65536).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_long_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SemiGlobal_long_mi355x_batch", "swmi_semiglobal_long", seq1s, seq2s, piece, threads, 2,
        SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)), swmi_semiglobal_long_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_semiglobal_long(a, len1, b, len2, m, score_matrix.data(), gap_penalty, out...);
        },
        detail::semiglobal_long_path);
}

// The same with affine gaps: result[k] == SemiGlobal_long_affine_mi355x(seq1s[k], seq2s[k], ...).  A piece is at most one
// traceback slice of swmi_semiglobal_long_affine.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_long_affine_mi355x_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return detail::shaped_batch(
        "SemiGlobal_long_affine_mi355x_batch", "swmi_semiglobal_long_affine", seq1s, seq2s, piece, threads, 2,
        SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(detail::common_length(seq1s), detail::common_length(seq2s)),
        swmi_semiglobal_long_affine_slices_for,
        [&](const uint8_t *a, size_t len1, const uint8_t *b, size_t len2, size_t m, auto... out) {
            return swmi_semiglobal_long_affine(a, len1, b, len2, m, score_matrix.data(), gap_open, gap_extend, out...);
        },
        detail::semiglobal_long_path);
}

// Any-length local alignments of mixed shapes (swmi_local_full_ragged and its affine twin): seq1s[k] and seq2s[k] each of any
// length in [0, 16384], in pieces of at most `piece` alignments (0 counts as 4096), each one ragged call, so only two pieces'
// inputs and moves are held at a time; the paths of one piece are rebuilt on `threads` host threads (0 = as many as the
// machine reports, at most 64) while the GPU aligns the next.  call(seq1 bytes, offsets, seq2 bytes, offsets, m, scores,
// ends, moves, counts) is the C entry with its parameters bound; it writes `ends_width` int32 of ends per alignment, and
// path(moves row, count, the alignment's ends) is the family's expander (detail::local_full_path, detail::semiglobal_path).
template <class Call, class Path>
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> full_ragged_batch(
    const char *name, const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, size_t piece,
    unsigned threads, size_t ends_width, Call call, Path path)
{
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument(std::string(name) + ": seq1s and seq2s differ in length");
    if (piece == 0) piece = 4096;
    threads = detail::expander_threads(threads);
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
    auto align = [&](detail::PieceBuffers &p, size_t off, size_t m) {
        stage(seq1s, off, m, p.seq1s, p.seq1_offsets);
        stage(seq2s, off, m, p.seq2s, p.seq2_offsets);
        p.move_offsets.resize(m + 1);
        if (swmi_local_full_ragged_move_offsets(p.seq1_offsets.data(), p.seq2_offsets.data(), m, p.move_offsets.data()) != SWMI_OK)
            throw std::invalid_argument(std::string(name) + ": " + swmi_last_error());
        p.scores.resize(m);
        p.ends.resize(ends_width * m);
        p.moves.resize(p.move_offsets[m] ? p.move_offsets[m] : 1);
        p.counts.resize(m);
        detail::check(call(p.seq1s.data(), p.seq1_offsets.data(), p.seq2s.data(), p.seq2_offsets.data(), m, p.scores.data(),
                           p.ends.data(), p.moves.data(), p.counts.data()),
                      name);
    };
    return detail::run_in_pieces(seq1s.size(), piece, threads, align, [=](const detail::PieceBuffers &p, size_t k) {
        return detail::Result{p.scores[k], path(p.moves.data() + p.move_offsets[k], p.counts[k], p.ends.data() + ends_width * k)};
    });
}

// The local and the global families: four ends per alignment, the path from the end cell (expand_local_full_moves).
template <class Call>
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> local_full_ragged_batch(
    const char *name, const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s, size_t piece,
    unsigned threads, Call call)
{
    return full_ragged_batch(name, seq1s, seq2s, piece, threads, 4, call, detail::local_full_path);
}

// Any-length local alignment of seq1s[k] against seq2s[k], every sequence of a length of its own in [0, 16384]: result[k] ==
// SmithWaterman_long_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty), and (0, {(0, 0)}) when either is empty.
// SmithWaterman_long_mi355x_batch keeps requiring one shape and throws on differing lengths.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_long_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 0, unsigned threads = 0)
{
    return local_full_ragged_batch("SmithWaterman_long_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                   [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                       int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return swmi_local_full_ragged(a, oa, b, ob, m, score_matrix.data(), gap_penalty, sc, e, mv, st);
                                   });
}

// The same with affine gaps: result[k] == SmithWaterman_long_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SmithWaterman_long_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return local_full_ragged_batch("SmithWaterman_long_affine_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                   [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                       int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return swmi_local_full_affine_ragged(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend,
                                                                            sc, e, mv, st);
                                   });
}

// Global / free-end-gap alignment of seq1s[k] against seq2s[k], every sequence of a length of its own in [0, 16384]
// (swmi_global_full_ragged): result[k] == NeedlemanWunsch_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty, free_ends), also
// for an empty sequence, whose table is one border (include/swmi.h has the closed form: not the local aligners' score 0).
// Pieces, moves and threads as in SmithWaterman_long_mi355x_ragged_batch, whose move layout this shares.
// NeedlemanWunsch_mi355x_batch keeps requiring one shape and throws on differing lengths.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return local_full_ragged_batch("NeedlemanWunsch_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                   [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                       int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return swmi_global_full_ragged(a, oa, b, ob, m, score_matrix.data(), gap_penalty, free_ends, sc, e,
                                                                      mv, st);
                                   });
}

// The same with affine gaps: result[k] == NeedlemanWunsch_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend,
// free_ends), also for an empty sequence.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> NeedlemanWunsch_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, unsigned free_ends = SWMI_ENDS_GLOBAL, size_t piece = 0,
    unsigned threads = 0)
{
    return local_full_ragged_batch("NeedlemanWunsch_affine_mi355x_ragged_batch", seq1s, seq2s, piece, threads,
                                   [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc,
                                       int32_t *e, uint64_t *mv, uint32_t *st) {
                                       return swmi_global_full_affine_ragged(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend,
                                                                             free_ends, sc, e, mv, st);
                                   });
}

// Exact semi-global alignment of seq1s[k] against seq2s[k], every sequence of a length of its own in [0, 16384]
// (swmi_semiglobal_full_ragged): result[k] == SemiGlobal_long_mi355x(seq1s[k], seq2s[k], score_matrix, gap_penalty), which with
// semiglobal_111_matrix() and gap 1 is the reference's SemiGlobal_111: the path from (0, 0) to the best cell, and
// (0, {(0, 0)}) when either sequence is empty (one border, all <= 0: include/swmi.h).
// Pieces, moves and threads as in SmithWaterman_long_mi355x_ragged_batch, whose move layout this shares.
// SemiGlobal_111_mi355x_batch and SemiGlobal_affine_mi355x_batch keep requiring one shape.
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_111_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty, size_t piece = 0, unsigned threads = 0)
{
    return full_ragged_batch(
        "SemiGlobal_111_mi355x_ragged_batch", seq1s, seq2s, piece, threads, 2,
        [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc, int32_t *e, uint64_t *mv,
            uint32_t *ln) { return swmi_semiglobal_full_ragged(a, oa, b, ob, m, score_matrix.data(), gap_penalty, sc, e, mv, ln); },
        detail::semiglobal_path);
}

// The same with affine gaps: result[k] == SemiGlobal_affine_mi355x(seq1s[k], seq2s[k], score_matrix, gap_open, gap_extend).
inline std::vector<std::pair<int, std::vector<std::pair<int, int>>>> SemiGlobal_affine_mi355x_ragged_batch(
    const std::vector<std::vector<uint8_t>> &seq1s, const std::vector<std::vector<uint8_t>> &seq2s,
    const std::array<int8_t, 16> &score_matrix, int gap_open, int gap_extend, size_t piece = 0, unsigned threads = 0)
{
    return full_ragged_batch(
        "SemiGlobal_affine_mi355x_ragged_batch", seq1s, seq2s, piece, threads, 2,
        [&](const uint8_t *a, const uint64_t *oa, const uint8_t *b, const uint64_t *ob, size_t m, int32_t *sc, int32_t *e, uint64_t *mv,
            uint32_t *ln) {
            return swmi_semiglobal_full_affine_ragged(a, oa, b, ob, m, score_matrix.data(), gap_open, gap_extend, sc, e, mv, ln);
        },
        detail::semiglobal_path);
}

// The reference's 1M-call loop (source.cpp:3074-3082) over arrays of pairs, on every GPU the library is bound to:
// scores[k] == SmithWaterman(seq1s[k], seq2s[k], score_matrix, gap_penalty).  std::array<uint8_t,128> has no padding, so a
// vector of them IS the concatenated layout the C ABI takes.  With swmi_init(device) it runs on that one GPU, with
// swmi_init_all(G) the batch is cut into G contiguous shards, one host thread and stream set per GPU (swmi_score_batch_multi).
inline std::vector<int32_t> SmithWaterman_mi355x_batch(const std::vector<std::array<uint8_t, 128>> &seq1s,
                                                       const std::vector<std::array<uint8_t, 128>> &seq2s,
                                                       const std::array<int8_t, 16> &score_matrix, const int8_t gap_penalty)
{
    static_assert(sizeof(std::array<uint8_t, 128>) == 128, "std::array<uint8_t,128> must be 128 contiguous bytes");
    if (seq1s.size() != seq2s.size()) throw std::invalid_argument("SmithWaterman_mi355x_batch: seq1s and seq2s differ in length");
    std::vector<int32_t> scores(seq1s.size());
    const uint8_t *a = seq1s.empty() ? nullptr : seq1s[0].data(), *b = seq2s.empty() ? nullptr : seq2s[0].data();
    const int rc = swmi_num_gpus() > 1
                       ? swmi_score_batch_multi(a, b, seq1s.size(), score_matrix.data(), gap_penalty, scores.data())
                       : swmi_score_batch(a, b, seq1s.size(), score_matrix.data(), gap_penalty, scores.data());
    detail::check(rc, "SmithWaterman_mi355x_batch");
    return scores;
}

// Batches per-pair calls: submit() has the reference's argument list and returns a ticket; scores() drains.
class PairQueue {
public:
    PairQueue(size_t max_pairs, const std::array<int8_t, 16> &score_matrix, int8_t gap_penalty)
    {
        detail::check(swmi_queue_create(max_pairs, score_matrix.data(), gap_penalty, &q_), "swmi_queue_create");
    }
    ~PairQueue() { swmi_queue_destroy(q_); }
    PairQueue(const PairQueue &) = delete;
    PairQueue &operator=(const PairQueue &) = delete;

    long long submit(const std::array<uint8_t, 128> &seq1, const std::array<uint8_t, 128> &seq2)
    {
        const long long t = swmi_queue_submit(q_, seq1.data(), seq2.data());
        if (t < 0) throw std::runtime_error(std::string("swmi_queue_submit: ") + swmi_last_error());
        return t;
    }
    // scores()[ticket] == SmithWaterman(seq1, seq2, score_matrix, gap_penalty) of that submit()
    std::vector<int32_t> scores()
    {
        const int32_t *p = nullptr;
        size_t n = 0;
        detail::check(swmi_queue_wait(q_, &p, &n), "swmi_queue_wait");
        return std::vector<int32_t>(p, p + n);
    }
    void reset() { swmi_queue_reset(q_); }

private:
    swmi_queue *q_ = nullptr;
};

}  // namespace swmi

inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_AdaptiveBanded_XDrop_mi355x(const std::array<uint8_t, 16384> &seq1,
                                                                                              const std::array<uint8_t, 16384> &seq2)
{
    return swmi::detail::one_alignment(
        "swmi_semiglobal_xdrop_moves", SWMI_SG_MOVE_WORDS,
        [&](int32_t *sc, int32_t *, uint64_t *mv, uint32_t *ln) {
            return swmi_semiglobal_xdrop_moves(seq1.data(), seq2.data(), 1, sc, mv, ln);
        },
        swmi::detail::semiglobal_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_local_mi355x(const std::vector<uint8_t> &seq1,
                                                                                  const std::array<uint8_t, 128> &seq2,
                                                                                  const std::array<int8_t, 16> &score_matrix,
                                                                                  const int8_t gap_penalty)
{
    return swmi::detail::one_alignment(
        "swmi_local_align", SWMI_LOCAL_MOVE_WORDS(seq1.size()),
        [&](auto... out) {
            return swmi_local_align(seq1.data(), seq1.size(), seq2.data(), 1, score_matrix.data(), gap_penalty, out...);
        },
        swmi::detail::local_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                   const std::array<uint8_t, 128> &seq2,
                                                                                   const std::array<int8_t, 16> &score_matrix,
                                                                                   int gap_open, int gap_extend)
{
    return swmi::detail::one_alignment(
        "swmi_local_align_affine", SWMI_LOCAL_MOVE_WORDS(seq1.size()),
        [&](auto... out) {
            return swmi_local_align_affine(seq1.data(), seq1.size(), seq2.data(), 1, score_matrix.data(), gap_open, gap_extend, out...);
        },
        swmi::detail::local_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_111_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::array<uint8_t, 128> &seq2)
{
    return SmithWaterman_local_mi355x(seq1, seq2, swmi::semiglobal_111_matrix(), 1);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                 const std::vector<uint8_t> &seq2,
                                                                                 const std::array<int8_t, 16> &score_matrix,
                                                                                 const int8_t gap_penalty)
{
    return swmi::detail::one_alignment(
        "swmi_local_full", SWMI_LOCAL_FULL_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_local_full(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_penalty, out...);
        },
        swmi::detail::local_full_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                        const std::vector<uint8_t> &seq2,
                                                                                        const std::array<int8_t, 16> &score_matrix,
                                                                                        int gap_open, int gap_extend)
{
    return swmi::detail::one_alignment(
        "swmi_local_full_affine", SWMI_LOCAL_FULL_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_local_full_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open, gap_extend,
                                          out...);
        },
        swmi::detail::local_full_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_xlong_mi355x(const std::vector<uint8_t> &seq1,
                                                                                  const std::vector<uint8_t> &seq2,
                                                                                  const std::array<int8_t, 16> &score_matrix,
                                                                                  const int8_t gap_penalty)
{
    return swmi::detail::one_alignment(
        "swmi_local_long", SWMI_LOCAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_local_long(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_penalty, out...);
        },
        swmi::detail::local_long_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SmithWaterman_xlong_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                         const std::vector<uint8_t> &seq2,
                                                                                         const std::array<int8_t, 16> &score_matrix,
                                                                                         int gap_open, int gap_extend)
{
    return swmi::detail::one_alignment(
        "swmi_local_long_affine", SWMI_LOCAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_local_long_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open, gap_extend,
                                          out...);
        },
        swmi::detail::local_long_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_mi355x(const std::vector<uint8_t> &seq1,
                                                                              const std::vector<uint8_t> &seq2,
                                                                              const std::array<int8_t, 16> &score_matrix,
                                                                              const int8_t gap_penalty, unsigned free_ends)
{
    // an empty sequence: the fixed-length entry takes no length 0, the ragged one does (one border, include/swmi.h)
    if (seq1.empty() || seq2.empty())
        return swmi::NeedlemanWunsch_mi355x_ragged_batch({seq1}, {seq2}, score_matrix, gap_penalty, free_ends, 1, 1).front();
    return swmi::detail::one_alignment(
        "swmi_global_full", SWMI_GLOBAL_FULL_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_global_full(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_penalty, free_ends,
                                    out...);
        },
        swmi::detail::local_full_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::vector<uint8_t> &seq2,
                                                                                     const std::array<int8_t, 16> &score_matrix,
                                                                                     int gap_open, int gap_extend, unsigned free_ends)
{
    if (seq1.empty() || seq2.empty())                       // as in NeedlemanWunsch_mi355x
        return swmi::NeedlemanWunsch_affine_mi355x_ragged_batch({seq1}, {seq2}, score_matrix, gap_open, gap_extend, free_ends, 1, 1).front();
    return swmi::detail::one_alignment(
        "swmi_global_full_affine", SWMI_GLOBAL_FULL_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_global_full_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open,
                                           gap_extend, free_ends, out...);
        },
        swmi::detail::local_full_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                                   const std::vector<uint8_t> &seq2,
                                                                                   const std::array<int8_t, 16> &score_matrix,
                                                                                   const int8_t gap_penalty, unsigned free_ends)
{
    return swmi::detail::one_alignment(
        "swmi_global_long", SWMI_GLOBAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_global_long(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_penalty, free_ends,
                                    out...);
        },
        swmi::detail::global_long_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> NeedlemanWunsch_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                          const std::vector<uint8_t> &seq2,
                                                                                          const std::array<int8_t, 16> &score_matrix,
                                                                                          int gap_open, int gap_extend, unsigned free_ends)
{
    return swmi::detail::one_alignment(
        "swmi_global_long_affine", SWMI_GLOBAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_global_long_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open,
                                           gap_extend, free_ends, out...);
        },
        swmi::detail::global_long_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_111_mi355x(const std::array<uint8_t, 16384> &seq1,
                                                                             const std::array<uint8_t, 16384> &seq2)
{
    return swmi::detail::one_alignment(
        "swmi_semiglobal_full", SWMI_SGFULL_MOVE_WORDS(16384, 16384),
        [&](auto... out) {
            return swmi_semiglobal_full(seq1.data(), 16384, seq2.data(), 16384, 1, swmi::semiglobal_111_matrix().data(), 1, out...);
        },
        swmi::detail::semiglobal_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                const std::vector<uint8_t> &seq2,
                                                                                const std::array<int8_t, 16> &score_matrix,
                                                                                int gap_open, int gap_extend)
{
    return swmi::detail::one_alignment(
        "swmi_semiglobal_full_affine", SWMI_SGFULL_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_semiglobal_full_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open,
                                               gap_extend, out...);
        },
        swmi::detail::semiglobal_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_long_mi355x(const std::vector<uint8_t> &seq1,
                                                                              const std::vector<uint8_t> &seq2,
                                                                              const std::array<int8_t, 16> &score_matrix,
                                                                              const int8_t gap_penalty)
{
    return swmi::detail::one_alignment(
        "swmi_semiglobal_long", SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_semiglobal_long(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_penalty, out...);
        },
        swmi::detail::semiglobal_long_path);
}

inline std::pair<int, std::vector<std::pair<int, int>>> SemiGlobal_long_affine_mi355x(const std::vector<uint8_t> &seq1,
                                                                                     const std::vector<uint8_t> &seq2,
                                                                                     const std::array<int8_t, 16> &score_matrix,
                                                                                     int gap_open, int gap_extend)
{
    return swmi::detail::one_alignment(
        "swmi_semiglobal_long_affine", SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(seq1.size(), seq2.size()),
        [&](auto... out) {
            return swmi_semiglobal_long_affine(seq1.data(), seq1.size(), seq2.data(), seq2.size(), 1, score_matrix.data(), gap_open,
                                               gap_extend, out...);
        },
        swmi::detail::semiglobal_long_path);
}
