// compat_pieces.cpp -- include/swmi_compat.hpp's batch overloads over stub C entries: no GPU and no library.  The stub aligners
// read alignment k's index from the first four bytes of its seq2, check the seq1 bytes the overload handed over, and write a
// score, end cells, a count and a row of move words derived from k; the stub expanders turn a row back into positions derived
// from k.  One aligner call can be made to fail, and one alignment can be given a count its expander rejects.
// Built and run by tests/test_compat_pieces.py (g++, ASan + UBSan).
//
//   compat_pieces <overload>     local | affine | ragged | affine_ragged | long_ragged | xdrop | sgfull |
//                                long | long_affine | nw | sg_affine
//
// With several pieces and a short last one: every result; the pieces the aligner sees (order, sizes, the entry's arguments);
// the moves buffers it is given (one for the overloads that expand on the calling thread, two in turn for the semi-global
// ones, whose expanders overlap the next call); piece 0 counting as 1; a failing aligner call (std::runtime_error with the
// stub's message, no call after it); a failing expansion in the first piece (std::runtime_error with the stub's message, no
// piece after the one being aligned, on 3 threads for the semi-global overloads); unequal seq1s and seq2s, and for the ragged
// overloads a seq1 the move layout rejects (std::invalid_argument).  The overloads with one (len1, len2) per batch (long,
// long_affine, nw, sg_affine) expand on 3 threads too; their stub *_slices_for report slices of 4, so instead of piece 0
// counting as 1, piece 0 and piece 9 both count as 4; nw's mask reaches every piece; sg_affine's ends are 2 wide, the others' 4;
// a seq1 or seq2 of another length is std::invalid_argument, an empty batch makes no call, and a length the stub refuses
// surfaces as std::runtime_error with its message before any piece is aligned.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "swmi_compat.hpp"

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond);     \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

using Results = std::vector<std::pair<int, std::vector<std::pair<int, int>>>>;

constexpr uint32_t kRejected = 1000;           // a count the stub expanders reject
constexpr size_t kLen1 = 40;                   // the fixed-length overloads' seq1 length
constexpr size_t kLen2 = 88;                   // the seq2 length of the overloads with one (len1, len2)
constexpr size_t kSlice = 4;                   // the slice their stub *_slices_for report

struct Call {                                  // one stub aligner call
    size_t first, n;                           // the index of the piece's first alignment, its alignments
    const uint64_t *moves;
    size_t len1, len2;                         // (ragged: 0, 128)
    std::array<int8_t, 16> sm;
    int gap_open, gap_extend;                  // (a linear gap: the gap twice; X-drop: 0, 0)
    unsigned free_ends;                        // (swmi_global_full only)
};
static std::vector<Call> g_calls;              // aligners run on the calling thread only
static int g_fail_call = -1;                   // the aligner call that fails
static size_t g_reject = SIZE_MAX;             // the alignment whose count the expander rejects
static thread_local std::string g_error;       // swmi_last_error() is per thread, as in the library

static uint32_t index_of(const uint8_t *seq)
{
    uint32_t k;
    memcpy(&k, seq, 4);
    return k;
}
static uint8_t seq1_byte(size_t k, size_t i) { return uint8_t(k * 5 + i); }
static size_t ragged_len(size_t k) { return k / 4 == 1 || k % 5 == 0 ? 0 : 17 * k % 300 + 1; }   // piece [4, 8) all empty
static int32_t score_of(size_t k) { return int32_t(k * 7 % 1000); }
static int32_t end_of(size_t k, int which) { return int32_t(k % 101 + 3 * which); }
static uint32_t count_of(size_t k) { return k == g_reject ? kRejected : uint32_t(k % 37 + 1); }
static std::pair<int, int> position(size_t k, uint32_t t, int32_t end_i, int32_t end_j) { return {int(k) * 100 + end_i, int(t) + end_j}; }

// Logs an aligner call; false, with the stub's error, for the call that fails.
static bool begin_call(const Call &c)
{
    g_calls.push_back(c);
    if (int(g_calls.size()) - 1 != g_fail_call) return true;
    g_error = "stub: call " + std::to_string(g_fail_call) + " fails";
    return false;
}

static void write_row(uint64_t *row, size_t words, size_t k)
{
    CHECK(words >= 4);
    row[0] = k;
    row[1] = ~uint64_t(k);
    row[words - 1] = k;                        // (the row's last word: ASan sees a buffer that is too short)
}

// Alignment k of a row write_row wrote; false, with the stub's error, for a corrupt row or a rejected count.
static bool read_row(const uint64_t *row, uint32_t count, size_t *k)
{
    *k = row[0];
    if (row[1] != ~row[0]) g_error = "stub: corrupt moves row";
    else if (count >= kRejected) g_error = "stub: count " + std::to_string(count) + " rejected for alignment " + std::to_string(*k);
    else return true;
    return false;
}

static void local_results(size_t r, size_t k, int32_t *scores, int32_t *ends, uint32_t *steps)
{
    scores[r] = score_of(k);
    ends[4 * r] = end_of(k, 0);
    ends[4 * r + 1] = end_of(k, 1);
    ends[4 * r + 2] = ends[4 * r + 3] = -7;    // (the start cell: the overloads do not read it)
    steps[r] = count_of(k);
}

static int local_stub(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t *sm, int gap_open, int gap_extend,
                      int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    Call c{index_of(seq2s), n, moves, len1, 128, {}, gap_open, gap_extend};
    memcpy(c.sm.data(), sm, 16);
    if (!begin_call(c)) return SWMI_ERR_HIP;
    for (size_t r = 0; r < n; ++r) {
        const size_t k = index_of(seq2s + 128 * r);
        for (size_t i = 0; i < len1; ++i) CHECK(seq1s[len1 * r + i] == seq1_byte(k, i));
        local_results(r, k, scores, ends, steps);
        write_row(moves + SWMI_LOCAL_MOVE_WORDS(len1) * r, SWMI_LOCAL_MOVE_WORDS(len1), k);
    }
    return SWMI_OK;
}

static int ragged_stub(const uint8_t *seq1s, const uint64_t *offsets, const uint8_t *seq2s, size_t n, const int8_t *sm, int gap_open,
                       int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    if (!seq1s) {
        g_error = "stub: NULL seq1s";
        return SWMI_ERR_INVALID_ARGUMENT;
    }
    Call c{index_of(seq2s), n, moves, 0, 128, {}, gap_open, gap_extend};
    memcpy(c.sm.data(), sm, 16);
    if (!begin_call(c)) return SWMI_ERR_HIP;
    CHECK(offsets[0] == 0);
    for (size_t r = 0, word = 0; r < n; word += SWMI_LOCAL_MOVE_WORDS(offsets[r + 1] - offsets[r]), ++r) {
        const size_t k = index_of(seq2s + 128 * r);
        CHECK(offsets[r + 1] - offsets[r] == ragged_len(k));
        for (size_t i = 0; i < ragged_len(k); ++i) CHECK(seq1s[offsets[r] + i] == seq1_byte(k, i));
        local_results(r, k, scores, ends, steps);
        write_row(moves + word, SWMI_LOCAL_MOVE_WORDS(ragged_len(k)), k);
    }
    return SWMI_OK;
}

static void semiglobal_results(const uint8_t *seq1s, const uint8_t *seq2s, size_t n, size_t mw, int32_t *scores, int32_t *ends,
                               uint64_t *moves, uint32_t *lengths)
{
    for (size_t r = 0; r < n; ++r) {
        const size_t k = index_of(seq2s + 16384 * r);
        CHECK(index_of(seq1s + 16384 * r) == k);
        scores[r] = score_of(k);
        if (ends) {                            // (swmi_semiglobal_full only)
            ends[2 * r] = end_of(k, 0);
            ends[2 * r + 1] = end_of(k, 1);
        }
        lengths[r] = count_of(k);
        write_row(moves + mw * r, mw, k);
    }
}

static bool shaped_in_range(size_t len1, size_t len2) { return len1 >= 1 && len1 <= 16384 && len2 >= 4 && len2 <= 16384; }

// The entries with one (len1, len2) per call; ends_width 2: the semi-global layout, 4: the local one.
static int shaped_stub(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t *sm, int gap_open,
                       int gap_extend, unsigned free_ends, size_t ends_width, int32_t *scores, int32_t *ends, uint64_t *moves,
                       uint32_t *counts)
{
    if (!shaped_in_range(len1, len2)) {
        g_error = "stub: (" + std::to_string(len1) + ", " + std::to_string(len2) + ") is out of range";
        return SWMI_ERR_INVALID_ARGUMENT;
    }
    Call c{index_of(seq2s), n, moves, len1, len2, {}, gap_open, gap_extend, free_ends};
    memcpy(c.sm.data(), sm, 16);
    if (!begin_call(c)) return SWMI_ERR_HIP;
    const size_t mw = SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2);
    for (size_t r = 0; r < n; ++r) {
        const size_t k = index_of(seq2s + len2 * r);
        for (size_t i = 0; i < len1; ++i) CHECK(seq1s[len1 * r + i] == seq1_byte(k, i));
        for (size_t i = 4; i < len2; ++i) CHECK(seq2s[len2 * r + i] == uint8_t(k));
        if (ends_width == 4) {
            local_results(r, k, scores, ends, counts);
        } else {
            scores[r] = score_of(k);
            ends[2 * r] = end_of(k, 0);
            ends[2 * r + 1] = end_of(k, 1);
            counts[r] = count_of(k);
        }
        write_row(moves + mw * r, mw, k);
    }
    return SWMI_OK;
}

// Their *_slices_for as the overloads call it: the first slice only.
static size_t shaped_slices(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    CHECK(traceback == 1 && sizes && cap == 1);
    if (!shaped_in_range(len1, len2)) return 0;
    sizes[0] = std::min(n, kSlice);
    return (n + kSlice - 1) / kSlice;
}

extern "C" {

int swmi_local_align(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                     int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return local_stub(seq1s, len1, seq2s, n, score_matrix, gap_penalty, gap_penalty, scores, ends, moves, steps);
}

int swmi_local_align_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16], int gap_open,
                            int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return local_stub(seq1s, len1, seq2s, n, score_matrix, gap_open, gap_extend, scores, ends, moves, steps);
}

int swmi_local_align_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                            int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return ragged_stub(seq1s, seq1_offsets, seq2s, n, score_matrix, gap_penalty, gap_penalty, scores, ends, moves, steps);
}

int swmi_local_align_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n,
                                   const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                   uint64_t *moves, uint32_t *steps)
{
    return ragged_stub(seq1s, seq1_offsets, seq2s, n, score_matrix, gap_open, gap_extend, scores, ends, moves, steps);
}

int swmi_local_ragged_move_offsets(const uint64_t *seq1_offsets, size_t n, uint64_t *move_offsets)
{
    move_offsets[0] = 0;
    for (size_t r = 0; r < n; ++r) {
        if (seq1_offsets[r + 1] < seq1_offsets[r] || seq1_offsets[r + 1] - seq1_offsets[r] > SWMI_LOCAL_MAX_LEN) {
            g_error = "stub: seq1 " + std::to_string(r) + " of the piece is out of range";
            return SWMI_ERR_INVALID_ARGUMENT;
        }
        move_offsets[r + 1] = move_offsets[r] + SWMI_LOCAL_MOVE_WORDS(seq1_offsets[r + 1] - seq1_offsets[r]);
    }
    return SWMI_OK;
}

int swmi_local_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    size_t k;
    if (!read_row(moves, steps, &k)) return SWMI_ERR_INVALID_ARGUMENT;
    CHECK(cap == size_t(steps) + 1);
    for (uint32_t t = 0; t <= steps; ++t) std::tie(positions[2 * t], positions[2 * t + 1]) = position(k, t, end_i, end_j);
    return SWMI_OK;
}

int swmi_semiglobal_xdrop_moves(const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int32_t *scores, uint64_t *moves, uint32_t *lengths)
{
    if (!begin_call({index_of(seq2s), n, moves, 16384, 16384, {}, 0, 0})) return SWMI_ERR_HIP;
    semiglobal_results(seq1s, seq2s, n, SWMI_SG_MOVE_WORDS, scores, nullptr, moves, lengths);
    return SWMI_OK;
}

int swmi_semiglobal_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                         int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths)
{
    Call c{index_of(seq2s), n, moves, len1, len2, {}, gap_penalty, gap_penalty};
    memcpy(c.sm.data(), score_matrix, 16);
    if (!begin_call(c)) return SWMI_ERR_HIP;
    semiglobal_results(seq1s, seq2s, n, SWMI_SGFULL_MOVE_WORDS(len1, len2), scores, ends, moves, lengths);
    return SWMI_OK;
}

int swmi_semiglobal_expand_moves(const uint64_t *moves, uint32_t length, int32_t *traceback, size_t cap)
{
    size_t k;
    if (!read_row(moves, length, &k)) return SWMI_ERR_INVALID_ARGUMENT;
    CHECK(cap == length);
    for (uint32_t t = 0; t < length; ++t) std::tie(traceback[2 * t], traceback[2 * t + 1]) = position(k, t, 0, 0);
    return SWMI_OK;
}

int swmi_local_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                    int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return shaped_stub(seq1s, len1, seq2s, len2, n, score_matrix, gap_penalty, gap_penalty, 0, 4, scores, ends, moves, steps);
}

int swmi_local_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                           int gap_open, int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return shaped_stub(seq1s, len1, seq2s, len2, n, score_matrix, gap_open, gap_extend, 0, 4, scores, ends, moves, steps);
}

int swmi_global_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n, const int8_t score_matrix[16],
                     int8_t gap_penalty, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps)
{
    return shaped_stub(seq1s, len1, seq2s, len2, n, score_matrix, gap_penalty, gap_penalty, free_ends, 4, scores, ends, moves, steps);
}

int swmi_semiglobal_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                uint64_t *moves, uint32_t *lengths)
{
    return shaped_stub(seq1s, len1, seq2s, len2, n, score_matrix, gap_open, gap_extend, 0, 2, scores, ends, moves, lengths);
}

size_t swmi_local_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return shaped_slices(n, len1, len2, traceback, sizes, cap);
}

size_t swmi_local_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return shaped_slices(n, len1, len2, traceback, sizes, cap);
}

size_t swmi_global_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return shaped_slices(n, len1, len2, traceback, sizes, cap);
}

size_t swmi_semiglobal_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap)
{
    return shaped_slices(n, len1, len2, traceback, sizes, cap);
}

int swmi_local_full_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions, size_t cap)
{
    return swmi_local_expand_moves(moves, steps, end_i, end_j, positions, cap);
}

const char *swmi_last_error(void) { return g_error.c_str(); }

}  // extern "C"

static const std::array<int8_t, 16> kMatrix = {5, -4, -4, -4, -4, 6, -4, -4, -4, -4, 7, -4, -4, -4, -4, 8};

struct Inputs {
    std::vector<std::vector<uint8_t>> seq1s;   // the local overloads
    std::vector<std::array<uint8_t, 128>> seq2s;
    std::vector<std::array<uint8_t, 16384>> sg1, sg2;   // the semi-global overloads
    std::vector<std::vector<uint8_t>> long2s;  // the seq2s of the overloads with one (len1, len2); their seq1s are seq1s
};

struct Overload {
    const char *name;
    const char *batch;                         // the overload's name, as its argument errors give it
    const char *entry;                         // what a failed aligner call's message starts with
    const char *expander;                      // what a failed expansion's message starts with
    bool local, ragged;
    unsigned threads;                          // 0: expanded on the calling thread
    size_t len1, len2;                         // what the entry is given (ragged: 0, 128)
    std::array<int8_t, 16> sm;
    int gap_open, gap_extend;
    Results (*run)(const Inputs &, size_t piece);
    size_t slice = 0;                          // one (len1, len2) per batch: the slice that caps a piece (else 0)
    unsigned free_ends = 0;
};

static const Overload kOverloads[] = {
    {"local", "SmithWaterman_local_mi355x_batch", "swmi_local_align", "swmi_local_expand_moves", true, false, 0, kLen1, 128, kMatrix, 3, 3,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_local_mi355x_batch(in.seq1s, in.seq2s, kMatrix, 3, piece); }},
    {"affine", "SmithWaterman_affine_mi355x_batch", "swmi_local_align_affine", "swmi_local_expand_moves", true, false, 0, kLen1, 128,
     kMatrix, 11, 2,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_affine_mi355x_batch(in.seq1s, in.seq2s, kMatrix, 11, 2, piece); }},
    {"ragged", "SmithWaterman_local_mi355x_ragged_batch", "SmithWaterman_local_mi355x_ragged_batch", "swmi_local_expand_moves", true, true,
     0, 0, 128, kMatrix, 3, 3,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_local_mi355x_ragged_batch(in.seq1s, in.seq2s, kMatrix, 3, piece); }},
    {"affine_ragged", "SmithWaterman_affine_mi355x_ragged_batch", "SmithWaterman_affine_mi355x_ragged_batch", "swmi_local_expand_moves",
     true, true, 0, 0, 128, kMatrix, 11, 2,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_affine_mi355x_ragged_batch(in.seq1s, in.seq2s, kMatrix, 11, 2, piece); }},
    {"long_ragged", "SmithWaterman_local_mi355x_ragged_batch", "SmithWaterman_local_mi355x_ragged_batch", "swmi_local_expand_moves", true,
     true, 0, 0, 128, swmi::semiglobal_111_matrix(), 1, 1,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_111_long_mi355x_batch(in.seq1s, in.seq2s, piece); }},
    {"xdrop", "SemiGlobal_mi355x_batch", "swmi_semiglobal_xdrop_moves", "swmi_semiglobal_expand_moves", false, false, 3, 16384, 16384, {},
     0, 0, [](const Inputs &in, size_t piece) { return swmi::SemiGlobal_mi355x_batch(in.sg1, in.sg2, 3, piece); }},
    {"sgfull", "SemiGlobal_111_mi355x_batch", "swmi_semiglobal_full", "swmi_semiglobal_expand_moves", false, false, 3, 16384, 16384,
     swmi::semiglobal_111_matrix(), 1, 1, [](const Inputs &in, size_t piece) { return swmi::SemiGlobal_111_mi355x_batch(in.sg1, in.sg2, 3, piece); }},
    {"long", "SmithWaterman_long_mi355x_batch", "swmi_local_full", "swmi_local_full_expand_moves", true, false, 3, kLen1, kLen2, kMatrix, 3,
     3, [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_long_mi355x_batch(in.seq1s, in.long2s, kMatrix, 3, piece, 3); },
     kSlice},
    {"long_affine", "SmithWaterman_long_affine_mi355x_batch", "swmi_local_full_affine", "swmi_local_full_expand_moves", true, false, 3,
     kLen1, kLen2, kMatrix, 11, 2,
     [](const Inputs &in, size_t piece) { return swmi::SmithWaterman_long_affine_mi355x_batch(in.seq1s, in.long2s, kMatrix, 11, 2, piece, 3); },
     kSlice},
    {"nw", "NeedlemanWunsch_mi355x_batch", "swmi_global_full", "swmi_local_full_expand_moves", true, false, 3, kLen1, kLen2, kMatrix, 3, 3,
     [](const Inputs &in, size_t piece) { return swmi::NeedlemanWunsch_mi355x_batch(in.seq1s, in.long2s, kMatrix, 3, SWMI_ENDS_FIT, piece, 3); },
     kSlice, SWMI_ENDS_FIT},
    {"sg_affine", "SemiGlobal_affine_mi355x_batch", "swmi_semiglobal_full_affine", "swmi_semiglobal_expand_moves", false, false, 3, kLen1,
     kLen2, kMatrix, 11, 2,
     [](const Inputs &in, size_t piece) { return swmi::SemiGlobal_affine_mi355x_batch(in.seq1s, in.long2s, kMatrix, 11, 2, 3, piece); },
     kSlice},
};

static Inputs inputs(const Overload &o, size_t n)
{
    Inputs in;
    for (uint32_t k = 0; k < n; ++k) {
        if (o.local || o.slice) {
            in.seq1s.emplace_back(o.ragged ? ragged_len(k) : kLen1);
            for (size_t i = 0; i < in.seq1s[k].size(); ++i) in.seq1s[k][i] = seq1_byte(k, i);
        }
        if (o.slice) {
            in.long2s.emplace_back(kLen2, uint8_t(k));
            memcpy(in.long2s[k].data(), &k, 4);
        } else if (o.local) {
            in.seq2s.emplace_back();
            in.seq2s[k].fill(uint8_t(k));
            memcpy(in.seq2s[k].data(), &k, 4);
        } else {
            in.sg1.emplace_back();
            in.sg2.emplace_back();
            in.sg1[k].fill(uint8_t(k));
            in.sg2[k].fill(uint8_t(k + 1));
            memcpy(in.sg1[k].data(), &k, 4);
            memcpy(in.sg2[k].data(), &k, 4);
        }
    }
    return in;
}

static Results expected(const Overload &o, size_t n)
{
    Results want(n);
    for (size_t k = 0; k < n; ++k) {
        want[k].first = score_of(k);
        for (uint32_t t = 0; t < count_of(k) + (o.local ? 1 : 0); ++t)
            want[k].second.push_back(o.local ? position(k, t, end_of(k, 0), end_of(k, 1)) : position(k, t, 0, 0));
    }
    return want;
}

static void reset()
{
    g_calls.clear();
    g_fail_call = -1;
    g_reject = SIZE_MAX;
}

// Runs f, which must throw E with the message `what`.
template <class E, class F>
static void expect_throw(F f, const std::string &what)
{
    try {
        f();
    } catch (const E &e) {
        if (e.what() == what) return;
        fprintf(stderr, "wrong message: \"%s\", expected \"%s\"\n", e.what(), what.c_str());
        exit(1);
    }
    fprintf(stderr, "expected an exception with \"%s\"\n", what.c_str());
    exit(1);
}

static void run(const Overload &o)
{
    reset();                                   // 11 alignments in pieces of 4, 4 and 3
    CHECK(o.run(inputs(o, 11), 4) == expected(o, 11));
    CHECK(g_calls.size() == 3);
    std::set<const uint64_t *> buffers;
    for (size_t c = 0; c < 3; ++c) {
        const Call &call = g_calls[c];
        CHECK(call.first == 4 * c && call.n == (c < 2 ? 4u : 3u));
        CHECK(call.len1 == o.len1 && call.len2 == o.len2 && call.sm == o.sm && call.gap_open == o.gap_open && call.gap_extend == o.gap_extend);
        CHECK(call.free_ends == o.free_ends);
        CHECK(o.threads == 0 || c == 0 || call.moves != g_calls[c - 1].moves);
        buffers.insert(call.moves);
    }
    CHECK(o.ragged || buffers.size() <= (o.threads ? 2u : 1u));
    printf("%s pieces: ok\n", o.name);

    if (o.slice) {                             // piece 0 and a piece above the slice both count as one slice
        for (size_t piece : {size_t(0), size_t(9)}) {
            reset();
            CHECK(o.run(inputs(o, 11), piece) == expected(o, 11));
            CHECK(g_calls.size() == 3 && g_calls[0].n == o.slice && g_calls[1].n == o.slice && g_calls[2].n == 11 - 2 * o.slice);
            CHECK(g_calls[0].free_ends == o.free_ends && g_calls[2].free_ends == o.free_ends);
        }
    } else {
        reset();
        CHECK(o.run(inputs(o, 3), 0) == expected(o, 3));
        CHECK(g_calls.size() == 3 && g_calls[0].n == 1 && g_calls[1].n == 1 && g_calls[2].n == 1);
    }
    printf("%s piece 0: ok\n", o.name);

    reset();
    g_fail_call = 1;
    expect_throw<std::runtime_error>([&] { o.run(inputs(o, 11), 4); }, std::string(o.entry) + ": stub: call 1 fails");
    CHECK(g_calls.size() == 2);
    printf("%s aligner failure: ok\n", o.name);

    reset();
    g_reject = 1;
    expect_throw<std::runtime_error>([&] { o.run(inputs(o, 11), 4); },
                                     std::string(o.expander) + ": stub: count 1000 rejected for alignment 1");
    CHECK(g_calls.size() == 1 || (o.threads && g_calls.size() == 2));   // (the next piece may be aligned while piece 0 expands)
    printf("%s expander failure: ok\n", o.name);

    reset();
    Inputs in = inputs(o, 5);
    if (o.slice)
        in.long2s.pop_back();
    else if (o.local)
        in.seq2s.pop_back();
    else
        in.sg2.pop_back();
    expect_throw<std::invalid_argument>([&] { o.run(in, 4); }, std::string(o.batch) + ": seq1s and seq2s differ in length");
    CHECK(g_calls.empty());
    if (o.ragged) {
        in = inputs(o, 11);
        in.seq1s[5].resize(SWMI_LOCAL_MAX_LEN + 1);
        expect_throw<std::invalid_argument>([&] { o.run(in, 4); }, std::string(o.batch) + ": stub: seq1 1 of the piece is out of range");
        CHECK(g_calls.size() == 1);
    }
    if (o.slice) {
        in = inputs(o, 5);
        in.seq1s[2].push_back(0);
        expect_throw<std::invalid_argument>([&] { o.run(in, 4); }, std::string(o.batch) + ": every seq1 must have the same length");
        in = inputs(o, 5);
        in.long2s[4].pop_back();
        expect_throw<std::invalid_argument>([&] { o.run(in, 4); }, std::string(o.batch) + ": every seq2 must have the same length");
        CHECK(o.run(Inputs(), 4).empty());
        in = inputs(o, 5);
        for (auto &seq1 : in.seq1s) seq1.resize(16385);
        expect_throw<std::runtime_error>([&] { o.run(in, 4); }, std::string(o.entry) + ": stub: (16385, 88) is out of range");
        CHECK(g_calls.empty());
    }
    printf("%s argument errors: ok\n", o.name);
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
    for (const Overload &o : kOverloads)
        if (argv[1] == std::string(o.name)) {
            run(o);
            printf("compat pieces ok\n");
            return 0;
        }
    CHECK(!"unknown overload");
}
