// swmi_internal.h -- declarations shared by the HIP kernels (sw_kernels.hip) and the C-ABI host side (swmi_api.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace swmi {

// The 4x4 int8 score matrix as four dwords: rows.r[a] holds sm[a*4 + 0..3] in bytes 0..3
// (index order of source.cpp:50: seq1 base selects the row, seq2 base the column).
struct SmRows {
    uint32_t r[4];
};

enum ScheduleFlags : unsigned {
    kNoGapFold = 1u,   // never use the gap-folded recurrence
    kUseLut = 4u,      // LDS score-lookup kernel (sw128_lut_kernel)
    kUseI16 = 2u,      // compiler-scheduled 16-bit max variant (v_max_i16 is full rate, but see DESIGN.md section 5)
    kNoPacked = 8u,    // never use the packed kernel (sw128_pk_kernel, what L = 4, 8, 16 run otherwise): A/B against the int32 cell
};

struct LaunchConfig {
    int lanes_per_alignment;   // 64, 32, 16, 8, 4, 2
    bool fold_gap;             // rows carry sm + gap (requires every sm + gap to fit int8)
    bool use_i16;
    unsigned extra_lds_bytes;  // unused dynamic LDS per workgroup: caps workgroups per CU (occupancy sweep, SWMI_EXTRA_LDS)
    bool use_lut;              // LDS score lookup instead of v_dot4 (gap-folded body only, L in {16, 8, 4})
    bool use_pk;               // L = 4, 8 or 16, no other variant asked for: packed kernel, two alignments per register;
    int pk_bias;               //   rows then hold s + gap + pk_bias (bytes 0..255), pk_bias = max(0, -(min s + gap))
    int pk_variant;            //   cell body: 0 = no bias needed, 1 = biased, 2 = vertical-offset form (rows hold s + 2 gap);
                               //   sw_kernels.hip PkVariant
    int pk_flag_unit;          //   variant 2 only, 0 = off: m + gap of its flag form (pk_form.h), which runs variant 0's cell on values
    int pk_flag_gap;           //   rescaled by 255 / (m + gap); rows then hold flag bytes, and this is the rescaled gap
    bool pk_product;           //   the flag form runs as its product form: rows hold the eight 16-bit multipliers (pk_form.h)
};

// Score n pairs resident in device memory. packed = 2-bit inputs (32 B per sequence).
hipError_t launch_score(const LaunchConfig &cfg, const uint8_t *d_seq1s, const uint8_t *d_seq2s, int32_t *d_scores,
                        size_t n, const SmRows &rows, int gap, bool packed, hipStream_t stream);
// Score n_seq1 sequences against one seq2 (device pointers; d_seq2 = 128 bytes).
hipError_t launch_score_one_vs_many(const LaunchConfig &cfg, const uint8_t *d_seq1s, const uint8_t *d_seq2,
                                    int32_t *d_scores, size_t n_seq1, const SmRows &rows, int gap, hipStream_t stream);
// Banded (128 diagonals) affine-gap local alignment of n pairs of `len`-mers (device pointers).
hipError_t launch_banded_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int32_t *d_scores, size_t n, int len,
                                const SmRows &rows, int gap_open, int gap_ext, hipStream_t stream,
                                bool allow_i16 = true,      // false: never the 16-bit-max build (SWMI_BANDED_NO_I16, A/B)
                                bool allow_pk = true);      // false: never the packed kernel (SWMI_BANDED_NO_PK, A/B)
// 2 = sw_banded_affine_pk_kernel (two alignments per wavefront), 1 = the int32 cell with 16-bit maxes, 0 = the int32 cell
int banded_affine_kernel_choice(int len, const SmRows &rows, int gap_open, int gap_ext, bool allow_i16, bool allow_pk);
hipError_t launch_generate(uint8_t *d_seq1s, uint8_t *d_seq2s, size_t n, uint64_t seed, uint64_t first_pair,
                           hipStream_t stream);
// Exhaustive check that v_pk_maximum3_f16 is a packed integer max on [0, 0x7C00)^2 (d_counts: two zeroed 64-bit words:
// comparisons made, comparisons that failed).
hipError_t launch_pk_max3_selftest(unsigned long long *d_counts, hipStream_t stream);
hipError_t launch_unpack(const uint8_t *d_packed, uint8_t *d_unpacked, size_t n_seqs, hipStream_t stream);

bool schedule_supported(int lanes_per_alignment);

// Semi-global adaptive-band X-drop aligner (sg_kernels.hip). Workspace: codes + band rows + summaries for n alignments.
size_t semiglobal_workspace_bytes(size_t n);
// Override of the sweep mapping (swmi_semiglobal_set_mapping; SWMI_SG_SWEEP gives the initial value at swmi_init): -1 = automatic
struct SgTuning {
    int force_sweep = -1;        // G or 10 * G + W (sg_kernels.hip choose_sweep)
    int exact_only = 0;          // 1: no calm windows -- every round runs the X-drop test (A/B and tests; same results either way)
};
hipError_t launch_semiglobal(const uint8_t *d_seq1s, const uint8_t *d_seq2s, size_t n, void *d_workspace,
                             int32_t *d_scores, int32_t *d_tracebacks, size_t cap, uint32_t *d_lengths, hipStream_t stream,
                             hipEvent_t between = nullptr,    // recorded between the sweep and the traceback kernel
                             int compute_units = 256,         // of the device: picks the sweep mapping (wavefronts per SIMD)
                             SgTuning tuning = SgTuning(),
                             unsigned long long *d_moves_out = nullptr);   // non-NULL: the walk's 2-bit moves go here
                                                                           //   ([n][semiglobal_move_words()]); with d_tracebacks
                                                                           //   NULL the expand kernel is skipped
size_t semiglobal_move_words();                  // 64-bit words of moves per alignment (32 moves each)
// Names of the sweep / traceback kernels launch_semiglobal picks for n alignments on a device with that many CUs.
void semiglobal_kernel_names(size_t n, int compute_units, char *sweep_name, size_t sweep_len, char *tb_name, size_t tb_len,
                             SgTuning tuning = SgTuning());

}  // namespace swmi

namespace swmi {
// One slot of a ragged launch of the local aligners (launch_local_ragged, launch_local_affine_ragged): the alignment it
// computes, every field relative to the launch's buffers.  The slots of a wavefront may have different lengths.
struct LocalWork {
    uint32_t k;             // results at index k, seq2 at d_seq2s + 128 k
    uint32_t s1_off;        // seq1 = the len1 bytes at d_seq1s + s1_off (not read when len1 is 0)
    uint32_t len1;          // 0 .. 16384
    uint32_t code_base;     // codes at d_codes + code_base: local_code_words(len1) / local_affine_code_words(len1) dwords
    uint32_t move_base;     // moves at d_moves + move_base: SWMI_LOCAL_MOVE_WORDS(len1) words
};

// Local aligner with end / start cell and traceback (local_kernels.hip).  n alignments of seq1 (len1 bytes each, at
// d_seq1s + len1 * k) against a 128-mer (d_seq2s + 128 k); d_codes holds local_code_words(len1) dwords per alignment of the
// launch.  d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_steps unused).
size_t local_code_words(int len1);
hipError_t launch_local(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, size_t n, const int8_t *sm, int gap,
                        int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                        size_t move_words, hipStream_t stream);
// The same for n slots of d_work (device memory), each of its own length: results at d_scores[work.k] etc.
hipError_t launch_local_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const LocalWork *d_work, size_t n, const int8_t *sm,
                               int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                               uint32_t *d_steps, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Affine-gap local aligner with end / start cell and traceback (local_affine_kernels.hip): launch_local's shapes, with
// local_affine_code_words(len1) dwords of codes per alignment of the launch.
size_t local_affine_code_words(int len1);
hipError_t launch_local_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, size_t n, const int8_t *sm, int gap_open,
                               int gap_extend, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                               uint32_t *d_steps, size_t move_words, hipStream_t stream);
hipError_t launch_local_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const LocalWork *d_work, size_t n,
                                      const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends,
                                      uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Exact semi-global aligner with traceback (sgfull_kernels.hip).  n alignments of seq1 (len1 bytes each, at d_seq1s +
// len1 * k) against seq2 (len2 bytes each, at d_seq2s + len2 * k), one workgroup of sgfull_waves(len2) wavefronts each;
// d_codes holds sgfull_code_words(len1, len2) dwords per alignment of the launch; d_ends two int32 per alignment.
// d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_lengths unused).
int sgfull_waves(int len2);
size_t sgfull_trips(int len1);
size_t sgfull_code_words(int len1, int len2);
hipError_t launch_sgfull(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                         int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                         size_t move_words, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Exact semi-global aligner with AFFINE gaps and traceback (sgfull_affine_kernels.hip): launch_sgfull's shapes and
// workgroups, with sgfull_affine_code_qwords(len1, len2) qwords of codes per alignment of the launch (4 bits per cell).
size_t sgfull_affine_code_qwords(int len1, int len2);
hipError_t launch_sgfull_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                unsigned long long *d_moves, uint32_t *d_lengths, size_t move_words, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Local aligner for two sequences of any length, with end / start cell and traceback (local_full_kernels.hip): launch_sgfull's
// shapes and workgroups, with local_full_code_words(len1, len2) dwords of codes per alignment of the launch; d_ends four
// int32 per alignment.  d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_steps unused).
size_t local_full_code_words(int len1, int len2);
hipError_t launch_local_full(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                             int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                             size_t move_words, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Local aligner for two sequences of any length with AFFINE gaps (local_full_affine_kernels.hip): launch_local_full's shapes,
// workgroups and d_ends, with local_full_affine_code_qwords(len1, len2) qwords of codes per alignment of the launch (4 bits
// per cell).  d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_steps unused).
size_t local_full_affine_code_qwords(int len1, int len2);
hipError_t launch_local_full_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                    int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, size_t move_words, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// One slot of a ragged launch of the any-length local aligners (launch_local_full_ragged, launch_local_full_affine_ragged):
// the alignment its workgroup computes, every field relative to the launch's buffers.  Every field is uniform across the
// workgroup, which reads its slot through blockIdx.x, so the values live in SGPRs.
// Widths: a slice holds at most 2^20 alignments (k), and a length is at most 16384.  The offsets and bases are 64-bit,
// because 32 bits are not enough: a traceback slice of the affine aligner holds up to about 32 GiB of codes (2^35 bytes, 2^33
// dwords), and a slice of 2^20 alignments whose other sequence is empty holds up to 2^34 sequence bytes and no codes at all.
// The planner's budget for a slice is below 2^36 bytes, and a 64-bit field counts that in any unit, so no field can wrap.
struct TileWork {
    uint64_t s1_off;        // seq1 = the len1 bytes at d_seq1s + s1_off (not read when either length is 0)
    uint64_t s2_off;        // seq2 = the len2 bytes at d_seq2s + s2_off (likewise)
    uint64_t code_base;     // codes at d_codes + code_base, in the kernel's code words (dwords; affine: qwords)
    uint64_t move_base;     // moves at d_moves + move_base: SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) words
    uint32_t k;             // results at index k
    uint32_t len1, len2;    // 0 .. 16384 each
    uint32_t pad;           // 0; a ragged STRIPED kernel's slot (wide_long_affine_kernels.hip): its carry block, in units of carry_stride
};

// The wave count of a slot's workgroup, 1 .. 16: one wavefront per 1024 columns; a slot with a zero length runs (and returns
// at once) in a workgroup of one wavefront.
int local_full_ragged_waves(int len1, int len2);
// n slots of d_work (device memory), ALL of wave count `waves`, one workgroup of that many wavefronts each: results at
// d_scores[work.k] etc.  The slice launcher calls it once per wave count present (tile_ragged_api.cpp).
hipError_t launch_local_full_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                    const int8_t *sm, int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);
hipError_t launch_local_full_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                           int waves, const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores,
                                           int32_t *d_ends, unsigned long long *d_codes, unsigned long long *d_moves,
                                           uint32_t *d_steps, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Global and free-end-gap aligner for two sequences of any length (global_full_kernels.hip): launch_local_full's shapes,
// workgroups, codes and d_ends, with free_ends a mask of SWMI_FREE_* (include/swmi.h; above 15: hipErrorInvalidValue).
// d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_steps unused).
size_t global_full_code_words(int len1, int len2);
hipError_t launch_global_full(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              unsigned free_ends, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                              uint32_t *d_steps, size_t move_words, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// Global and free-end-gap aligner with AFFINE gaps (global_full_affine_kernels.hip): launch_global_full's shapes, workgroups,
// d_ends and mask, with global_full_affine_code_qwords(len1, len2) qwords of codes per alignment of the launch (4 bits per
// cell).  d_moves NULL: the ends-only kernel (no codes, no walk; d_codes and d_steps unused).
size_t global_full_affine_code_qwords(int len1, int len2);
hipError_t launch_global_full_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_steps, size_t move_words,
                                     hipStream_t stream);
}  // namespace swmi

namespace swmi {
// The striped global aligners for lengths up to 65536 (global_long_kernels.hip, global_long_affine_kernels.hip; DESIGN.md
// section 23): launch_global_full's / launch_global_full_affine's arguments, shapes up to 65536 x 65536, and d_carry: len1
// dwords (affine: 2 len1) per alignment of the launch, 8-byte aligned, needed when len2 > 16384 and else unused.
size_t global_long_code_words(int len1, int len2);
hipError_t launch_global_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              unsigned free_ends, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves,
                              uint32_t *d_steps, size_t move_words, int32_t *d_carry, hipStream_t stream);
size_t global_long_affine_code_qwords(int len1, int len2);
hipError_t launch_global_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_steps, size_t move_words,
                                     int32_t *d_carry, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// The striped local aligners for lengths up to 65536 (local_long_kernels.hip, local_long_affine_kernels.hip; DESIGN.md section
// 25): launch_local_full's / launch_local_full_affine's arguments, shapes up to 65536 x 65536, and d_carry as for the striped
// global aligners: len1 dwords (affine: 2 len1) per alignment of the launch, 8-byte aligned, needed when len2 > 16384 and else
// unused (may be NULL).
size_t local_long_code_words(int len1, int len2);
hipError_t launch_local_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                             int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps,
                             size_t move_words, int32_t *d_carry, hipStream_t stream);
size_t local_long_affine_code_qwords(int len1, int len2);
hipError_t launch_local_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                    int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                    unsigned long long *d_moves, uint32_t *d_steps, size_t move_words, int32_t *d_carry,
                                    hipStream_t stream);
}  // namespace swmi

namespace swmi {
// The striped semi-global aligners for lengths up to 65536 (sgfull_long_kernels.hip, sgfull_long_affine_kernels.hip; DESIGN.md
// section 26): launch_sgfull's / launch_sgfull_affine's arguments, shapes up to 65536 x 65536, and d_carry as for the striped
// global aligners: len1 dwords (affine: 2 len1) per alignment of the launch, 8-byte aligned, needed when len2 > 16384 and else
// unused (may be NULL).
size_t sgfull_long_code_words(int len1, int len2);
hipError_t launch_sgfull_long(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int gap,
                              int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                              size_t move_words, int32_t *d_carry, hipStream_t stream);
size_t sgfull_long_affine_code_qwords(int len1, int len2);
hipError_t launch_sgfull_long_affine(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                                     int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                     unsigned long long *d_moves, uint32_t *d_lengths, size_t move_words, int32_t *d_carry,
                                     hipStream_t stream);
}  // namespace swmi

namespace swmi {
// The ragged launches of the two global aligners: launch_local_full_ragged's slots, wave counts and
// buffers, with the call's one mask.  A slot with a zero length runs in a workgroup of one wavefront and writes the closed
// form of its one border (tile_sweep.h, end_rule_zero_length): it takes no code words, but its move words.
int global_full_ragged_waves(int len1, int len2);
hipError_t launch_global_full_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                     const int8_t *sm, int gap, unsigned free_ends, int32_t *d_scores, int32_t *d_ends,
                                     uint32_t *d_codes, unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);
hipError_t launch_global_full_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n,
                                            int waves, const int8_t *sm, int gap_open, int gap_extend, unsigned free_ends,
                                            int32_t *d_scores, int32_t *d_ends, unsigned long long *d_codes,
                                            unsigned long long *d_moves, uint32_t *d_steps, hipStream_t stream);
}  // namespace swmi

namespace swmi {
// The ragged launches of the two exact semi-global aligners: launch_local_full_ragged's slots, wave
// counts and buffers, with d_ends two int32 per alignment and d_lengths the path's cells.  A slot with a zero length runs in a
// workgroup of one wavefront and writes score 0, end cell (0, 0) and length 1: it takes no code words and writes no move word.
int sgfull_ragged_waves(int len1, int len2);
hipError_t launch_sgfull_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                const int8_t *sm, int gap, int32_t *d_scores, int32_t *d_ends, uint32_t *d_codes,
                                unsigned long long *d_moves, uint32_t *d_lengths, hipStream_t stream);
hipError_t launch_sgfull_affine_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves,
                                       const int8_t *sm, int gap_open, int gap_extend, int32_t *d_scores, int32_t *d_ends,
                                       unsigned long long *d_codes, unsigned long long *d_moves, uint32_t *d_lengths,
                                       hipStream_t stream);
}  // namespace swmi
