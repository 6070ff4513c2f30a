/*
 * swmi.h -- C ABI of the MI355X-native batched Smith-Waterman scorer (libswmi.so).
 *
 * Drop-in boundary for ONE path of eukaryo/smith-waterman-simd: the fixed-shape
 * (128 x 128, 2-bit alphabet held one base per byte, 4x4 int8 score matrix, linear gap,
 * score only) Smith-Waterman scorer.  The reference has no FFI layer; its boundary is
 * the free-function signature
 *
 *     int SmithWaterman_simdN(const std::array<uint8_t,128>& seq1,
 *                             const std::array<uint8_t,128>& seq2,
 *                             const std::array<int8_t,16>&  score_matrix,
 *                             const int8_t gap_penalty);
 *
 * (source.cpp:35-39 scalar, :462-466 simd4, :758-762 simd7, :953-957 simd9).  Every entry
 * point below cites the reference interface it replaces.  Semantics are those of the
 * scalar SmithWaterman (source.cpp:49-53) in int32:
 *
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)
 *     score  = max over the 128 x 128 cells
 *
 * Valid domain (bit-exact with the reference scalar, and with simd..simd8 wherever those
 * are themselves valid): every score_matrix entry in [-128,127], gap_penalty in [0,127].
 * Bases are taken modulo 4 (the reference indexes out of range for bases >= 4).
 * gap_penalty < 0 is rejected with SWMI_ERR_DOMAIN.
 *
 * There is NO CPU fallback: every scoring entry point runs hand-written gfx950 HIP kernels
 * and fails with an error code when no MI355X-class (gfx950) device is usable.
 *
 * Plain C: pointers and sizes only, no C++/torch types.
 */
#ifndef SWMI_H
#define SWMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define SWMI_API __attribute__((visibility("default")))
#else
#define SWMI_API
#endif

#define SWMI_SEQ_LEN 128        /* std::array<uint8_t,128>, source.cpp:463-464 */
#define SWMI_PACKED_LEN 32      /* std::array<uint8_t,32>,  source.cpp:1580     */
#define SWMI_VERSION 300

enum swmi_status {
    SWMI_OK = 0,
    SWMI_ERR_NOT_INITIALIZED = -1,
    SWMI_ERR_NO_DEVICE = -2,         /* no HIP device / HIP runtime unusable            */
    SWMI_ERR_UNSUPPORTED_ARCH = -3,  /* device is not gfx950                             */
    SWMI_ERR_INVALID_ARGUMENT = -4,  /* NULL pointer, bad size, unknown schedule ...     */
    SWMI_ERR_DOMAIN = -5,            /* gap_penalty < 0                                  */
    SWMI_ERR_ALIGNMENT = -6,         /* device pointer not 16-byte aligned               */
    SWMI_ERR_HIP = -7,               /* a HIP call failed; text in swmi_last_error()     */
    SWMI_ERR_QUEUE_FULL = -8
};

/* ---- lifetime -----------------------------------------------------------------------
 *
 * The library keeps one CONTEXT per bound GPU (streams, staging buffers, workspaces).  Two ways to run:
 *   one process per GPU   swmi_init(device): one context; what bench.py's ranks and every single-GPU caller use
 *   one process, G GPUs   swmi_init_all(G) / swmi_init_devices(list): G contexts, index 0..G-1; the *_multi and
 *                         swmi_sharded_* entry points below split a batch over them
 * Every single-GPU entry point addresses the context the calling THREAD has selected with swmi_use_gpu(index)
 * (default: index 0) and makes that context's device current (hipSetDevice) before it touches HIP -- the model of
 * hipSetDevice itself.  The reference has no counterpart (a single-threaded CPU program, source.cpp:3275-3301). */

/* Bind the process to one GPU (device = ordinal as seen by HIP, or -1 for "LOCAL_RANK env var if set, else 0").
 * Idempotent for the same device; another device needs swmi_shutdown() first. */
SWMI_API int swmi_init(int device);
/* Bind the first n_gpus visible devices (n_gpus <= 0: all of them).  Returns the number of contexts (> 0) or a negative
 * swmi_status; every device must be gfx950.  Enables peer access between the bound devices where the platform allows. */
SWMI_API int swmi_init_all(int n_gpus);
/* Bind an explicit list.  A device may appear more than once -- two contexts on one GPU behave like two GPUs that share
 * the hardware (how the multi-GPU path is rehearsed on a one-GPU box). */
SWMI_API int swmi_init_devices(const int *devices, int n);
SWMI_API int swmi_num_gpus(void);                 /* number of contexts (0 before init) */
SWMI_API int swmi_use_gpu(int index);             /* select the context this thread's single-GPU calls address */
/* Releases every context (streams, staging buffers, workspaces).  Must not race with other calls into the library.
 * Handles created earlier (swmi_queue, swmi_sharded_batch) stay valid OBJECTS: every call on one returns
 * SWMI_ERR_NOT_INITIALIZED from now on -- also after a new swmi_init* -- and its *_destroy call still releases what the
 * handle owns.  Destroy handles before shutting down where you can; you do not have to (a garbage-collected binding cannot
 * promise the order). */
SWMI_API int swmi_shutdown(void);
/* Text of the last error on the calling thread ("" if none). Never NULL. */
SWMI_API const char *swmi_last_error(void);
SWMI_API int swmi_version(void);

/* ---- scoring ------------------------------------------------------------------------ */

/* Replaces a call to SmithWaterman / SmithWaterman_simd .. _simd9
 * (source.cpp:35-39, :462-466, :758-762, :953-957; call sites :2961-2970, :3077, :3212).
 * std::array<>::data() passes straight through.  Synchronous: one launch per call, so it
 * is correct but launch-latency bound -- use the batch or queue entry points for
 * throughput.  Returns the score (>= 0) or a negative swmi_status. */
SWMI_API int swmi_score_pair(const uint8_t seq1[SWMI_SEQ_LEN], const uint8_t seq2[SWMI_SEQ_LEN],
                             const int8_t score_matrix[16], int8_t gap_penalty);

/* The reference's 1M-call loop (source.cpp:3074-3082: `for 1,000,000: score = simd4(a,b,sm,gap)`)
 * as ONE call: pair k is the 128 bytes at seq1s + 128*k and seq2s + 128*k (the per-pair
 * layout of std::array<uint8_t,128>, concatenated).  Host buffers (pageable or pinned).  The PCIe link bounds this entry
 * (256 B per pair in, against ~1 ns of kernel time per pair), so the batch goes through the GPU in GRANULES on a few device
 * buffer sets with a stream each: granule k's kernel runs while granule k+1 is being copied in, and the granules TAPER by the
 * ratio of kernel time to copy time per pair, so that no kernel is still running when the next granule has landed and
 * almost nothing is left to compute when the last copy ends: at 256 B per pair each granule is three quarters of what is
 * left (1M pairs at most, 16K at least: a 1M-pair batch goes as 768K, 192K, 48K, 16K); the one-vs-many entry (128 B per
 * pair) halves; the 2-bit packed entry (64 B per pair), whose copy and kernel take the same time, uses near-equal granules
 * (DESIGN.md section 6).  The scores come back in ONE copy per 16M pairs after the last kernel -- a copy into pageable
 * memory blocks the caller until the stream reaches it, so copying scores back behind
 * every granule (round 2) serialised copy and kernel.  swmi_host_granules_for() reports the schedule.  The copies are issued
 * straight from the caller's memory (the HIP runtime stages pageable pages itself; an extra copy into library-owned pinned
 * memory measured slower); batches of up to 64 pairs go through a pinned, device-visible buffer
 * instead (no copy commands at all).  Thread-safe: calls on one context serialise.
 * scores[k] receives what SmithWaterman(seq1_k, seq2_k, score_matrix, gap) returns.
 * n may be 0.  Returns SWMI_OK or a negative swmi_status. */
SWMI_API int swmi_score_batch(const uint8_t *seq1s, const uint8_t *seq2s, size_t n,
                              const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores);

/* The granules a host batch of n pairs is cut into (the pipeline above), in order; returns how many there are and writes
 * the first `cap` sizes to granules (NULL to count).  Needs no device. */
SWMI_API size_t swmi_host_granules(size_t n, size_t *granules, size_t cap);

/* The same for any of the three host-batch entries: SWMI_ENTRY_PAIRS = swmi_score_batch (256 B per pair over the link;
 * what swmi_host_granules reports), SWMI_ENTRY_PACKED = swmi_score_batch_packed (64 B), SWMI_ENTRY_ONE_VS_MANY =
 * swmi_score_one_vs_many (128 B).  Returns 0 for an unknown entry.  Needs no device. */
#define SWMI_ENTRY_PAIRS 0
#define SWMI_ENTRY_PACKED 1
#define SWMI_ENTRY_ONE_VS_MANY 2
SWMI_API size_t swmi_host_granules_for(size_t n, int entry, size_t *granules, size_t cap);

/* Same contract with all three buffers already resident in device memory (16-byte aligned
 * device pointers; `stream` is a hipStream_t, NULL meaning the HIP null stream as usual).
 * Asynchronous: returns after the launch; the caller synchronises the stream.  This is the
 * entry bench.py times (inputs resident in HBM). */
SWMI_API int swmi_score_batch_device(const void *d_seq1s, const void *d_seq2s, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty,
                                     void *d_scores, void *stream);

/* One-vs-many shape of SmithWaterman_8b111x32mark1/2/3 (source.cpp:1227-1230: 32 seq1 x one
 * seq2 -> int[32]) generalised to n_seq1 sequences and arbitrary parameters:
 * scores[k] = SmithWaterman(seq1s + 128*k, seq2, sm, gap).  Host buffers. */
SWMI_API int swmi_score_one_vs_many(const uint8_t *seq1s, size_t n_seq1, const uint8_t seq2[SWMI_SEQ_LEN],
                                    const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores);

/* Same, device-resident (d_seq1s: n_seq1 x 128 bytes, d_seq2: 128 bytes, 16-byte aligned), asynchronous on `stream`. */
SWMI_API int swmi_score_one_vs_many_device(const void *d_seq1s, size_t n_seq1, const void *d_seq2,
                                           const int8_t score_matrix[16], int8_t gap_penalty,
                                           void *d_scores, void *stream);

/* 2-bit packed inputs in the reference's own wire format (unpack(), source.cpp:1580-1583:
 * base k of byte i = (src[i] >> 2k) & 3): pair k is the 32 bytes at seq1s_packed + 32*k.
 * The kernel unpacks on the fly (no unpacked copy in HBM).  Host buffers.  64 B per pair over the link: copy and kernel
 * take the same time, so this entry runs near-equal granules and issues them from TWO host threads -- the caller's and a
 * persistent helper the context creates on first use -- so that one copy command's DMA runs while the other thread
 * prepares the next (SWMI_HOST_THREADS=1 in the environment keeps everything on the calling thread). */
SWMI_API int swmi_score_batch_packed(const uint8_t *seq1s_packed, const uint8_t *seq2s_packed, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores);
SWMI_API int swmi_score_batch_packed_device(const void *d_seq1s_packed, const void *d_seq2s_packed, size_t n,
                                            const int8_t score_matrix[16], int8_t gap_penalty,
                                            void *d_scores, void *stream);

/* ---- multi-GPU: one batch over the G bound GPUs -----------------------------------------
 * The reference's 1M-call loop (source.cpp:3074-3082) pointed at G GPUs.  Pairs are independent, so shard g of G is the
 * contiguous range swmi_shard_bounds(n, g, G) (shards differ by at most one pair) and the only exchange step is the
 * final gather of the int32 scores.  No input byte ever crosses GPUs. */
SWMI_API int swmi_shard_bounds(size_t n, int shard, int n_shards, size_t *lo, size_t *hi);   /* needs no device */

/* swmi_score_batch / swmi_score_batch_packed over every bound GPU: one host thread and one stream set per GPU, each
 * copying its shard in, scoring it and copying its scores straight into the caller's slice scores[lo..hi). */
SWMI_API int swmi_score_batch_multi(const uint8_t *seq1s, const uint8_t *seq2s, size_t n,
                                    const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores);
SWMI_API int swmi_score_batch_packed_multi(const uint8_t *seq1s_packed, const uint8_t *seq2s_packed, size_t n,
                                           const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores);

/* A batch whose shards stay RESIDENT on the GPUs (what a multi-GPU caller times): shard g of the inputs and of the scores
 * lives in GPU g's HBM; swmi_sharded_score launches every GPU's kernel on that GPU's own stream and then runs the gather:
 *   SWMI_GATHER_NONE   scores stay sharded (read them with swmi_sharded_scores_host)
 *   SWMI_GATHER_ROOT   every GPU pushes its shard into the full int32[n] vector on GPU 0 (peer-to-peer DMA over xGMI)
 *   SWMI_GATHER_ALL    every GPU ends up with the full vector: RCCL (librccl, loaded on first use; ncclAllGather for
 *                      equal shards, grouped ncclBroadcast for ragged ones); peer copies when a GPU is bound twice
 * All calls are asynchronous until swmi_sharded_wait. */
typedef struct swmi_sharded_batch swmi_sharded_batch;
enum swmi_gather { SWMI_GATHER_NONE = 0, SWMI_GATHER_ROOT = 1, SWMI_GATHER_ALL = 2 };
SWMI_API int swmi_sharded_create(size_t n, int packed, swmi_sharded_batch **out);
SWMI_API int swmi_sharded_destroy(swmi_sharded_batch *b);
/* inputs: generated on each GPU from (seed, first_pair + global pair index), or copied from host arrays of n pairs */
SWMI_API int swmi_sharded_generate(swmi_sharded_batch *b, uint64_t seed, uint64_t first_pair);
SWMI_API int swmi_sharded_upload(swmi_sharded_batch *b, const uint8_t *seq1s, const uint8_t *seq2s);
SWMI_API int swmi_sharded_score(swmi_sharded_batch *b, const int8_t score_matrix[16], int8_t gap_penalty, int gather);
SWMI_API int swmi_sharded_wait(swmi_sharded_batch *b);
/* scores[0..n) in pair order from the shards (synchronous, D2H from every GPU into its slice) */
SWMI_API int swmi_sharded_scores_host(swmi_sharded_batch *b, int32_t *scores);
/* device pointer of the gathered int32[n] vector on GPU `index` (valid after a score call with ROOT (index 0) / ALL) */
SWMI_API int swmi_sharded_gathered_device(swmi_sharded_batch *b, int index, void **d_scores);
/* the same vector copied to host memory (synchronous): what GPU `index` holds after the gather */
SWMI_API int swmi_sharded_gathered_host(swmi_sharded_batch *b, int index, int32_t *scores);
/* What SWMI_GATHER_ALL runs on for this batch: 2 = RCCL, 1 = peer copies (a GPU bound twice, librccl not loadable,
 * ncclCommInitAll failed, or SWMI_GATHER_BACKEND=p2p), 0 = not decided yet (no SWMI_GATHER_ALL call so far).  Falling back
 * to peer copies is not an error (same bytes), but it is never silent: the call that decides leaves the reason in
 * swmi_last_error() while returning SWMI_OK, and swmi_sharded_gather_note() returns it at any later time ("" while RCCL
 * is in use or nothing is decided). */
SWMI_API int swmi_sharded_gather_backend(swmi_sharded_batch *b);
SWMI_API int swmi_sharded_gather_note(swmi_sharded_batch *b, char *text, size_t text_len);
/* 1 if librccl can be loaded with every entry point the gather needs, else 0 with the loader's reason in `why`.  Needs no
 * device.  (The library is dlopen()ed on first use, never linked; SWMI_RCCL_LIB names another file to load.) */
SWMI_API int swmi_rccl_probe(char *why, size_t why_len);
/* Measurement: `iters` score calls back to back; kernel_ms[g] = average kernel time of GPU g (HIP events on its stream),
 * gather_ms[g] = average time from the end of GPU g's kernel to the end of its part of the gather, *wall_ms = host wall
 * time per call, everything drained.  kernel_ms / gather_ms have swmi_num_gpus() entries (NULL to skip). */
SWMI_API int swmi_sharded_time(swmi_sharded_batch *b, const int8_t score_matrix[16], int8_t gap_penalty, int gather,
                               int iters, float *kernel_ms, float *gather_ms, double *wall_ms);

/* ---- extension: banded affine-gap scoring (BASELINE.json configs[4]; NO reference counterpart) -----------
 * The reference has linear gaps and no band on this path, so this entry point replaces
 * nothing in source.cpp; its semantics are defined by oracle/sw_oracle.c sw_oracle_banded_affine() and its
 * parity is NOT pinned by the reference.  n pairs of `len`-mers (64 <= len <= 1792, pair k at byte offset
 * len*k), local alignment restricted to the 128 diagonals -64 <= j - i <= 63, a gap of length k costs
 * gap_open + (k-1)*gap_extend (both in [0,127]).  One wavefront per alignment -- or per TWO alignments that share every
 * register as 16-bit halves (sw_banded_affine_pk_kernel, round 4) where len * max(s, 0) + 18 max(0, -min s) + gap_open +
 * gap_extend + 64 < 0x7C00 (18 = the kernel's trip of 16 iterations + 2); swmi_banded_affine_kernel_for() reports which --
 * see DESIGN.md section 9. */
SWMI_API int swmi_score_banded_affine(const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int len,
                                      const int8_t score_matrix[16], int gap_open, int gap_extend,
                                      int32_t *scores);
SWMI_API int swmi_score_banded_affine_device(const void *d_seq1s, const void *d_seq2s, size_t n, int len,
                                             const int8_t score_matrix[16], int gap_open, int gap_extend,
                                             void *d_scores, void *stream);
/* Which kernel instantiation a banded-affine launch with these parameters runs, e.g. "sw_banded_affine_pk_kernel<1>" or
 * "sw_banded_affine_kernel<1,1>", and how many alignments one wavefront scores (2 / 1; NULL to skip).  Needs no device. */
SWMI_API int swmi_banded_affine_kernel_for(int len, const int8_t score_matrix[16], int gap_open, int gap_extend, char *name,
                                           size_t name_len, int *alignments_per_wavefront);

/* ---- semi-global adaptive-band X-drop aligner -------------------------------------
 * Replaces SemiGlobal_AdaptiveBanded_XDrop_111_32_70 and its _simd / _simd_mark2..4 variants
 * (source.cpp:1836-1976, :1978-2725; call sites TestSemiGlobal :2774-2778, SpeedtestSemiGlobal :2818-2856):
 * two 16384-mers per alignment (alignment k at byte offset 16384*k), match +1 / mismatch -1 / gap -1, band of 32,
 * X-drop 70, result = (score, traceback).  scores[k] = .first; tracebacks + k*cap*2 receives the (i, j) pairs of
 * .second in the reference's order (from (0,0) to the best cell), at most `cap` of them; lengths[k] = .second.size()
 * (<= 32769).  Host buffers.  Where the reference reads one byte past its padded sequences (the band at the very
 * last position, source.cpp:1917-1919) this implementation reads a pad.  Bases must be 0..3: the reference's sweep scores
 * any other byte as a mismatch against everything (:1918-1920) but its traceback indexes the 4x4 matrix with it (:1961,
 * out of range); here such a byte is a mismatch against everything in both. */
#define SWMI_SG_LEN 16384
#define SWMI_SG_MAX_TRACEBACK 32769
SWMI_API int swmi_semiglobal_xdrop(const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int32_t *scores,
                                   int32_t *tracebacks, size_t cap, uint32_t *lengths);
/* Same with every buffer resident in device memory (every pointer 16-byte aligned: the kernels use 16-byte loads and
 * 8-byte stores); asynchronous on `stream`.  The library keeps one workspace per (GPU, stream) of ~0.29 MB per alignment
 * (2-bit predecessor codes, the band's move bits, packed character streams, traceback moves), grown on demand and kept until
 * swmi_semiglobal_release_workspaces() / swmi_shutdown(): calls on one stream serialise by themselves, calls on
 * different streams use different workspaces and may be in flight together, from any threads. */
SWMI_API int swmi_semiglobal_xdrop_device(const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores,
                                          void *d_tracebacks, size_t cap, void *d_lengths, void *stream);
/* The same alignment with the traceback returned as MOVES instead of positions (round 4): the list of source.cpp:1962-1975
 * is 8 bytes per position, up to 262 KB per alignment, which made the host entry above 11 x slower than the device entry --
 * it ships positions over PCIe.  The walk itself produces 2 bits per step: moves + k * SWMI_SG_MOVE_WORDS receives
 * alignment k's steps in WALKING order (step 0 leaves the best cell, the last one arrives at (0, 0)), step t at bits
 * 2 (t % 32) of word t / 32: 3 = diagonal (i - 1, j - 1), 2 = up (i - 1), 1 = left (j - 1); lengths[k] = positions of the
 * reference's list = steps + 1; words past the last step are unspecified.  swmi_semiglobal_expand_moves() turns one
 * alignment's moves into the reference's (i, j) list on the host (no device; `cap` positions at most) -- the C++ overload of
 * swmi_compat.hpp does that on several threads.  The best cell is (number of steps with bit 1, number with bit 0). */
#define SWMI_SG_MOVE_WORDS 1040      /* 1025 words hold the longest path; rows are padded to whole 128-byte lines */
SWMI_API int swmi_semiglobal_xdrop_moves(const uint8_t *seq1s, const uint8_t *seq2s, size_t n, int32_t *scores,
                                         uint64_t *moves, uint32_t *lengths);
SWMI_API int swmi_semiglobal_xdrop_moves_device(const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores,
                                                void *d_moves, void *d_lengths, void *stream);
SWMI_API int swmi_semiglobal_expand_moves(const uint64_t *moves, uint32_t length, int32_t *traceback, size_t cap);
/* Which sweep kernel the aligner runs is chosen from the batch size; this overrides the choice, the
 * way swmi_set_schedule does for the scorer -- every mapping returns the same (score, traceback), tests/test_semiglobal.py
 * runs them all.  sweep: -1 = automatic, 4 / 2 / 1 = the band over 4 / 2 lanes or in one lane (16 / 32 / 64 alignments per
 * wavefront; the build for the most wavefronts per SIMD), 10 * lanes + W = that mapping compiled for W wavefronts per SIMD (41..44, 21..23, 11..12).  Anything else:
 * SWMI_ERR_INVALID_ARGUMENT.  Process-wide, one atomic word.  SWMI_SG_SWEEP in the environment sets the initial value at
 * swmi_init* (a value this call would reject is ignored).  (The traceback has one mapping: a lane per walk + expand kernel.) */
SWMI_API int swmi_semiglobal_set_mapping(int sweep);
/* The sweeps skip the X-drop test in windows of 16 rounds in which no band cell of the wavefront's alignments can reach the
 * threshold (a margin test once per window, DESIGN.md section 10: the same results by construction).  exact_only = 1 makes
 * every round run the test (A/B, tests); 0 = default.  Process-wide; SWMI_SG_EXACT in the environment gives the initial
 * value at swmi_init*. */
SWMI_API int swmi_semiglobal_set_exact(int exact_only);
/* What the last swmi_semiglobal_xdrop[_moves]_device call on `stream` of the current GPU ran: counts[0] = windows of 8 rounds
 * summed over its sweep wavefronts, counts[1] = how many of them were calm (no X-drop test); counts[2] = windows of 16 rounds
 * summed over its traceback wavefronts, counts[3] = how many of them were decoded a second time because a walk left band cells
 * 8 .. 23 (the traceback fetches that half of the predecessor records only, the other half on demand: DESIGN.md section 10).
 * Waits for the stream.  SWMI_ERR_INVALID_ARGUMENT when no call has run on that stream. */
SWMI_API int swmi_semiglobal_window_stats(void *stream, uint64_t counts[4]);
/* Free the per-stream workspaces of the current GPU (synchronises the device first). */
SWMI_API int swmi_semiglobal_release_workspaces(void);
/* Names of the sweep and traceback kernels a call with n alignments runs on the current GPU (the mapping depends on the
 * batch size and the device's CU count) -- so that a profiler-side tool asks instead of guessing. */
SWMI_API int swmi_semiglobal_kernels_for_batch(size_t n, char *sweep, size_t sweep_len, char *traceback, size_t traceback_len);
/* Measurement helper (no reference counterpart): one swmi_semiglobal_xdrop_device call bracketed by HIP events on
 * `stream`, synchronous; phase_ms[0] = the sweep kernel (source.cpp:1886-1949), phase_ms[1] = the traceback kernel
 * (source.cpp:1951-1975). */
SWMI_API int swmi_semiglobal_time_device(const void *d_seq1s, const void *d_seq2s, size_t n, void *d_scores,
                                         void *d_tracebacks, size_t cap, void *d_lengths, void *stream, float phase_ms[2]);

/* ---- local alignment with end cell, start cell and traceback ---------------------------
 * Replaces SmithWaterman_111_long (source.cpp:1526-1576: a seq1 of any length against a 128-mer -> (score, path of (i, j)))
 * for a batch of n alignments, with any int8 matrix and gap in [0, 127] (the reference's own function is score_matrix =
 * match 1 / mismatch -1, gap 1).  seq1 k = the len1 bytes at seq1s + len1 * k (1 <= len1 <= 16384, one length per call),
 * seq2 k = the 128 bytes at seq2s + 128 * k; bases are taken modulo 4 as in swmi_score_batch.
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),  i = 1..len1, j = 1..128
 * scores[k] = max H.  ends[k] = (end_i, end_j, start_i, start_j): the end cell is the first cell in row-major order that
 * holds the score ((0, 0) when it is 0, source.cpp:1545); the walk from it takes a diagonal step when H(i,j) = H(i-1,j-1) + s,
 * else an up step (i - 1) when H(i,j) = H(i-1,j) - gap, else a left step (j - 1), until it reaches a cell holding 0, the start
 * cell (source.cpp:1553-1569).  moves + k * SWMI_LOCAL_MOVE_WORDS(len1) receives the steps in WALKING order (step 0 leaves the
 * end cell), step t at bits 2 (t % 32) of word t / 32: 3 = diagonal, 2 = up, 1 = left (the encoding of
 * swmi_semiglobal_xdrop_moves); steps[k] = their number, so the reference's list has steps[k] + 1 positions; words past the
 * last step are unspecified.  moves and steps both NULL: ENDS-ONLY -- no traceback is stored or walked, the score and the end
 * cell are the same, the start cell is reported as (-1, -1).  The score is at most 127 * 128.
 * Host buffers.  The batch runs in SLICES (swmi_local_slices_for) on two sets of device buffers, one slice's copies beside
 * the other's kernel.  Errors: SWMI_ERR_INVALID_ARGUMENT for len1 outside [1, 16384], a NULL buffer, or only one of
 * moves / steps; SWMI_ERR_DOMAIN for gap_penalty < 0. */
#define SWMI_LOCAL_SEQ2_LEN 128
#define SWMI_LOCAL_MAX_LEN 16384
#define SWMI_LOCAL_MOVE_WORDS(len1) (((((size_t)(len1)) + 128 + 31) / 32 + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_local_align(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n, const int8_t score_matrix[16],
                              int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
/* The slices a swmi_local_align call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns how
 * many there are and writes the first `cap` sizes (NULL to count).  Every slice's device buffers stay within 256 MiB.
 * Needs no device.  0 for len1 outside [1, 16384]. */
SWMI_API size_t swmi_local_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes (32 * len1
 * bytes per alignment) go to a workspace of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_shutdown(): calls on one stream serialise by themselves, calls on different streams may be in flight together. */
SWMI_API int swmi_local_align_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                     void *d_moves, void *d_steps, void *stream);
/* One alignment's moves -> the reference's list of (i, j) positions from the start cell to the end cell (steps + 1 of them;
 * at most `cap` are written), on the host.  No device. */
SWMI_API int swmi_local_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                                     size_t cap);
/* Measurement helper: `iters` swmi_local_align_device calls back to back on `stream`, bracketed by HIP events; *avg_ms = the
 * average time of one call.  Synchronous. */
SWMI_API int swmi_local_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n,
                                    const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                    void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);

/* ---- local alignment with AFFINE gaps, end cell, start cell and traceback ---------------------
 * No reference counterpart: swmi_local_align with Gotoh's gaps, a gap of length k costing gap_open + (k-1) gap_extend (the
 * convention of swmi_score_banded_affine).  Same inputs, outputs, move encoding and slicing as swmi_local_align; any int8
 * matrix, gap_open and gap_extend each in [0, 127] in either order, bases taken modulo 4, 1 <= len1 <= 16384.  With
 * H(0,.) = H(.,0) = 0 and E(0,.) = F(.,0) = -inf, for i = 1..len1, j = 1..128:
 *     E(i,j) = max(H(i-1,j) - gap_open, E(i-1,j) - gap_extend)      vertical gap: consumes seq1, an up move
 *     F(i,j) = max(H(i,j-1) - gap_open, F(i,j-1) - gap_extend)      horizontal gap: consumes seq2, a left move
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))
 * scores[k] = max H; the end cell is the first cell in row-major order holding it ((0, 0) when it is 0).  The walk starts at
 * the end cell in state H.  State H at (i,j): stop if H = 0 (the start cell); else a diagonal step if H = H(i-1,j-1) + s;
 * else state E if H = E(i,j); else state F.  State E at (i,j): an up step to (i-1,j), after which the state is H if
 * E(i,j) = H(i-1,j) - gap_open (opening wins a tie) and stays E otherwise; state F likewise with left steps.  moves +
 * k * SWMI_LOCAL_MOVE_WORDS(len1) receives the steps in walking order, 3 = diagonal, 2 = up, 1 = left; steps[k] = their
 * number, so swmi_local_expand_moves rebuilds the (i, j) list.  moves and steps both NULL: ENDS-ONLY (start cell (-1, -1)).
 * With gap_open == gap_extend == g every field equals swmi_local_align's with gap g.  The score is at most 127 * 128.
 * Host buffers, in SLICES on two sets of device buffers.  Errors: SWMI_ERR_INVALID_ARGUMENT for len1 outside [1, 16384], a
 * NULL buffer, or only one of moves / steps; SWMI_ERR_DOMAIN for gap_open or gap_extend outside [0, 127]; n = 0 is a no-op
 * that needs no device. */
SWMI_API int swmi_local_align_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t n,
                                     const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                     uint64_t *moves, uint32_t *steps);
/* The slices a swmi_local_align_affine call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns
 * how many there are and writes the first `cap` sizes (NULL to count).  With a traceback a slice's device buffers stay within
 * what 4096 alignments of len1 = 16384 take (about 4.1 GiB: 1 MiB of codes each, 4 bits per cell), so that a full-length slice
 * gives every CU of an MI355X a workgroup; ends-only slices stay within 256 MiB.  At most 2^20 alignments per slice.  Needs
 * no device.  0 for len1 outside [1, 16384]. */
SWMI_API size_t swmi_local_affine_slices_for(size_t n, size_t len1, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes go to a workspace
 * of the library's per (GPU, stream), grown on demand up to one slice and kept until swmi_shutdown(). */
SWMI_API int swmi_local_align_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                            void *d_ends, void *d_moves, void *d_steps, void *stream);
/* Measurement helper: `iters` swmi_local_align_affine_device calls back to back on `stream`, bracketed by HIP events;
 * *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_local_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t n,
                                           const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                           void *d_ends, void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);

/* ---- the local aligners on a batch of MIXED seq1 lengths --------------------------------------------
 * swmi_local_align and swmi_local_align_affine with one seq1 length per alignment, as the reference's SmithWaterman_111_long
 * (source.cpp:1526) takes a seq1 of any length.  Alignment k is seq1 = bytes [seq1_offsets[k], seq1_offsets[k+1]) of seq1s
 * against the 128-mer at seq2s + 128 k; seq1_offsets holds n + 1 non-decreasing entries, and every length is in [0, 16384].
 * A length of 0 gives score 0, ends (0, 0, 0, 0) and 0 steps (ends-only: (0, 0, -1, -1)), and reads no seq1 byte.  scores,
 * ends and steps are those of the fixed-length entries, in caller order, with the same semantics, tie rules and move
 * encoding.  Alignment k's moves start at word move_offsets[k] = the sum over m < k of SWMI_LOCAL_MOVE_WORDS(length m)
 * (swmi_local_ragged_move_offsets), so swmi_local_expand_moves(moves + move_offsets[k], ...) rebuilds its path.  moves and
 * steps both NULL: ends-only.
 * Host buffers.  The batch runs in slices (swmi_local_ragged_slices_for) on two sets of device buffers, the slots of a slice
 * ordered longest first so that the alignments sharing a wavefront have similar lengths; results go to caller positions.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for decreasing offsets, a length above 16384, a NULL buffer, or only one of moves /
 * steps; SWMI_ERR_DOMAIN for parameters out of range (those of the fixed-length entries).  n = 0 is a no-op.  Every argument
 * is checked before any device is touched. */
SWMI_API int swmi_local_align_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                                     uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_local_align_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores,
                                            int32_t *ends, uint64_t *moves, uint32_t *steps);
/* move_offsets[0 .. n] of a ragged batch (the layout of its moves).  Needs no device.  SWMI_ERR_INVALID_ARGUMENT as above. */
SWMI_API int swmi_local_ragged_move_offsets(const uint64_t *seq1_offsets, size_t n, uint64_t *move_offsets);
/* The slices a ragged call of n alignments cuts its batch into (affine = 0: swmi_local_align_ragged, else the affine one;
 * traceback = 0: ends-only), in order; returns how many there are and writes the first `cap` sizes (NULL to count).  Each is
 * the longest run of the alignments left, in caller order, whose device buffers fit the fixed-length aligner's budget for one
 * slice (256 MiB; the affine aligner with a traceback: swmi_local_affine_slices_for's), at most 2^20 alignments and at least
 * one.  Needs no device.  0 for invalid offsets. */
SWMI_API size_t swmi_local_ragged_slices_for(const uint64_t *seq1_offsets, size_t n, int affine, int traceback, size_t *sizes,
                                             size_t cap);
/* Same with every data buffer in device memory (16-byte aligned), asynchronous on `stream`; d_moves uses the move_offsets
 * layout.  seq1_offsets stays a HOST array, read during the call only (it sizes the workspace and orders the work).  The
 * codes and slots go to the workspace of the fixed-length entry per (GPU, stream). */
SWMI_API int swmi_local_align_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s, size_t n,
                                            const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                            void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_local_align_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                                   size_t n, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                                   void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);

/* ---- exact semi-global aligner with traceback (SemiGlobal_111, source.cpp:1776-1834) ------------------------------------
 * The full table of the reference's SemiGlobal_111, with no band and no X-drop: the exact answer that
 * swmi_semiglobal_xdrop approximates.  n alignments of seq1 (len1 bytes, alignment k at seq1s + len1 * k) against seq2
 * (len2 bytes, at seq2s + len2 * k), one (len1, len2) per call, 1 <= len1, len2 <= 16384; any int8 matrix, gap in
 * [0, 127]; bases are taken modulo 4.  The reference's own parameters are match 1, mismatch -1, gap 1 at 16384 x 16384:
 *     H(0,0) = 0,  H(0,j) = -j gap,  H(i,0) = -i gap,
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap)      (no zero floor)
 * The BEST CELL is the first cell in row-major order over i = 0..len1, j = 0..len2 whose H is strictly greater than every
 * earlier one, starting from 0 at (0,0); scores[k] = H there (>= 0), ends[2k], ends[2k+1] = its (i, j).  When no cell is
 * above 0 the best cell is (0,0).  The walk goes from the best cell to (0,0): a diagonal step if i && j and
 * H = H(i-1,j-1) + s, else an up step if i and H = H(i-1,j) - gap, else a left step (source.cpp:1815-1827).
 * moves + k * SWMI_SGFULL_MOVE_WORDS(len1, len2) receives it in WALKING order, step t at bits 2 (t % 32) of word t / 32:
 * 3 = diagonal, 2 = up, 1 = left (the encoding of swmi_semiglobal_xdrop_moves); lengths[k] = positions of the reference's
 * list = steps + 1, so swmi_semiglobal_expand_moves(moves_k, lengths[k], ...) rebuilds that list, from (0,0) to the best
 * cell; words past the last step are unspecified.  moves and lengths both NULL: ENDS-ONLY, no codes are stored or walked.
 * H lies in [-(len1 + len2) 127, 127 min(len1, len2)].
 * Host buffers.  The batch runs in SLICES (swmi_semiglobal_full_slices_for) on two sets of device buffers, one slice's
 * copies beside the other's kernel.  Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], a NULL buffer, or
 * only one of moves / lengths; SWMI_ERR_DOMAIN for gap_penalty < 0. */
#define SWMI_SGFULL_MAX_LEN 16384
#define SWMI_SGFULL_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_semiglobal_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                  const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                                  uint64_t *moves, uint32_t *lengths);
/* The slices a swmi_semiglobal_full call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns
 * how many there are and writes the first `cap` sizes (NULL to count).  With a traceback a slice's device buffers stay
 * within what 256 alignments of 16384 x 16384 take (about 16.1 GiB: 64.25 MiB of codes each), so that a full-size slice
 * gives every CU of an MI355X a workgroup; ends-only slices stay within 256 MiB of inputs and results.  At most 2^20
 * alignments per slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_semiglobal_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes (2 bits per
 * cell) go to a workspace of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_semiglobal_full_release_workspaces() / swmi_shutdown(): calls on one stream serialise by themselves, calls on
 * different streams may be in flight together. */
SWMI_API int swmi_semiglobal_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                         void *d_moves, void *d_lengths, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_semiglobal_full_release_workspaces(void);
/* Measurement helper: `iters` swmi_semiglobal_full_device calls back to back on `stream`, bracketed by HIP events;
 * *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_semiglobal_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                              const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                              void *d_moves, void *d_lengths, void *stream, int iters, float *avg_ms);

/* ---- exact semi-global aligner with AFFINE gaps and traceback ----------------------------------
 * No reference counterpart: swmi_semiglobal_full with Gotoh's gaps, a gap of length k costing gap_open + (k-1) gap_extend
 * (the convention of swmi_score_banded_affine and swmi_local_align_affine).  n alignments; seq1 k = the len1 bytes at
 * seq1s + len1 * k, seq2 k = the len2 bytes at seq2s + len2 * k, one (len1, len2) per call, 1 <= len1, len2 <= 16384; any
 * int8 matrix; gap_open and gap_extend each in [0, 127], in either order; bases are taken modulo 4.
 *     H(0,0) = 0;  H(0,j) = -(open + (j-1) extend)  (j >= 1);  H(i,0) = -(open + (i-1) extend)  (i >= 1)
 *     E(0,j) = -inf;  F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap: consumes seq1, an up move
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap: consumes seq2, a left move
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))          (no zero floor)
 * The BEST CELL is swmi_semiglobal_full's: the first cell in row-major order over i = 0..len1, j = 0..len2 whose H is
 * strictly greater than every earlier one, starting from 0 at (0,0); (0,0) when no cell is above 0.  scores[k] = H there,
 * ends[2k], ends[2k+1] = its (i, j).  The walk starts at the best cell in state H.  State H at (i,j), i > 0 and j > 0: a
 * diagonal step if H = H(i-1,j-1) + s, else state E if H = E(i,j), else state F.  State E: an up step, after which the state
 * is H if E(i,j) = H(i-1,j) - open (opening wins a tie) and stays E otherwise; state F likewise with left steps.  On row 0
 * and column 0 the walk is forced: up along column 0, left along row 0.  moves + k * SWMI_SGFULL_MOVE_WORDS(len1, len2)
 * receives the steps in WALKING order, 3 = diagonal, 2 = up, 1 = left (every step decreases i or j); lengths[k] = steps + 1,
 * so swmi_semiglobal_expand_moves(moves_k, lengths[k], ...) rebuilds the (i, j) list from (0,0) to the best cell.  moves
 * and lengths both NULL: ENDS-ONLY, no codes are stored or walked.
 * Every H, E and F that can be reached lies in [-127 (len1 + len2), 127 min(len1, len2)], within +-2^22 (what sizes the
 * kernel's keys).  With gap_open == gap_extend == g, E(i,j) = H(i-1,j) - g exactly and opening wins the tie, so H is
 * swmi_semiglobal_full's table and the walk its walk: every field equals swmi_semiglobal_full's with gap g.
 * Host buffers, in SLICES (swmi_semiglobal_full_affine_slices_for) on two sets of device buffers.  Errors:
 * SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], a NULL buffer, or only one of moves / lengths; SWMI_ERR_DOMAIN
 * for gap_open or gap_extend outside [0, 127]; n = 0 is a no-op that needs no device.  Every argument is checked before any
 * device is touched. */
SWMI_API int swmi_semiglobal_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores,
                                         int32_t *ends, uint64_t *moves, uint32_t *lengths);
/* The slices a swmi_semiglobal_full_affine call of n alignments cuts its batch into (traceback = 0: ends-only), in order;
 * returns how many there are and writes the first `cap` sizes (NULL to count).  With a traceback a slice's device buffers
 * stay within what 256 alignments of 16384 x 16384 take (about 32.1 GiB: 128.5 MiB of codes each, 4 bits per cell), so that
 * a full-size slice gives every CU of an MI355X a workgroup; ends-only slices stay within 256 MiB.  At most 2^20 alignments
 * per slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_semiglobal_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes,
                                                       size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes go to a workspace
 * of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_semiglobal_full_affine_release_workspaces() / swmi_shutdown(). */
SWMI_API int swmi_semiglobal_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                                void *d_ends, void *d_moves, void *d_lengths, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_semiglobal_full_affine_release_workspaces(void);
/* Measurement helper: `iters` swmi_semiglobal_full_affine_device calls back to back on `stream`, bracketed by HIP events;
 * *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_semiglobal_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2,
                                                     size_t n, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                                     void *d_scores, void *d_ends, void *d_moves, void *d_lengths, void *stream,
                                                     int iters, float *avg_ms);

/* ---- local alignment of two sequences of ANY length, with end cell, start cell and traceback -----
 * swmi_local_align (SmithWaterman_111_long, source.cpp:1526-1576) with a seq2 of len2 bases instead of 128.  n alignments of
 * seq1 (len1 bytes, alignment k at seq1s + len1 * k) against seq2 (len2 bytes, at seq2s + len2 * k), one (len1, len2) per
 * call, 1 <= len1, len2 <= 16384; any int8 matrix, gap in [0, 127]; bases are taken modulo 4.
 *     H(i,0) = H(0,j) = 0
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),  i = 1..len1, j = 1..len2
 * scores[k] = max H, at most 127 * min(len1, len2) < 2^21.  ends[k] = (end_i, end_j, start_i, start_j): the end cell is the
 * first cell in row-major order that holds the score ((0, 0) when it is 0, source.cpp:1545).  The walk from it
 * (source.cpp:1555-1570) stops at a cell holding 0, the start cell -- that test comes first, so a cell holding 0 ends the
 * walk even when its diagonal candidate is also 0 -- else takes a diagonal step when H(i,j) = H(i-1,j-1) + s, else an up step
 * (i - 1) when H(i,j) = H(i-1,j) - gap, else a left step (j - 1).  Border cells hold 0: there is no forced walk along a
 * border.  moves + k * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) receives the steps in WALKING order (step 0 leaves the end
 * cell), step t at bits 2 (t % 32) of word t / 32: 3 = diagonal, 2 = up, 1 = left; steps[k] = their number, so
 * swmi_local_full_expand_moves rebuilds the reference's list of steps[k] + 1 positions; words past the last step are
 * unspecified.  moves and steps both NULL: ENDS-ONLY -- no codes are stored or walked, the start cell is reported as (-1, -1).
 * With len2 == 128 every field equals swmi_local_align's -- and swmi_local_align is the FASTER entry for that shape (its
 * kernel puts 16 lanes on the 128 columns; this one gives every alignment a workgroup of at least one wavefront of 1024
 * columns, of which 128 columns keep 8 lanes busy).  Use this entry when len2 is not 128.
 * Host buffers.  The batch runs in SLICES (swmi_local_full_slices_for) on two sets of device buffers, one slice's copies
 * beside the other's kernel.  Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], a NULL buffer, or only one
 * of moves / steps; SWMI_ERR_DOMAIN for gap_penalty < 0; n = 0 is a no-op that needs no device.  Every argument is checked
 * before any device is touched. */
#define SWMI_LOCAL_FULL_MAX_LEN 16384
#define SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_local_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                             const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves,
                             uint32_t *steps);
/* The slices a swmi_local_full call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns how
 * many there are and writes the first `cap` sizes (NULL to count).  With a traceback a slice's device buffers stay within
 * what 256 alignments of 16384 x 16384 take (about 16.1 GiB: 64.25 MiB of codes each), so that a full-size slice gives every
 * CU of an MI355X a workgroup; ends-only slices stay within 256 MiB of inputs and results.  At most 2^20 alignments per
 * slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_local_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes (2 bits per
 * cell) go to a workspace of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_local_full_release_workspaces() / swmi_shutdown(): calls on one stream serialise by themselves, calls on different
 * streams may be in flight together. */
SWMI_API int swmi_local_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                    const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                    void *d_moves, void *d_steps, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_local_full_release_workspaces(void);
/* Measurement helper: `iters` swmi_local_full_device calls back to back on `stream`, bracketed by HIP events; *avg_ms = the
 * average time of one call.  Synchronous. */
SWMI_API int swmi_local_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                         void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);
/* One alignment's moves -> the reference's list of (i, j) positions from the start cell to the end cell (steps + 1 of them;
 * at most `cap` are written), on the host: swmi_local_expand_moves with both axes up to 16384.  No device.
 * SWMI_ERR_INVALID_ARGUMENT for an end cell outside the matrix, a move of 0, or moves that leave the matrix. */
SWMI_API int swmi_local_full_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                                          size_t cap);

/* ---- local alignment of two sequences of ANY length with AFFINE gaps, end cell, start cell and traceback (DESIGN.md
 * section 18) ------------------------------------------------------------------------------------------------------------
 * No reference counterpart: swmi_local_full with Gotoh's gaps, a gap of length k costing gap_open + (k-1) gap_extend (the
 * convention of swmi_score_banded_affine, swmi_local_align_affine and swmi_semiglobal_full_affine).  n alignments; seq1 k =
 * the len1 bytes at seq1s + len1 * k, seq2 k = the len2 bytes at seq2s + len2 * k, one (len1, len2) per call,
 * 1 <= len1, len2 <= 16384 (SWMI_LOCAL_FULL_MAX_LEN); any int8 matrix; gap_open and gap_extend each in [0, 127], in either
 * order; bases are taken modulo 4.
 *     H(i,0) = H(0,j) = 0;  E(0,j) = -inf;  F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap: consumes seq1, an up move
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap: consumes seq2, a left move
 *     H(i,j) = max(0, H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j)),   i = 1..len1, j = 1..len2
 * scores[k] = max H, at most 127 * min(len1, len2) < 2^21.  ends[k] = (end_i, end_j, start_i, start_j): the end cell is the
 * first cell in row-major order that holds the score, (0, 0) when it is 0.  The walk is swmi_local_align_affine's on
 * swmi_local_full's borders.  It starts at the end cell in state H.  State H at (i,j): stop if H = 0 (this test comes first:
 * the floor wins every tie at 0), else a diagonal step if H = H(i-1,j-1) + s, else state E if H = E(i,j), else state F.
 * State E: an up step to (i-1,j), after which the state is H if E(i,j) = H(i-1,j) - open (opening wins a tie) and stays E
 * otherwise; state F likewise with left steps.  Border cells hold 0 and E(1,j), F(i,1) always open, so the walk arrives on
 * a border in state H and stops there: there is no forced walk along a border.
 * moves + k * SWMI_LOCAL_FULL_MOVE_WORDS(len1, len2) receives the steps in WALKING order, step t at bits 2 (t % 32) of word
 * t / 32: 3 = diagonal, 2 = up, 1 = left; steps[k] = their number.  Every step decreases i or j, so
 * swmi_local_full_expand_moves rebuilds the list of steps[k] + 1 positions from the start cell to the end cell; words past
 * the last step are unspecified.  moves and steps both NULL: ENDS-ONLY -- no codes are stored or walked, the start cell is
 * reported as (-1, -1).
 * With gap_open == gap_extend == g, E(i,j) = H(i-1,j) - g exactly and opening wins the tie, so every field equals
 * swmi_local_full's with gap g.  With len2 == 128 every field equals swmi_local_align_affine's -- and
 * swmi_local_align_affine is the FASTER entry for that shape (its kernel puts 16 lanes on the 128 columns; this one gives
 * every alignment a workgroup of at least one wavefront of 1024 columns).  Use this entry when len2 is not 128.
 * Host buffers, in SLICES (swmi_local_full_affine_slices_for) on two sets of device buffers.  Errors:
 * SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], a NULL buffer or matrix, or only one of moves / steps;
 * SWMI_ERR_DOMAIN for gap_open or gap_extend outside [0, 127]; n = 0 is a no-op that needs no device.  Every argument is
 * checked before any device is touched. */
SWMI_API int swmi_local_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                    const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                    uint64_t *moves, uint32_t *steps);
/* The slices a swmi_local_full_affine call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns
 * how many there are and writes the first `cap` sizes (NULL to count).  With a traceback a slice's device buffers stay
 * within what 256 alignments of 16384 x 16384 take (about 32.1 GiB: 128.5 MiB of codes each, 4 bits per cell), so that a
 * full-size slice gives every CU of an MI355X a workgroup; ends-only slices stay within 256 MiB.  At most 2^20 alignments
 * per slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_local_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes go to a workspace
 * of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_local_full_affine_release_workspaces() / swmi_shutdown(). */
SWMI_API int swmi_local_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                           const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                           void *d_ends, void *d_moves, void *d_steps, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_local_full_affine_release_workspaces(void);
/* Measurement helper: `iters` swmi_local_full_affine_device calls back to back on `stream`, bracketed by HIP events;
 * *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_local_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                                void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                                float *avg_ms);

/* ---- the any-length local aligners on a batch of MIXED (len1, len2) ----------------------------------
 * swmi_local_full and swmi_local_full_affine with one (len1, len2) per alignment.  Alignment k is seq1 = bytes
 * [seq1_offsets[k], seq1_offsets[k+1]) of seq1s against seq2 = bytes [seq2_offsets[k], seq2_offsets[k+1]) of seq2s; both
 * offset arrays hold n + 1 non-decreasing entries, and every length is in [0, 16384].  If either length is 0 the alignment
 * gives score 0, ends (0, 0, 0, 0) and 0 steps (ends-only: (0, 0, -1, -1)), and reads no byte of either sequence.  scores,
 * ends and steps are those of the fixed-length entries, in caller order, with the same semantics, tie rules and move
 * encoding.  Alignment k's moves start at word move_offsets[k] = the sum over m < k of
 * SWMI_LOCAL_FULL_MOVE_WORDS(len1 of m, len2 of m) (swmi_local_full_ragged_move_offsets), so
 * swmi_local_full_expand_moves(moves + move_offsets[k], ...) rebuilds its path.  moves and steps both NULL: ends-only.
 * Host buffers.  The batch runs in slices (swmi_local_full_ragged_slices_for) on two sets of device buffers.  One workgroup
 * of ceil(len2 / 1024) wavefronts computes an alignment, so a slice runs as one launch per wave count present in it, the
 * widest first, and inside a launch the longest seq1 first; results go to caller positions.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for decreasing offsets, a length above 16384, a NULL buffer, or only one of moves /
 * steps; SWMI_ERR_DOMAIN for parameters out of range (those of the fixed-length entries).  n = 0 is a no-op that needs no
 * device.  Every argument is checked before any device is touched. */
SWMI_API int swmi_local_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                    const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                                    int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_local_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                           const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                           int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
/* move_offsets[0 .. n] of a ragged batch (the layout of its moves).  Needs no device.  SWMI_ERR_INVALID_ARGUMENT as above. */
SWMI_API int swmi_local_full_ragged_move_offsets(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n,
                                                 uint64_t *move_offsets);
/* The slices a ragged call of n alignments cuts its batch into (affine = 0: swmi_local_full_ragged, else the affine one;
 * traceback = 0: ends-only), in order; returns how many there are and writes the first `cap` sizes (NULL to count).  Each is
 * the longest run of the alignments left, in caller order, whose device bytes -- inputs, slots and results, plus codes, moves
 * and steps with a traceback -- fit the fixed-length aligner's budget for one slice (swmi_local_full_slices_for's or
 * swmi_local_full_affine_slices_for's with a traceback; 256 MiB ends-only), at most 2^20 alignments and at least one.  Needs
 * no device.  0 for invalid offsets. */
SWMI_API size_t swmi_local_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                                  int traceback, size_t *sizes, size_t cap);
/* Same with every data buffer in device memory (16-byte aligned at its base; an alignment's offsets need no alignment),
 * asynchronous on `stream`; d_moves uses the move_offsets layout.  Both offset arrays stay HOST arrays, read during the call
 * only (they size the workspace and order the work).  The codes and slots go to the workspace of the fixed-length entry per
 * (GPU, stream). */
SWMI_API int swmi_local_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                           const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                           int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                           void *stream);
SWMI_API int swmi_local_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                                  const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                                  int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves,
                                                  void *d_steps, void *stream);

/* unpack() itself (source.cpp:1580-1583) for n packed sequences, on the GPU. Host buffers. */
SWMI_API int swmi_unpack(const uint8_t *packed, size_t n_seqs, uint8_t *unpacked);

/* ---- global and free-end-gap alignment of two sequences of ANY length, with end cell, start cell and traceback (DESIGN.md
 * section 20) ------------------------------------------------------------------------------------------------------------
 * No reference counterpart: Needleman-Wunsch and its end-gap-free relatives, with linear gaps.  n alignments; seq1 k = the
 * len1 bytes at seq1s + len1 * k, seq2 k = the len2 bytes at seq2s + len2 * k, one (len1, len2) per call,
 * 1 <= len1, len2 <= 16384 (SWMI_GLOBAL_FULL_MAX_LEN); any int8 matrix, gap in [0, 127]; bases are taken modulo 4.
 * free_ends is a mask of SWMI_FREE_* that says which end gaps cost nothing; all 16 masks are valid:
 *     SWMI_FREE_BEGIN1  leading bases of seq1 may stay unaligned: H(i,0) = 0, else H(i,0) = -i gap
 *     SWMI_FREE_BEGIN2  H(0,j) = 0, else H(0,j) = -j gap
 *     SWMI_FREE_END1    trailing bases of seq1 are free: the end cell may be any (i, len2), i = 0..len1
 *     SWMI_FREE_END2    the end cell may be any (len1, j), j = 0..len2
 * SWMI_ENDS_GLOBAL (0) aligns both sequences end to end, SWMI_ENDS_FIT all of seq1 against a stretch of seq2,
 * SWMI_ENDS_OVERLAP a suffix of one sequence against a prefix of the other.
 *     H(0,0) = 0
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], H(i-1,j) - gap, H(i,j-1) - gap),  i = 1..len1, j = 1..len2
 * with no zero floor.  The end cell is (len1, len2), or with SWMI_FREE_END1 / SWMI_FREE_END2 the cell of the last column /
 * last row (border cells (0, len2) and (len1, 0) included) that holds the largest H; among equal ones the first in row-major
 * order (smallest i, then smallest j).  scores[k] = that H, which may be NEGATIVE; |score| < 2^22.
 * ends[k] = (end_i, end_j, start_i, start_j).  The walk goes back from the end cell: a diagonal step when
 * H(i,j) = H(i-1,j-1) + s, else an up step (i - 1) when H(i,j) = H(i-1,j) - gap, else a left step (j - 1).  At (0, 0) it
 * ends.  On row 0 with j > 0 it ends if SWMI_FREE_BEGIN2 is set, else goes left to (0, 0) by forced steps; on column 0 with
 * i > 0 it ends if SWMI_FREE_BEGIN1 is set, else goes up to (0, 0) by forced steps.  The start cell is where it ended.
 * moves + k * SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2) receives the steps in WALKING order (step 0 leaves the end cell), step t
 * at bits 2 (t % 32) of word t / 32: 3 = diagonal, 2 = up, 1 = left; steps[k] = their number, forced steps included, so
 * swmi_local_full_expand_moves rebuilds the list of steps[k] + 1 positions from the start cell to the end cell; words past
 * the last step are unspecified.  moves and steps both NULL: ENDS-ONLY -- no codes are stored or walked, the start cell is
 * reported as (-1, -1).
 * Host buffers.  The batch runs in SLICES (swmi_global_full_slices_for) on two sets of device buffers, one slice's copies
 * beside the other's kernel.  Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], free_ends above 15, a NULL
 * buffer, or only one of moves / steps; SWMI_ERR_DOMAIN for gap_penalty < 0; n = 0 is a no-op that needs no device.  Every
 * argument is checked before any device is touched. */
#define SWMI_FREE_BEGIN1 1u
#define SWMI_FREE_BEGIN2 2u
#define SWMI_FREE_END1 4u
#define SWMI_FREE_END2 8u
#define SWMI_ENDS_GLOBAL 0u
#define SWMI_ENDS_FIT (SWMI_FREE_BEGIN2 | SWMI_FREE_END2)
#define SWMI_ENDS_OVERLAP (SWMI_FREE_BEGIN1 | SWMI_FREE_BEGIN2 | SWMI_FREE_END1 | SWMI_FREE_END2)
#define SWMI_GLOBAL_FULL_MAX_LEN 16384
#define SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_global_full(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                              const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, int32_t *scores,
                              int32_t *ends, uint64_t *moves, uint32_t *steps);
/* The slices a swmi_global_full call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns how
 * many there are and writes the first `cap` sizes (NULL to count).  The budgets are swmi_local_full_slices_for's: with a
 * traceback what 256 alignments of 16384 x 16384 take (about 16.1 GiB), ends-only 256 MiB; at most 2^20 alignments per
 * slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_global_full_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes (2 bits per
 * cell) go to a workspace of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_global_full_release_workspaces() / swmi_shutdown(): calls on one stream serialise by themselves, calls on different
 * streams may be in flight together. */
SWMI_API int swmi_global_full_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores,
                                     void *d_ends, void *d_moves, void *d_steps, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_global_full_release_workspaces(void);
/* Measurement helper: `iters` swmi_global_full_device calls back to back on `stream`, bracketed by HIP events; *avg_ms = the
 * average time of one call.  Synchronous. */
SWMI_API int swmi_global_full_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                          const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores,
                                          void *d_ends, void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);

/* ---- global and free-end-gap alignment with AFFINE gaps of two sequences of ANY length, with end cell, start cell and
 * traceback ------------------------------------------------------------------------------------------
 * No reference counterpart: swmi_global_full with Gotoh's gaps, a gap of length k costing gap_open + (k-1) gap_extend (the
 * convention of swmi_semiglobal_full_affine and swmi_local_full_affine).  n alignments; seq1 k = the len1 bytes at
 * seq1s + len1 * k, seq2 k = the len2 bytes at seq2s + len2 * k, one (len1, len2) per call, 1 <= len1, len2 <= 16384
 * (SWMI_GLOBAL_FULL_MAX_LEN); any int8 matrix; gap_open and gap_extend each in [0, 127], in either order; bases are taken
 * modulo 4.  free_ends is swmi_global_full's mask of SWMI_FREE_*; all 16 masks are valid.
 *     H(0,0) = 0
 *     H(i,0) = SWMI_FREE_BEGIN1 ? 0 : -(open + (i-1) extend)  (i >= 1)
 *     H(0,j) = SWMI_FREE_BEGIN2 ? 0 : -(open + (j-1) extend)  (j >= 1)
 *     E(0,j) = -inf;  F(i,0) = -inf
 *     E(i,j) = max(H(i-1,j) - open, E(i-1,j) - extend)        vertical gap: consumes seq1, an up move
 *     F(i,j) = max(H(i,j-1) - open, F(i,j-1) - extend)        horizontal gap: consumes seq2, a left move
 *     H(i,j) = max(H(i-1,j-1) + sm[seq1[i-1]*4 + seq2[j-1]], E(i,j), F(i,j))          (no zero floor)
 * The END CELL is swmi_global_full's rule on H: (len1, len2), or with SWMI_FREE_END1 / SWMI_FREE_END2 the cell of the last
 * column / last row (border cells (0, len2) and (len1, 0) included, with the values above) that holds the largest H; among
 * equal ones the first in row-major order.  scores[k] = that H, which may be NEGATIVE; every H, E and F that can be reached
 * lies in [-127 (len1 + len2), 127 min(len1, len2)], so |score| < 2^22.  ends[k] = (end_i, end_j, start_i, start_j).
 * The walk is swmi_semiglobal_full_affine's: it starts at the end cell in state H.  State H at (i,j), i > 0 and j > 0: a
 * diagonal step if H = H(i-1,j-1) + s, else state E if H = E(i,j), else state F.  State E: an up step, after which the state
 * is H if E(i,j) = H(i-1,j) - open (opening wins a tie) and stays E otherwise; state F likewise with left steps.  E(1,j) and
 * F(i,1) always open, so the walk reaches row 0 or column 0 in state H, and there swmi_global_full's border rule holds: at
 * (0, 0) it ends; on row 0 with j > 0 it ends if SWMI_FREE_BEGIN2 is set, else goes left to (0, 0) by forced steps; on column
 * 0 with i > 0 it ends if SWMI_FREE_BEGIN1 is set, else goes up to (0, 0) by forced steps.  The start cell is where it ended.
 * moves + k * SWMI_GLOBAL_FULL_MOVE_WORDS(len1, len2) receives the steps in WALKING order, 3 = diagonal, 2 = up, 1 = left;
 * steps[k] = their number, forced steps included, so swmi_local_full_expand_moves rebuilds the list of steps[k] + 1 positions
 * from the start cell to the end cell; words past the last step are unspecified.  moves and steps both NULL: ENDS-ONLY -- no
 * codes are stored or walked, the start cell is reported as (-1, -1).
 * Two identities follow from the definition:
 *     gap_open == gap_extend == g: E(i,j) = H(i-1,j) - g and F(i,j) = H(i,j-1) - g exactly, opening wins the tie and the
 *     borders are -i g / -j g or 0, so every field equals swmi_global_full's with gap g, under every mask;
 *     mask 0: the table is swmi_semiglobal_full_affine's table.  For a pair whose best cell (ei, ej) there has ei, ej >= 1,
 *     the mask-0 alignment of seq1[:ei] against seq2[:ej] has that score, steps == lengths - 1 and the same moves.
 * Host buffers, in SLICES (swmi_global_full_affine_slices_for) on two sets of device buffers.  Errors:
 * SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 16384], free_ends above 15, a NULL buffer, or only one of moves / steps;
 * SWMI_ERR_DOMAIN for gap_open or gap_extend outside [0, 127]; n = 0 is a no-op that needs no device.  Every argument is
 * checked before any device is touched. */
SWMI_API int swmi_global_full_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                     int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
/* The slices a swmi_global_full_affine call of n alignments cuts its batch into (traceback = 0: ends-only), in order; returns
 * how many there are and writes the first `cap` sizes (NULL to count).  The budgets are swmi_semiglobal_full_affine_slices_for's:
 * with a traceback what 256 alignments of 16384 x 16384 take (about 32.1 GiB: 128.5 MiB of codes each, 4 bits per cell),
 * ends-only 256 MiB; at most 2^20 alignments per slice.  Needs no device.  0 for a length outside [1, 16384]. */
SWMI_API size_t swmi_global_full_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
/* Same with every buffer in device memory (16-byte aligned), asynchronous on `stream`.  The traceback codes go to a workspace
 * of the library's per (GPU, stream), grown on demand up to one slice and kept until
 * swmi_global_full_affine_release_workspaces() / swmi_shutdown(): calls on one stream serialise by themselves, calls on
 * different streams may be in flight together. */
SWMI_API int swmi_global_full_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                            void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);
/* Free the device buffers of both entries above on the current GPU (synchronises the device first). */
SWMI_API int swmi_global_full_affine_release_workspaces(void);
/* Measurement helper: `iters` swmi_global_full_affine_device calls back to back on `stream`, bracketed by HIP events;
 * *avg_ms = the average time of one call.  Synchronous. */
SWMI_API int swmi_global_full_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                 const int8_t score_matrix[16], int gap_open, int gap_extend,
                                                 unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                                 void *stream, int iters, float *avg_ms);

/* ---- the global / fit / overlap aligners on a batch of MIXED (len1, len2) ----------------------------
 * swmi_global_full and swmi_global_full_affine with one (len1, len2) per alignment and one mask and one set of gaps per
 * call.  Alignment k is seq1 = bytes [seq1_offsets[k], seq1_offsets[k+1]) of seq1s against seq2 = bytes
 * [seq2_offsets[k], seq2_offsets[k+1]) of seq2s; both offset arrays hold n + 1 non-decreasing entries, and every length is in
 * [0, 16384].  scores, ends = (end_i, end_j, start_i, start_j) and steps are those of the fixed-length entries, in caller
 * order, with the same semantics, tie rules, forced border steps and move encoding, under every one of the 16 masks.
 * Alignment k's moves start at word move_offsets[k].  SWMI_GLOBAL_FULL_MOVE_WORDS is SWMI_LOCAL_FULL_MOVE_WORDS, so
 * swmi_local_full_ragged_move_offsets gives the layout, and there is no second function for it;
 * swmi_local_full_expand_moves(moves + move_offsets[k], ...) rebuilds a path.  moves and steps both NULL: ends-only, the
 * start cell reported as (-1, -1).
 * ZERO LENGTHS follow from the definitions above extended to an empty sequence -- they are NOT the local aligners' "score 0".
 * The table is then one border.  Let L be the non-empty sequence's length and cost(L) = L gap (linear gaps) or
 * open + (L - 1) extend (affine gaps).  For len2 == 0 the border is column 0: BEGIN = SWMI_FREE_BEGIN1, END = SWMI_FREE_END1,
 * the forced move is "up" (2).  For len1 == 0 it is row 0: BEGIN = SWMI_FREE_BEGIN2, END = SWMI_FREE_END2, the move "left" (1).
 *     case                    score      ends                                      steps
 *     both lengths 0          0          (0, 0, 0, 0)                              0
 *     END set                 0          (0, 0, 0, 0)                              0
 *     END clear, BEGIN set    0          end = start = (L, 0) or (0, L)            0
 *     neither                 -cost(L)   end (L, 0) or (0, L), start (0, 0)        L forced moves
 * With END set the first border cell in row-major order, (0, 0), holds the largest H (0), also at gap 0.  In the last row
 * the L forced moves are all the same code: whole words of 0xAAAA... (up) or 0x5555... (left); bits past step L are
 * unspecified, as everywhere.  Ends-only gives the same score and end cell, with start (-1, -1).  No byte of either sequence
 * is read.
 * Host buffers.  The batch runs in slices (swmi_global_full_ragged_slices_for) on two sets of device buffers.  One workgroup of
 * ceil(len2 / 1024) wavefronts computes an alignment (one wavefront when a length is 0), so a slice runs as one launch per
 * wave count present in it, the widest first, and inside a launch the longest seq1 first; results go to caller positions.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for decreasing offsets, a length above 16384, free_ends above 15, a NULL buffer, or only
 * one of moves / steps; SWMI_ERR_DOMAIN as in the fixed-length entries.  n = 0 is a no-op that needs no device.  Every argument
 * is checked before any device is touched. */
SWMI_API int swmi_global_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                     const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                                     unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API int swmi_global_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                            const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                            int gap_extend, unsigned free_ends, int32_t *scores, int32_t *ends, uint64_t *moves,
                                            uint32_t *steps);
/* The slices a ragged call of n alignments cuts its batch into (affine = 0: swmi_global_full_ragged, else the affine one;
 * traceback = 0: ends-only), in order; returns how many there are and writes the first `cap` sizes (NULL to count).  Each is
 * the longest run of the alignments left, in caller order, whose device bytes -- inputs, slots and results, plus codes, moves
 * and steps with a traceback -- fit the fixed-length aligner's budget for one slice (swmi_global_full_slices_for's or
 * swmi_global_full_affine_slices_for's with a traceback; 256 MiB ends-only), at most 2^20 alignments and at least one.  An
 * alignment with a zero length takes no codes, but its move words.  Needs no device.  0 for invalid offsets. */
SWMI_API size_t swmi_global_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n, int affine,
                                                   int traceback, size_t *sizes, size_t cap);
/* Same with every data buffer in device memory (16-byte aligned at its base; an alignment's offsets need no alignment),
 * asynchronous on `stream`; d_moves uses the move_offsets layout.  Both offset arrays stay HOST arrays, read during the call
 * only.  The codes and slots go to the workspace of the fixed-length entry per (GPU, stream)
 * (swmi_global_full_release_workspaces / swmi_global_full_affine_release_workspaces free it). */
SWMI_API int swmi_global_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                            const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                            int8_t gap_penalty, unsigned free_ends, void *d_scores, void *d_ends, void *d_moves,
                                            void *d_steps, void *stream);
SWMI_API int swmi_global_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                                   const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                                   int gap_open, int gap_extend, unsigned free_ends, void *d_scores,
                                                   void *d_ends, void *d_moves, void *d_steps, void *stream);

/* ---- global, fit and overlap alignment of sequences up to 65536 long ---------------------------------
 * swmi_global_full and swmi_global_full_affine for 1 <= len1, len2 <= 65536 (SWMI_GLOBAL_LONG_MAX_LEN): the same recurrences,
 * free_ends mask (all 16 values), end-cell rule, tie order and walk, and the same scores / ends[4] / moves / steps layout,
 * ends-only with moves and steps both NULL.  moves + k * SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2) receives alignment k's steps
 * (the formula of SWMI_GLOBAL_FULL_MOVE_WORDS); swmi_global_long_expand_moves rebuilds the list of steps[k] + 1 positions
 * (swmi_local_full_expand_moves with end cells up to (65536, 65536)).  On a shape with both lengths <= 16384 every field
 * equals the fixed-length entry's.
 * DOMAIN.  Bytes are taken modulo 4, gaps lie in [0, 127], and with
 *     P = max(1, max |score_matrix[k]|, gap_penalty)           (affine: max(.., gap_open, gap_extend))
 * a call is accepted iff P * (len1 + len2) <= 2^23: then every |H| <= 2^23 and the kernels' 32-bit keys cannot wrap.  So every
 * shape up to 32768 x 32768 is accepted with any int8 parameters, and 65536 x 65536 with every magnitude <= 64.  |score| <= 2^23.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 65536], a call outside the domain rule, free_ends above 15, a
 * NULL buffer, or only one of moves / steps; SWMI_ERR_DOMAIN for a gap outside [0, 127]; n = 0 is a no-op that needs no
 * device.  Every argument is checked before any device is touched and before any launch.
 * One workgroup aligns one pair and sweeps len2 in stripes of 16384 columns (the kernels' files tell how); between two
 * stripes a column of len1 values (affine: 2 len1) per alignment waits in device memory, which the library keeps beside the
 * traceback codes and counts in a slice.
 * SLICES (swmi_global_long_slices_for, swmi_global_long_affine_slices_for): the budgets are the fixed-length entries' -- with
 * a traceback what 256 alignments of 16384 x 16384 take, ends-only 256 MiB, at most 2^20 alignments and never fewer than
 * one.  KNOWN LIMIT: at 65536 x 65536 a traceback slice holds 16 alignments (about 1 GiB of codes each, 2 GiB with affine
 * gaps, whose budget is twice as large), fewer than an MI355X has CUs.  0 for a length outside [1, 65536].
 * The _device, _release_workspaces and _time_device forms are the fixed-length entries' (16-byte aligned device buffers,
 * asynchronous on `stream`, a workspace of the library's per (GPU, stream)). */
#define SWMI_GLOBAL_LONG_MAX_LEN 65536
#define SWMI_GLOBAL_LONG_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_global_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                              const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, int32_t *scores,
                              int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API size_t swmi_global_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
SWMI_API int swmi_global_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores,
                                     void *d_ends, void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_global_long_release_workspaces(void);
SWMI_API int swmi_global_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                          const int8_t score_matrix[16], int8_t gap_penalty, unsigned free_ends, void *d_scores,
                                          void *d_ends, void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);
SWMI_API int swmi_global_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                                           size_t cap);
SWMI_API int swmi_global_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                     const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                     int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *steps);
SWMI_API size_t swmi_global_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
SWMI_API int swmi_global_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                            const int8_t score_matrix[16], int gap_open, int gap_extend, unsigned free_ends,
                                            void *d_scores, void *d_ends, void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_global_long_affine_release_workspaces(void);
SWMI_API int swmi_global_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                 const int8_t score_matrix[16], int gap_open, int gap_extend,
                                                 unsigned free_ends, void *d_scores, void *d_ends, void *d_moves, void *d_steps,
                                                 void *stream, int iters, float *avg_ms);

/* ---- local alignment of sequences up to 65536 long ---------------------------------------------------
 * swmi_local_full and swmi_local_full_affine for 1 <= len1, len2 <= 65536 (SWMI_LOCAL_LONG_MAX_LEN): the same recurrences, zero
 * floor, end cell (the first cell in row-major order holding max H; (0, 0) when that is 0), walk (it stops on the first cell
 * holding 0) and tie order, and the same scores / ends[4] / moves / steps layout, field for field; ends-only (moves and steps
 * both NULL) ends[4 k + 2] = ends[4 k + 3] = -1.  moves + k * SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) receives alignment k's
 * steps (the formula of SWMI_LOCAL_FULL_MOVE_WORDS); swmi_local_long_expand_moves rebuilds the list of steps[k] + 1 positions
 * (swmi_local_full_expand_moves with end cells up to (65536, 65536)).  On a shape with both lengths <= 16384 the fixed-length
 * kernel runs, so every field equals the fixed-length entry's.
 * DOMAIN.  Bytes are taken modulo 4.  There is NO domain rule: 0 <= H <= 127 * 65536 < 2^23 whatever the parameters, so every
 * int8 matrix and gap (affine: gap_open and gap_extend each in [0, 127]) is accepted at every shape.  0 <= score < 2^23.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 65536], a NULL buffer, or only one of moves / steps; with affine
 * gaps SWMI_ERR_DOMAIN for a gap outside [0, 127]; n = 0 is a no-op that needs no device.  Every argument is checked before
 * any device is touched and before any launch.
 * One workgroup aligns one pair and sweeps len2 in stripes of 16384 columns (the kernels' files tell how); where len2 > 16384
 * a column of len1 values (affine: 2 len1) per alignment waits between two stripes in device memory, which the library keeps
 * beside the traceback codes and counts in a slice.
 * SLICES (swmi_local_long_slices_for, swmi_local_long_affine_slices_for): the budgets are the fixed-length local entries' --
 * with a traceback what 256 alignments of 16384 x 16384 take, ends-only 256 MiB, at most 2^20 alignments and never fewer than
 * one.  KNOWN LIMIT: at 65536 x 65536 a traceback slice holds 16 alignments (about 1 GiB of codes each, 2 GiB with affine
 * gaps, whose budget is twice as large), fewer than an MI355X has CUs.  0 for a length outside [1, 65536].
 * The _device, _release_workspaces and _time_device forms are the fixed-length entries' (16-byte aligned device buffers,
 * asynchronous on `stream`, a workspace of the library's per (GPU, stream)). */
#define SWMI_LOCAL_LONG_MAX_LEN 65536
#define SWMI_LOCAL_LONG_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
SWMI_API int swmi_local_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                             const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends, uint64_t *moves,
                             uint32_t *steps);
SWMI_API size_t swmi_local_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
SWMI_API int swmi_local_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                    const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                    void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_local_long_release_workspaces(void);
SWMI_API int swmi_local_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                         void *d_moves, void *d_steps, void *stream, int iters, float *avg_ms);
SWMI_API int swmi_local_long_expand_moves(const uint64_t *moves, uint32_t steps, int32_t end_i, int32_t end_j, int32_t *positions,
                                          size_t cap);
SWMI_API int swmi_local_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                    const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores, int32_t *ends,
                                    uint64_t *moves, uint32_t *steps);
SWMI_API size_t swmi_local_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
SWMI_API int swmi_local_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                           const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                           void *d_ends, void *d_moves, void *d_steps, void *stream);
SWMI_API int swmi_local_long_affine_release_workspaces(void);
SWMI_API int swmi_local_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                                void *d_ends, void *d_moves, void *d_steps, void *stream, int iters,
                                                float *avg_ms);

/* ---- exact semi-global alignment of sequences up to 65536 long ---------------------------------------
 * swmi_semiglobal_full and swmi_semiglobal_full_affine for 1 <= len1, len2 <= 65536 (SWMI_SEMIGLOBAL_LONG_MAX_LEN): the same
 * recurrences and charged borders (no zero floor), the same best cell (the first cell in row-major order over i = 0..len1,
 * j = 0..len2 strictly above every earlier one, from 0 at (0, 0); (0, 0) when nothing is above 0), the same walk back to
 * (0, 0), forced on row 0 and column 0, the same tie order (diagonal, up, left; affine: diagonal, E, F, and opening wins), and
 * the same scores / ends[2] / moves / lengths layout, field for field: ends[2 k .. 2 k + 1] = the best cell, moves +
 * k * SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(len1, len2) alignment k's moves in WALKING order (the formula of SWMI_SGFULL_MOVE_WORDS),
 * lengths[k] = steps + 1 <= SWMI_SEMIGLOBAL_LONG_MAX_TRACEBACK.  moves and lengths both NULL: ENDS-ONLY.
 * swmi_semiglobal_long_expand_moves(moves_k, lengths[k], ...) rebuilds the (i, j) list from (0, 0) to the best cell; it is
 * swmi_semiglobal_expand_moves for lengths up to 131073 (that one keeps refusing a length above 32769).  On a shape with both
 * lengths <= 16384 the fixed-length kernel runs, so every field equals the fixed-length entry's.
 * DOMAIN.  Bytes are taken modulo 4.  H is not floored, so swmi_global_long's rule applies: with P = max(1, max |score_matrix|,
 * gap_penalty) (affine: gap_open and gap_extend in place of gap_penalty) a call is accepted iff P * (len1 + len2) <= 2^23.
 * Every shape up to 32768 x 32768 passes with any int8 parameters, 65536 x 65536 with every magnitude <= 64.  0 <= score <
 * 2^23.
 * Errors: SWMI_ERR_INVALID_ARGUMENT for a length outside [1, 65536], a NULL buffer, only one of moves / lengths, or a call
 * outside the domain rule; SWMI_ERR_DOMAIN for gap_penalty < 0 (affine: a gap outside [0, 127]); n = 0 is a no-op that needs
 * no device.  Every argument is checked before any device is touched and before any launch.
 * One workgroup aligns one pair and sweeps len2 in stripes of 16384 columns (the kernels' files tell how); where len2 > 16384
 * a column of len1 values (affine: 2 len1) per alignment waits between two stripes in device memory, which the library keeps
 * beside the traceback codes and counts in a slice.
 * SLICES (swmi_semiglobal_long_slices_for, swmi_semiglobal_long_affine_slices_for): the budgets are the fixed-length
 * semi-global entries' -- with a traceback what 256 alignments of 16384 x 16384 take, ends-only 256 MiB, at most 2^20
 * alignments and never fewer than one.  KNOWN LIMIT: at 65536 x 65536 a traceback slice holds 16 alignments (about 1 GiB of
 * codes each, 2 GiB with affine gaps, whose budget is twice as large), fewer than an MI355X has CUs.  0 for a length outside
 * [1, 65536].
 * The _device, _release_workspaces and _time_device forms are the fixed-length entries' (16-byte aligned device buffers,
 * asynchronous on `stream`, a workspace of the library's per (GPU, stream)). */
#define SWMI_SEMIGLOBAL_LONG_MAX_LEN 65536
#define SWMI_SEMIGLOBAL_LONG_MOVE_WORDS(len1, len2) ((((((size_t)(len1)) + ((size_t)(len2)) + 31) / 32) + 1) & ~(size_t)1)   /* 16-byte rows */
#define SWMI_SEMIGLOBAL_LONG_MAX_TRACEBACK 131073      /* 65536 + 65536 steps + 1 */
SWMI_API int swmi_semiglobal_long(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                  const int8_t score_matrix[16], int8_t gap_penalty, int32_t *scores, int32_t *ends,
                                  uint64_t *moves, uint32_t *lengths);
SWMI_API size_t swmi_semiglobal_long_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes, size_t cap);
SWMI_API int swmi_semiglobal_long_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                         void *d_moves, void *d_lengths, void *stream);
SWMI_API int swmi_semiglobal_long_release_workspaces(void);
SWMI_API int swmi_semiglobal_long_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                              const int8_t score_matrix[16], int8_t gap_penalty, void *d_scores, void *d_ends,
                                              void *d_moves, void *d_lengths, void *stream, int iters, float *avg_ms);
SWMI_API int swmi_semiglobal_long_expand_moves(const uint64_t *moves, uint32_t length, int32_t *traceback, size_t cap);
SWMI_API int swmi_semiglobal_long_affine(const uint8_t *seq1s, size_t len1, const uint8_t *seq2s, size_t len2, size_t n,
                                         const int8_t score_matrix[16], int gap_open, int gap_extend, int32_t *scores,
                                         int32_t *ends, uint64_t *moves, uint32_t *lengths);
SWMI_API size_t swmi_semiglobal_long_affine_slices_for(size_t n, size_t len1, size_t len2, int traceback, size_t *sizes,
                                                       size_t cap);
SWMI_API int swmi_semiglobal_long_affine_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2, size_t n,
                                                const int8_t score_matrix[16], int gap_open, int gap_extend, void *d_scores,
                                                void *d_ends, void *d_moves, void *d_lengths, void *stream);
SWMI_API int swmi_semiglobal_long_affine_release_workspaces(void);
SWMI_API int swmi_semiglobal_long_affine_time_device(const void *d_seq1s, size_t len1, const void *d_seq2s, size_t len2,
                                                     size_t n, const int8_t score_matrix[16], int gap_open, int gap_extend,
                                                     void *d_scores, void *d_ends, void *d_moves, void *d_lengths,
                                                     void *stream, int iters, float *avg_ms);

/* ---- the exact semi-global aligners on a batch of MIXED (len1, len2) ----------------------------------
 * swmi_semiglobal_full and swmi_semiglobal_full_affine with one (len1, len2) per alignment and one set of gaps per call.  The
 * arguments are swmi_local_full_ragged's: alignment k is seq1 = bytes [seq1_offsets[k], seq1_offsets[k+1]) of seq1s against
 * seq2 = bytes [seq2_offsets[k], seq2_offsets[k+1]) of seq2s; both offset arrays hold n + 1 non-decreasing entries, and every
 * length is in [0, 16384].  For two non-zero lengths scores[k], ends[2 k .. 2 k + 1] = the best cell (TWO int32 per alignment),
 * the moves in walking order (3 / 2 / 1 = diagonal / up / left) and lengths[k] = steps + 1 are, field for field, those of the
 * fixed-length entry called with that pair, in caller order.  Alignment k's moves start at word move_offsets[k]:
 * SWMI_SGFULL_MOVE_WORDS is SWMI_LOCAL_FULL_MOVE_WORDS, so swmi_local_full_ragged_move_offsets gives the layout, and there is
 * no second function for it; swmi_semiglobal_expand_moves(moves + move_offsets[k], lengths[k], ...) rebuilds a path.  moves
 * and lengths both NULL: ends-only.
 * ZERO LENGTHS follow from the definition extended to an empty sequence: the table is one border, every cell of which is <= 0,
 * and (0, 0) holds 0 and comes first.  So the score is 0, the best cell (0, 0), there is no move, and lengths[k] = 1 (the one
 * position (0, 0)), also at gap 0 -- NOT the local aligners' count of 0.  Ends-only gives the same score and cell.  No byte of
 * either sequence is read, and no move word is written.
 * Host buffers.  The batch runs in slices (swmi_semiglobal_full_ragged_slices_for) on two sets of device buffers, one launch
 * per wave count present in a slice, the widest first, and inside a launch the longest seq1 first; results go to caller
 * positions.  The checks run in this order: the matrix and the gaps, moves / lengths given both or neither, n = 0 (a no-op that
 * needs no device), the buffers, the offsets.  Errors: SWMI_ERR_INVALID_ARGUMENT for decreasing offsets, a length above 16384, a
 * NULL buffer, or only one of moves / lengths; SWMI_ERR_DOMAIN as in the fixed-length entries.  Every argument is checked
 * before any device is touched. */
SWMI_API int swmi_semiglobal_full_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                         const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int8_t gap_penalty,
                                         int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths);
SWMI_API int swmi_semiglobal_full_affine_ragged(const uint8_t *seq1s, const uint64_t *seq1_offsets, const uint8_t *seq2s,
                                                const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16], int gap_open,
                                                int gap_extend, int32_t *scores, int32_t *ends, uint64_t *moves, uint32_t *lengths);
/* The slices a ragged call of n alignments cuts its batch into (affine = 0: swmi_semiglobal_full_ragged, else the affine one;
 * traceback = 0: ends-only), in order; returns how many there are and writes the first `cap` sizes (NULL to count).  Each is
 * the longest run of the alignments left, in caller order, whose device bytes fit the fixed-length aligner's budget for one
 * slice (swmi_semiglobal_full_slices_for's or swmi_semiglobal_full_affine_slices_for's with a traceback; 256 MiB ends-only), at
 * most 2^20 alignments and at least one.  The bytes are counted as for the other ragged families (five result dwords per
 * alignment, an upper bound here).  Needs no device.  0 for invalid offsets. */
SWMI_API size_t swmi_semiglobal_full_ragged_slices_for(const uint64_t *seq1_offsets, const uint64_t *seq2_offsets, size_t n,
                                                       int affine, int traceback, size_t *sizes, size_t cap);
/* Same with every data buffer in device memory (16-byte aligned at its base; an alignment's offsets need no alignment),
 * asynchronous on `stream`; d_moves uses the move_offsets layout.  Both offset arrays stay HOST arrays, read during the call
 * only.  The codes and slots go to the workspace of the fixed-length entry per (GPU, stream)
 * (swmi_semiglobal_full_release_workspaces / swmi_semiglobal_full_affine_release_workspaces free it). */
SWMI_API int swmi_semiglobal_full_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                                const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                                int8_t gap_penalty, void *d_scores, void *d_ends, void *d_moves, void *d_lengths,
                                                void *stream);
SWMI_API int swmi_semiglobal_full_affine_ragged_device(const void *d_seq1s, const uint64_t *seq1_offsets, const void *d_seq2s,
                                                       const uint64_t *seq2_offsets, size_t n, const int8_t score_matrix[16],
                                                       int gap_open, int gap_extend, void *d_scores, void *d_ends, void *d_moves,
                                                       void *d_lengths, void *stream);

/* ---- deferred queue behind the per-pair signature -------------------------------------
 * Lets a per-pair caller (the reference's timing loop) keep its call shape while the
 * library batches: submit() copies the pair into pinned staging memory and returns its
 * ticket (0,1,2,...); full staging blocks are shipped to the GPU asynchronously;
 * swmi_queue_wait() drains everything and exposes scores[ticket]. */
typedef struct swmi_queue swmi_queue;
SWMI_API int swmi_queue_create(size_t max_pairs, const int8_t score_matrix[16], int8_t gap_penalty,
                               swmi_queue **out);
SWMI_API long long swmi_queue_submit(swmi_queue *q, const uint8_t seq1[SWMI_SEQ_LEN],
                                     const uint8_t seq2[SWMI_SEQ_LEN]);
SWMI_API int swmi_queue_wait(swmi_queue *q, const int32_t **scores, size_t *n_scores);
SWMI_API int swmi_queue_reset(swmi_queue *q);
SWMI_API int swmi_queue_destroy(swmi_queue *q);

/* ---- schedules ------------------------------------------------------------------------
 * The reference ships nine schedules of one semantics (simd .. simd9).  So does this
 * library: `lanes_per_alignment` L in {64,32,16,8,4,2} lanes of a 64-lane wavefront walk one
 * alignment's anti-diagonal (each lane owns 128/L consecutive rows); L = 64 is literally
 * "one wavefront per alignment".  0 (the default) lets the library choose by batch size: L = 4 from ~100 000 pairs per
 * launch on (fewest instructions per cell), more lanes per alignment below that (lowest latency: L = 64 up to 2048 pairs,
 * then 32, 16, 8); swmi_get_schedule reports 0 in that case.
 * flags (all give identical scores): bit 0 = never fold the gap into the matrix rows (general cell body);
 * bit 1 = 16-bit-max cell body; bit 2 = LDS score-lookup kernel (L in 16, 8, 4 and foldable parameters only);
 * bit 3 = never the packed kernel.  (Without it, L = 4, 8 and 16 -- what the automatic choice resolves to from 5121 pairs
 * up -- run sw128_pk_kernel<MODE, VARIANT, L>: two alignments per register and L lanes per PAIR of alignments, i.e. 32 / 16 / 8
 * alignments per wavefront, 16-bit cells, v_pk_maximum3_f16 as a packed integer max.  VARIANT is the cell body, chosen from
 * the parameters: 0 when every score_matrix entry + gap_penalty is >= 0 (e.g. (1,-1,1), the parameters of the reference's
 * SmithWaterman_8bit111simd, source.cpp:1105-1225: ~1.55x the int32 kernel), 2 when every entry + 2 * gap_penalty lies in
 * [0, 255] (e.g. (120,-120,62): ~1.4x), 1 otherwise (~1.3x).  Variant 2 has a FLAG FORM, which runs variant 0's cell inside
 * the variant-2 kernel (same reported name) and which the harness's (10,-30,15) gets (~1.55x).  It applies when ALL of:
 *   - the rule above gives 2;
 *   - every score_matrix entry is either one common value m with m + gap_penalty > 0, or <= -2 * gap_penalty (such a score
 *     never decides a cell: H(i,j-1) >= H(i-1,j-1) - gap);
 *   - (m + gap_penalty) divides 255 * gap_penalty (the recurrence is rescaled by 255 / (m + gap_penalty), exactly);
 *   - 255 * (128 * m + gap_penalty) / (m + gap_penalty) + 255 < 0x7C00 (the largest rescaled value).
 * (127,-127,64), (120,-120,62), (7,-30,15), (10,-29,15) do not qualify and keep the vertical-offset cell; (10,-40,15) is
 * variant 1 as before.  swmi_pk_cell_form (swmi_pk_form.h, libswmi_pk_form.so) reports the form without a device.
 * Where the flag form's enabled entries are exactly the four diagonal ones (plain match / mismatch scoring) and the largest
 * rescaled H, 255 * 128 * m / (m + gap_penalty), is at most 16383, it runs as its PRODUCT FORM: lookup and diagonal add of a
 * row are one 16-bit multiply-add (swmi_pk_product_form reports it; the harness's (10,-30,15) qualifies, same kernel name,
 * same scores).  The environment variable SWMI_PK_NO_PRODUCT, read at swmi_init, keeps such sets on the flag form's own cell.
 * DESIGN.md section 5a.) */
SWMI_API int swmi_set_schedule(int lanes_per_alignment, unsigned flags);
SWMI_API int swmi_get_schedule(int *lanes_per_alignment, unsigned *flags);
/* Lanes per alignment a launch of n pairs runs with under the current setting (what 0 = automatic resolves to). */
SWMI_API int swmi_schedule_for_batch(size_t n);
/* Which kernel instantiation a launch of n pairs with these parameters runs under the current setting, e.g.
 * "sw128_pk_kernel<0,1>" or "sw128_kernel<64,1,0,0>" (template arguments as tools/isa_census.py prints them), and how many
 * alignments one of its wavefronts scores.  mode: 0 = pairs, 1 = 2-bit packed input, 2 = one-vs-many.  For profiling
 * tools and bench.py, which derive the issue-bound fraction from the disassembly of exactly that kernel. */
SWMI_API int swmi_score_kernel_for_batch(size_t n, const int8_t score_matrix[16], int8_t gap_penalty, int mode,
                                         char *name, size_t name_len, int *alignments_per_wavefront);

/* Self-test of the premise the packed kernel rests on: gfx950's v_pk_maximum3_f16, applied to 16-bit integers in
 * [0, 0x7C00) held two per register, is a packed THREE-INPUT INTEGER MAX (such integers order like the half-precision
 * numbers with the same bit patterns; the kernels pin MODE.FP_DENORM so that the patterns below 1024, which are f16
 * denormals, are kept).  Runs the instruction on EVERY pair (a, b) of that range -- 31744^2 pairs, six operand
 * arrangements each, the third operand one of the two or a pseudo-random third value -- inside a kernel that sets the
 * mode exactly as the scoring kernels do, and compares with the integer maximum of each half on the device.
 * *checked = comparisons made (6 * 31744^2), *mismatches = how many failed (0 on gfx950).  No reference counterpart. */
SWMI_API int swmi_selftest_pk_max3(unsigned long long *checked, unsigned long long *mismatches);

/* ---- synthetic inputs ----------------------------------------------------
 * Counter-based generator, identical on host and device: pair p, sequence s (0/1), 64-bit
 * word w (0..3): x = splitmix64(seed ^ ((p*2+s)*4+w) * 0x9E3779B97F4A7C15); base k of the
 * word = (x >> 2k) & 3.  Stands in for the reference's mt19937_64 + uniform_int_distribution
 * draw (source.cpp:3033-3040), which is implementation-defined across standard libraries. */
SWMI_API int swmi_generate_pairs_device(void *d_seq1s, void *d_seq2s, size_t n, uint64_t seed,
                                        uint64_t first_pair, void *stream);
SWMI_API int swmi_generate_pairs_host(uint8_t *seq1s, uint8_t *seq2s, size_t n, uint64_t seed,
                                      uint64_t first_pair);

/* ---- measurement ----------------------------------------------------------------------
 * Launches the batch kernel `iters` times back to back on `stream` (NULL = the null stream)
 * bracketed by hipEvents on that same stream and returns the average per-launch duration. */
SWMI_API int swmi_time_batch_device(const void *d_seq1s, const void *d_seq2s, size_t n,
                                    const int8_t score_matrix[16], int8_t gap_penalty,
                                    void *d_scores, void *stream, int iters, float *avg_ms);

typedef struct swmi_device_info {
    int device;
    int compute_units;
    int clock_khz;
    int wavefront_size;
    size_t hbm_bytes;
    char arch[64];
    char name[128];
} swmi_device_info;
SWMI_API int swmi_get_device_info(swmi_device_info *info);

#ifdef __cplusplus
}
#endif
#endif /* SWMI_H */
