// tile_sweep.h -- what the any-length aligners share (sgfull_kernels.hip, sgfull_affine_kernels.hip,
// local_full_kernels.hip, local_full_affine_kernels.hip, global_full_kernels.hip, global_full_affine_kernels.hip,
// global_long_kernels.hip, global_long_affine_kernels.hip, local_long_kernels.hip, local_long_affine_kernels.hip,
// sgfull_long_kernels.hip, sgfull_long_affine_kernels.hip): the mapping and its constants, the helpers, the geometry and the launcher; the few helpers that the 16-lane local aligners take from here as well.  The sweep and the
// walk of the linear-gap kernels are tile_sweep_body.inc, those of the affine kernels tile_sweep_affine_body.inc.
//
// Mapping: ONE workgroup per alignment, W = ceil(len2 / 1024) wavefronts; lane l of wave w owns the 16 columns
// 16 G + 1 .. 16 G + 16 of G = 64 w + l.  Inside a wave, lane l computes row s - l + 1 at the wave's local step s; what
// the lane needs of the column to its left (H's key; with affine gaps F too) comes from lane l - 1 one step earlier (one
// v_mov_b32_dpp wave_shr:1 per dword and step).  Lane 0 of wave w > 0 takes it from lane 63 of wave w - 1 through an LDS
// ring of 256 rows per wave boundary; lane 0 of wave 0 takes the border.
//
// Ring timing: the waves run in CHUNKS of 32 steps separated by a workgroup barrier, wave w delayed by 3 chunks behind
// wave w - 1.  Lane 63 of wave w - 1 computes row r at its step r + 62, lane 0 of wave w needs it at its step r - 1, and
// floor((r + 62) / 32) - floor((r - 1) / 32) <= 2 < 3, so every ring entry is written a chunk before it is read; at most
// 64 rows separate the newest entry written from the oldest one still to read, so 256 entries never wrap onto one unread.
// Neither the step at which a lane computes a row nor the ring's indexing depends on the recurrence or on what an entry
// holds, so the argument holds for all four kernels.
//
// Columns past len2 (the last lanes of the last wave) are computed with every score -128 (the profile's padding); each
// kernel's file proves that the best-cell rule never picks one and that the walk never enters one.
//
// Best cell: per row one max chain over the lane's 16 stored keys names the row's largest H and its FIRST column (the low
// bits hold 15 - jj); it replaces the lane's best only when its H is strictly greater (compared against best | 63), so the
// lane keeps the first row.  Lanes and waves are reduced at the end (value desc, row asc, column asc).
//
// Codes: one code word (a dword, with affine gaps a qword) per lane and row.  A lane keeps the words of a trip (4 steps)
// and writes them with 16-byte stores, so a wave writes 1 or 2 KiB contiguous per trip: word
// ((w * n_trips + s / 4) * 64 + l) * 4 + s % 4 of the alignment's codes holds row s - l + 1 of lane l (code_index).
//
// Walk: after the sweep every wave drains its stores (s_waitcnt vmcnt(0): a workgroup-scope fence lowers to nothing here,
// DESIGN.md section 12) and the workgroup meets at a barrier; then the whole workgroup loads a block of 128 rows x
// kStageLanes lanes (64 dwords or 32 qwords: 32 KiB of LDS) of code words ending at the walk's cell into LDS (non-temporal
// loads: the stores went to L2), and one lane walks inside the block.  The walk only moves up and left, so every block
// takes it at least 128 rows or 16 kStageLanes columns further.  Moves are packed 32 to a word, first move in the low bits.
//
// tile_sweep_body.inc is that sweep and walk for a linear-gap VARIANT, a type that is built from the kernel's gap argument
// and supplies what depends on the recurrence:
//     Gaps                          the kernel's gap arguments as an aggregate
//     kStageLanes, kEnds            lanes of a staging block; int32 of `ends` per alignment (2: end cell; 4: start cell too)
//     kRowMin, kZeroKey             below every stored key (where a row's max chain starts); the stored key of H = 0
//     row0(jj, -j, gaps)            the stored key of row 0 in the lane's column jj (global column j)
//     border(-j), left_border(-i)   the stored key of H(0, j) = H(j, 0), column bits aside; that of column 0 in row i
//     cell<TB>(jj, sc, diag, left, key, code)
//                                   one cell with substitution score sc: diag, left and key hold its neighbours before and
//                                   ITS values after (diag the key above, for the next column); returns the stored key
//                                   and, with TB, the cell's bits of the row's code word
//     step(word, cc)                the walk's move (3 / 2 / 1 = diagonal / up / left, 0 = stop) at column cc of a word
//     kWalkStops                    whether a code can stop the walk (else it goes on to (0, 0), forced on the border)
// The borders take the NEGATED row or column so that the caller's sum folds into the negation as it did before the split.
//
// The END RULE (global_full_kernels.hip, global_full_affine_kernels.hip; DESIGN.md sections 20 and 21): a variant with a
// static member kFreeEnds = true -- the other variants have no such member, and kEndRule<V> is then false -- asks the body
// for another best cell and another end of the walk.  Its kernel has an argument `free_ends` (uniform, so in SGPRs; a kernel without one finds tile::free_ends = 0 below),
// a mask of kFreeBegin1 / kFreeBegin2 (column 0 / row 0 hold 0: the variant's left_border / row0 and border follow them) and
// kFreeEnd1 / kFreeEnd2 (the end cell may lie anywhere in column len2 / row len1).  Such a variant has kWalkStops = false,
// kEnds = 4 and kRowMin below every key.  With it
//     the sweep keeps no row maximum: the one lane that owns column len2 reads that column's key from the finished row (only
//     with kFreeEnd1), so the loop has no max chain over the cells;
//     after the sweep key[] holds row len1: each lane takes the largest key of its columns <= len2 (kFreeEnd2; the key's low
//     bits name the first such column), the owner of column len2 the corner, thread 0 the border cells (0, len2) and
//     (len1, 0) in closed form; columns past len2 are masked out, so no proof about them is needed;
//     the reduction packs H + kEndBias above the row and column fields (end_pack), so that a negative H orders as it should:
//     H descending, row ascending, column ascending, as for the other variants;
//     the walk runs as staged while i > 0 and j > 0; on a border it ends if that border is free, else goes on to (0, 0) by
//     forced moves; the count is the moves, ends[2..3] the cell where it ended.
//
// tile_sweep_affine_body.inc is the sweep and walk for an affine-gap variant, a type of static members only (the body reads
// the kernel's gap_open and gap_extend itself).  The key array, E's array, the column loop and the E / F recurrences stay in
// the body; the variant supplies
//     kEnds, kWalkStops, kRowMin    as above; where kWalkStops, the code that stops the walk is kTagH's + 1 (the floor's)
//     kTagH, kTagE, kTagF           tag << 4 of a stored H key (also the key of H = 0 and, >> 4, the walk's diagonal code), of
//                                   E and of F as kept with a traceback
//     kOpenBitE, kOpenBitF          the bit of E's / F's winner that is set when the gap opens (kTagH has it, the gap's tag not)
//     row0(jj, j, open, extend)     the stored key of row 0 in the lane's column jj (global column j)
//     border(j, open, extend)       the stored key of H(0, j) = H(j, 0), column bits aside
//     floor(m)                      H's largest candidate m with the zero floor joined, or m itself
// With the end rule (a variant with kFreeEnds = true; its kernel names free_ends) the affine body keeps one (open, extend) per
// border, (0, 0) where the mask frees it, and hands border() and row0() that border's pair; E on row 0 and F on column 0 stay
// -inf.  It reads the last column's key of row i - 1 before it computes row i, through the same uniform switch, where the
// linear body reads row i's from the finished row: the body says why.  Thread 0 packs the two border cells before the sweep
// and keeps them in VGPRs.  The last row, the corner, the reduction and the walk's tail are the linear body's.
//
// Ragged launches (the two local, the two global and the two semi-global kernels; DESIGN.md sections 19, 22 and 27): a kernel with a template parameter RAGGED has a last
// parameter `work` (NULL and unread in a fixed launch; last, so that every other argument lies where it did), and with RAGGED
// takes its alignment from one TileWork per workgroup, `slot` = work[blockIdx.x], instead of from k = blockIdx.x and the
// launch's one (len1, len2): its sequences, lengths, trips, code block, move row and result index.  The slot is loaded through an address
// that is uniform by construction, so all of it stays in SGPRs.  Both bodies read the names RAGGED and slot; a kernel without
// a ragged form (the striped kernels) finds tile::RAGGED = false and an empty tile::slot below, and a kernel with one shadows both.  One
// launch serves one wave count: every slot of a launch has W = blockDim.x >> 6, so no wave ever leaves before the
// workgroup's last barrier -- except that a slot with a zero length, which runs in a W = 1 launch, returns as a whole
// workgroup, on a uniform test, before the first barrier and before any load from either sequence.  What it writes first is
// "score 0 at (0, 0)" with the count that the variant's walk would write there -- the local aligners' 0 moves, the semi-global
// pair's path of 1 position -- or with the end rule the closed form of end_rule_zero_length below.
//
// Why the bodies are includes, and why there are two: this compiler optimises a function on its own before it inlines it.
// A body behind a call -- even the unchanged kernel moved into a forceinline function -- is optimised twice and came out
// with 12 fewer SGPRs and 30 more instructions per sweep loop in the linear traceback kernels; a variant that held the key
// array or the column loop lost the array-to-vector promotion (68 VGPRs for 119).  As text inside the named kernel each pair
// compiles to the code it had.  The affine pair needs two values in the carry and two dwords in the code word; behind
// generic carry and code types of the linear body they became other allocas, other registers and other loops (DESIGN.md
// section 13), so it has a body of its own, written with the concrete types both affine kernels had (an int2 ring, separate
// H and F arrays, two code dwords): from it both compile to the parent's instructions, one for one.
#pragma once
#include "swmi_internal.h"

#include <type_traits>

namespace swmi {

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int max3(int a, int b, int c) { return imax(imax(a, b), c); }

// cols[b] = bytes a = 0..3: sm[a*4 + b] -- the column of the score matrix that a seq2 base b selects
struct SmCols {
    uint32_t c[4];
};

inline SmCols sm_cols(const int8_t *sm)
{
    SmCols cols;
    for (int b = 0; b < 4; ++b) {
        uint32_t c = 0;
        for (int a = 0; a < 4; ++a) c |= uint32_t(uint8_t(sm[4 * a + b])) << (8 * a);
        cols.c[b] = c;
    }
    return cols;
}

namespace tile {

constexpr int kCols = 16;              // columns per lane
constexpr int kMaxWaves = 16;          // 16 x 64 x 16 = 16384 columns
constexpr int kUnroll = 4;             // steps per trip (one or two 16-byte code stores)
constexpr int kChunk = 32;             // steps between two workgroup barriers
constexpr int kDelay = 3;              // chunks between wave w - 1 and wave w
constexpr int kRing = 256;             // rows of each wave boundary's LDS ring
constexpr int kStageRows = 128;        // rows of a walk staging block

constexpr bool RAGGED = false;         // what a kernel without a ragged form sees (above)
constexpr TileWork slot{};

// Column stripes (global_long_kernels.hip, global_long_affine_kernels.hip, with a local variant local_long_kernels.hip,
// local_long_affine_kernels.hip, and with a semi-global one sgfull_long_kernels.hip, sgfull_long_affine_kernels.hip; DESIGN.md
// sections 23, 25 and 26): a kernel that shadows STRIPED
// with true sweeps len2 > kStripeCols columns as stripes of kStripeCols, one after another, in the same workgroup; it names
// `carry` (linear body: int per row) or `carry_hf` (affine body: int2 per row), the per-alignment device buffer through which
// a stripe's last column reaches the next stripe's wave 0.  What every other kernel sees:
constexpr bool STRIPED = false;
constexpr int *carry = nullptr;
constexpr int2 *carry_hf = nullptr;
// (a kernel that is RAGGED and STRIPED -- wide_long_affine_kernels.hip -- also names `carry_stride`: slot.pad * carry_stride
// entries into carry_hf lies the slot's carry block, for the slots of one launch differ in len1)
constexpr uint32_t carry_stride = 0;
constexpr int kStripeCols = 64 * 16 * 16;   // kMaxWaves x 64 lanes x kCols columns (asserted below)

// Where a cell's substitution score comes from (wide_affine_kernels.hip): a kernel that shadows WIDE with
// true scores over 32 letters.  It names `wide_sm`, the 32 x 32 int8 matrix in device memory, and `wide_prof`, its profile in
// LDS: per wave 32 letter rows of 64 lanes x 16 bytes, a lane's 16 column scores of letter a at wide_prof[(32 w + a) 64 + l],
// which the lane itself builds before its sweep and reads back a row at a time (wide_row below), one trip ahead of use.  Such
// a kernel has no `cols`, so it names an empty one; the walk's staging block takes the profile's place after the sweep's last
// barrier.  What every other kernel sees (the affine body alone reads these names):
constexpr bool WIDE = false;
constexpr const int8_t *wide_sm = nullptr;
constexpr uint4 *wide_prof = nullptr;
// A WIDE kernel whose column scores are the caller's, one column of 32 scores per position of seq2's side and no seq2 at all
// (wide_profile_kernels.hip), shadows PROFILED with true as well and names `wide_pssm` in place of
// wide_sm: the profile in device memory in the lane-ready form, letter-major, 32 rows of 64 W uint4, byte jj of entry G of row
// a the score of letter a in column 16 G + jj + 1 (-128 past len2).  The lane loads its 32 entries where the others build them.
constexpr bool PROFILED = false;
constexpr const uint4 *wide_pssm = nullptr;

// The end rule (above).  The flags are SWMI_FREE_* of include/swmi.h, which no kernel file includes.
constexpr unsigned kFreeBegin1 = 1, kFreeBegin2 = 2, kFreeEnd1 = 4, kFreeEnd2 = 8;
constexpr unsigned free_ends = 0;      // what a kernel without the argument sees
constexpr int kEndBias = 1 << 22;      // |H| <= 128 * 32768 = 2^22, and the bound is never met: H + kEndBias > 0
                                       // (a striped kernel shadows it: its |H| reaches 2^23)
static_assert(kStripeCols == kMaxWaves * 64 * kCols);

template <class V, class = void>
constexpr bool kEndRule = false;
template <class V>
constexpr bool kEndRule<V, std::void_t<decltype(V::kFreeEnds)>> = V::kFreeEnds;

// a candidate end cell for the reduction's maximum: H descending, row ascending, column ascending; above 0, which no cell packs to
// (`bias`: the kEndBias that the calling kernel sees)
__device__ __forceinline__ unsigned long long end_pack(int h, int row, int col, int bias)
{
    return ((unsigned long long)(uint32_t)(h + bias) << 34) | ((unsigned long long)(0x1FFFF - row) << 17) |
           (unsigned long long)(0x1FFFF - col);
}

__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__host__ __device__ inline int waves(int len2) { return (len2 + 64 * kCols - 1) / (64 * kCols); }

__host__ __device__ inline size_t trips(int len1) { return (size_t)((len1 + 63 + kChunk - 1) / kChunk) * (kChunk / kUnroll); }

// code words per alignment: one per lane for every step of the padded sweep
__host__ __device__ inline size_t code_words(int len1, int len2) { return (size_t)waves(len2) * trips(len1) * 256; }

// the code word of row i, lane G (i >= 1)
__device__ __forceinline__ size_t code_index(int i, int G, uint32_t n_trips)
{
    const int w = G >> 6, l = G & 63, s = i + l - 1;
    return (((size_t)w * n_trips + (uint32_t)(s >> 2)) * 64 + l) * 4 + (s & 3);
}

// the same register in lane l - 1 of the wave; lane 0 gets `edge`
__device__ __forceinline__ int from_left(int edge, int v)
{
    return __builtin_amdgcn_update_dpp(edge, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

// 8 * (seq1[idx] & 3), the load clamped into the sequence (so that it issues a trip ahead of its use)
__device__ __forceinline__ int base_shift(const uint8_t *s1, int idx, int len1)
{
    const int c = idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx;
    return 8 * (s1[c] & 3);
}

// A WIDE kernel's form of it: 64 * (seq1[idx] & 31), the letter's row in the lane's view of the profile (in uint4)
__device__ __forceinline__ int wide_row(const uint8_t *s1, int idx, int len1)
{
    const int c = idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx;
    return 64 * (s1[c] & 31);
}

// dword x (a constant) of a profile row
__device__ __forceinline__ uint32_t wide_dword(const uint4 &v, int x) { return x == 0 ? v.x : x == 1 ? v.y : x == 2 ? v.z : v.w; }

// The carry entry that a lane of a striped kernel's wave 0 loads for the row `idx` + 1, clamped into the buffer.  Only lane
// 0's value is used (it is from_left's `edge`), and lane 0 asks for the row it needs; the other lanes' indices run backwards
// from it, so that the load is one coalesced vector load and not a scalar load of memory that this kernel writes.
__device__ __forceinline__ int carry_row(int idx, int len1) { return idx < 0 ? 0 : idx >= len1 ? len1 - 1 : idx; }

__device__ __forceinline__ uint4 code_quad(const unsigned long long *c)
{
    return make_uint4((uint32_t)c[0], (uint32_t)(c[0] >> 32), (uint32_t)c[1], (uint32_t)(c[1] >> 32));
}

// v itself, which with ON the compiler may not look through: nothing derived from the result is computed before this point.
// The end rule's ragged kernels read len2 through it after the sweep.  Without it the compiler evaluates the last row's sixteen
// column tests (j <= len2, j == len2) before the sweep and keeps the lane masks in SGPR pairs across it; the fixed-length
// kernels fit that in their SGPRs with none to spare, the ragged ones, with a slot to hold, spilled up to 7 SGPRs into a VGPR.
template <bool ON>
__device__ __forceinline__ int opaque(int v)
{
    if constexpr (ON) asm volatile("" : "+s"(v));
    return v;
}

// The same for a per-lane value.  A striped kernel re-derives its lane and wave from it in every stripe, so that nothing made
// of them -- the first rows' base shifts, addresses, the border candidates -- is hoisted out of the stripe loop and kept in
// registers across the sweep.
template <bool ON>
__device__ __forceinline__ int opaque_lane(int v)
{
    if constexpr (ON) asm volatile("" : "+v"(v));
    return v;
}

// Whether the thread is lane 0 of its wavefront, made of no register that lives anywhere else.  The zero-length arm of a
// ragged semi-global kernel elects its writer with it (the slot's workgroup is one wavefront, so lane 0 is thread 0).  The
// compiler places that arm behind the sweep in the structured control flow; elected by threadIdx.x, the arm kept the thread id
// in a VGPR across the whole sweep, which made the affine ends-only kernel one VGPR larger than its fixed sibling.
__device__ __forceinline__ bool first_lane() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u; }

// the slot of a ragged launch's workgroup; nothing is loaded for a fixed launch
template <bool RAGGED>
__device__ __forceinline__ TileWork load_slot(const TileWork *work)
{
    if constexpr (RAGGED) return work[blockIdx.x];
    else return TileWork{};
}

// A ragged slot with a zero length under the end rule: the table is one border, `steps` = the other
// sequence's length cells long, and everything is a closed form of the mask.  With len2 == 0 the border is column 0 (its
// begin flag kFreeBegin1, its end flag kFreeEnd1, the forced move "up" = 2), with len1 == 0 row 0 (kFreeBegin2, kFreeEnd2,
// "left" = 1); `cost` is what the whole border costs as one gap.  A free end: every border cell holds at most 0 and (0, 0)
// holds 0 and comes first, so the end cell is (0, 0) -- also at gap 0.  Else the end cell is the far corner: with a free
// begin it holds 0 and the walk ends on it, else it holds -cost and the walk is `steps` forced moves, whole words of one
// code (bits past the last step are unspecified).  The slot's workgroup is one wavefront; it writes the words lane-strided,
// with vector stores, inside the slot's move row.  No byte of either sequence is read.
template <bool TB>
__device__ __forceinline__ void end_rule_zero_length(int len1, int len2, unsigned free_ends, int cost, size_t k, int32_t *scores,
                                                     int32_t *ends, unsigned long long *mv, uint32_t *counts)
{
    const bool up = len2 == 0;
    const bool forced = (len1 | len2) != 0 && !(free_ends & (up ? kFreeEnd1 : kFreeEnd2));   // the end cell is the far corner
    const bool walks = forced && !(free_ends & (up ? kFreeBegin1 : kFreeBegin2));
    const uint32_t steps = walks ? (uint32_t)(len1 + len2) : 0u;
    if (threadIdx.x == 0) {
        scores[k] = walks ? -cost : 0;
        ends[4 * k + 0] = forced ? len1 : 0;
        ends[4 * k + 1] = forced ? len2 : 0;
        ends[4 * k + 2] = !TB ? -1 : forced && !walks ? len1 : 0;
        ends[4 * k + 3] = !TB ? -1 : forced && !walks ? len2 : 0;
        if constexpr (TB) counts[k] = steps;
    }
    if constexpr (TB) {
        const unsigned long long word = up ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull;
        for (uint32_t x = threadIdx.x; x < (steps + 31) >> 5; x += blockDim.x) mv[x] = word;
    }
}

// launches k with `args`, and with a last argument of nullptr when k takes one more (the `work` of a kernel with a ragged form)
template <class... P, class... A>
void fire(void (*k)(P...), dim3 grid, dim3 block, hipStream_t stream, A... args)
{
    if constexpr (sizeof...(P) == sizeof...(A) + 1) hipLaunchKernelGGL(k, grid, block, 0, stream, args..., nullptr);
    else hipLaunchKernelGGL(k, grid, block, 0, stream, args...);
}

// Launches KTb (codes, walk) or KEnds (d_moves NULL: no codes, no walk; d_codes and d_counts unused), one workgroup of
// waves(len2) wavefronts per alignment; `gaps` are the kernels' gap arguments.
template <auto KTb, auto KEnds, class Code, class... Gaps>
hipError_t launch(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm, int32_t *d_scores,
                  int32_t *d_ends, Code *d_codes, unsigned long long *d_moves, uint32_t *d_counts, size_t move_words,
                  hipStream_t stream, Gaps... gaps)
{
    if (n == 0) return hipSuccess;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)n), block(64 * waves(len2));
    const uint32_t n_trips = (uint32_t)trips(len1);
    if (d_moves)
        fire(KTb, grid, block, stream, d_seq1s, d_seq2s, len1, len2, cols, gaps..., d_scores, d_ends, d_codes, d_moves, d_counts,
             (uint32_t)move_words, n_trips);
    else
        fire(KEnds, grid, block, stream, d_seq1s, d_seq2s, len1, len2, cols, gaps..., d_scores, d_ends, (Code *)nullptr,
             (unsigned long long *)nullptr, (uint32_t *)nullptr, 0u, n_trips);
    return hipGetLastError();
}

// The ragged sibling: n slots of d_work, all of wave count `waves`, one workgroup of that many wavefronts each (KTb, KEnds: the
// RAGGED instantiations).  The launch's own lengths, move_words and n_trips are unused (0): the slot holds them.
template <auto KTb, auto KEnds, class Code, class... Gaps>
hipError_t launch_ragged(const uint8_t *d_seq1s, const uint8_t *d_seq2s, const TileWork *d_work, size_t n, int waves, const int8_t *sm,
                         int32_t *d_scores, int32_t *d_ends, Code *d_codes, unsigned long long *d_moves, uint32_t *d_counts,
                         hipStream_t stream, Gaps... gaps)
{
    if (n == 0) return hipSuccess;
    if (waves < 1 || waves > kMaxWaves || n > (size_t(1) << 20)) return hipErrorInvalidValue;
    const SmCols cols = sm_cols(sm);
    const dim3 grid((unsigned)n), block(64 * waves);
    if (d_moves)
        hipLaunchKernelGGL(KTb, grid, block, 0, stream, d_seq1s, d_seq2s, 0, 0, cols, gaps..., d_scores, d_ends, d_codes, d_moves,
                           d_counts, 0u, 0u, d_work);
    else
        hipLaunchKernelGGL(KEnds, grid, block, 0, stream, d_seq1s, d_seq2s, 0, 0, cols, gaps..., d_scores, d_ends, (Code *)nullptr,
                           (unsigned long long *)nullptr, (uint32_t *)nullptr, 0u, 0u, d_work);
    return hipGetLastError();
}

// The striped sibling (a kernel with STRIPED, whose last parameter is its carry buffer): one workgroup of
// min(waves(len2), kMaxWaves) wavefronts per alignment, which sweeps ceil(len2 / kStripeCols) stripes.  d_carry: len1 entries
// per alignment of the launch, unused (may be NULL) when len2 <= kStripeCols.
template <auto KTb, auto KEnds, class Code, class Carry, class... Gaps>
hipError_t launch_striped(const uint8_t *d_seq1s, const uint8_t *d_seq2s, int len1, int len2, size_t n, const int8_t *sm,
                          int32_t *d_scores, int32_t *d_ends, Code *d_codes, unsigned long long *d_moves, uint32_t *d_counts,
                          size_t move_words, Carry *d_carry, hipStream_t stream, Gaps... gaps)
{
    if (n == 0) return hipSuccess;
    if (len1 < 1 || len2 < 1 || len1 > 4 * kStripeCols || len2 > 4 * kStripeCols || (len2 > kStripeCols && !d_carry))
        return hipErrorInvalidValue;
    const SmCols cols = sm_cols(sm);
    const int w = waves(len2);
    const dim3 grid((unsigned)n), block(64 * (w < kMaxWaves ? w : kMaxWaves));
    const uint32_t n_trips = (uint32_t)trips(len1);
    if (d_moves)
        hipLaunchKernelGGL(KTb, grid, block, 0, stream, d_seq1s, d_seq2s, len1, len2, cols, gaps..., d_scores, d_ends, d_codes, d_moves,
                           d_counts, (uint32_t)move_words, n_trips, d_carry);
    else
        hipLaunchKernelGGL(KEnds, grid, block, 0, stream, d_seq1s, d_seq2s, len1, len2, cols, gaps..., d_scores, d_ends,
                           (Code *)nullptr, (unsigned long long *)nullptr, (uint32_t *)nullptr, 0u, n_trips, d_carry);
    return hipGetLastError();
}

}  // namespace tile
}  // namespace swmi
