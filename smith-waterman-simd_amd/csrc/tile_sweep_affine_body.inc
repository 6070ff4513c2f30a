// tile_sweep_affine_body.inc -- the sweep and the walk of an AFFINE-gap tile aligner: the body of its kernel (tile_sweep.h
// tells the mapping and what an affine variant V supplies).  Included INSIDE the kernel, after `using V = <variant>;`,
// where the kernel's parameters are named seq1s, seq2s, len1, len2, cols, gap_open, gap_extend, scores, ends, codes, moves,
// counts, move_words, n_trips and its template parameter TB.  A kernel with a ragged form also names RAGGED and slot, and
// then len1, len2 and n_trips are the slot's (tile_sweep.h).  A kernel whose variant has the end rule (kEndRule<V>,
// tile_sweep.h) also names free_ends.  A kernel that sweeps column stripes shadows STRIPED and kEndBias and names `carry_hf`
// (tile_sweep.h; tile_sweep_body.inc tells the stripe loop, which is the same here with (H, F) pairs in the carry); one that is
// RAGGED as well names `carry_stride` and finds its carry block through slot.pad (wide_long_affine_kernels.hip).  A kernel
// over 32 letters shadows WIDE and names wide_sm and wide_prof (tile_sweep.h, wide_affine_kernels.hip): where a cell's score
// comes from is the one thing that changes, and every `if constexpr (WIDE)` below is that.  One that also shadows PROFILED
// names wide_pssm and an empty seq2s (tile_sweep.h, wide_profile_kernels.hip): it loads the profile that the others build.
// Text and not a function on purpose: tile_sweep.h says why.
//
// E runs down a column and stays with the lane; F runs along the row, so what lane l - 1 hands over (and lane 63 through
// the ring) is its H(i, 16 G) AND its F(i, 16 G): two v_mov_b32_dpp wave_shr:1 per step, (H, F) pairs in the ring.  With a
// traceback E and F are kept masked to V's tags (one v_and_or_b32 after their max); ends-only they are not.
//
// Code word: 4 bits per cell, one qword per lane and row.  The low dword holds the tag of H's winner in the lane's 16
// columns (2 bits each, column jj at bits 2 jj); the high dword E's open bit of column jj at bit jj and F's at bit
// 16 + jj.  A staging block of the walk is 128 rows x 32 lanes (512 columns) of qwords.
//
// Walk: one lane, in state H / E / F, carried from block to block.  In H it reads the cell's H code -- the floor's (V::kTagH's
// code + 1, where V::kWalkStops) ends the walk on that cell -- and goes on in the state the code names; a cell's H code is not
// consulted inside E or F.  H takes a diagonal; E an up and F a left step, back to H where that cell's open bit is set.  E(1,j)
// and F(i,1) always open (E(0,j) = F(i,0) = -inf), so the walk reaches row 0 or column 0 in state H.
    constexpr int kStageLanes = 32;
    constexpr int kMinusInf = -(1 << 30);               // E on row 0, F on column 0
    __shared__ int2 ring[(kMaxWaves - 1) * kRing];
    __shared__ unsigned long long red[kMaxWaves];
    __shared__ int walk_at[V::kWalkStops ? 3 : 2];
    // (a WIDE kernel stages the walk's blocks where its profile lay: nothing reads the profile after the sweep's last barrier)
    __shared__ unsigned long long stage_lds[TB && !WIDE ? kStageRows * kStageLanes : 1];
    unsigned long long *const stage = WIDE ? reinterpret_cast<unsigned long long *>(wide_prof) : stage_lds;

    const int W = blockDim.x >> 6;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const size_t k = RAGGED ? (size_t)slot.k : (size_t)blockIdx.x;
    const uint8_t *s1 = seq1s + (RAGGED ? (size_t)slot.s1_off : k * (size_t)len1);
    // (a PROFILED kernel has no seq2: it names an empty seq2s, and nothing below reads s2)
    [[maybe_unused]] const uint8_t *s2 = PROFILED ? nullptr : seq2s + (RAGGED ? (size_t)slot.s2_off : k * (size_t)len2);
    if constexpr (RAGGED) {
        // a slot with a zero length: the whole workgroup (one wavefront) leaves here, before any barrier and any sequence load
        if (len1 == 0 || len2 == 0) {
            if constexpr (kEndRule<V>) {
                // the end rule's closed form of one border (tile_sweep.h); an affine gap run of L >= 1 cells costs open + (L - 1) extend
                end_rule_zero_length<TB>(len1, len2, free_ends, gap_open + (len1 + len2 - 1) * gap_extend, k, scores, ends,
                                         TB ? moves + (size_t)slot.move_base : nullptr, counts);
            } else if (V::kWalkStops ? tid == 0 : first_lane()) {   // (first_lane: tile_sweep.h says why)
                scores[k] = 0;
                ends[V::kEnds * k + 0] = 0;
                ends[V::kEnds * k + 1] = 0;
                for (int x = 2; x < V::kEnds; ++x) ends[V::kEnds * k + x] = TB ? 0 : -1;
                // the count the variant's walk would write from (0, 0) (tile_sweep_body.inc): its moves, or the path's cells
                if constexpr (TB) counts[k] = V::kWalkStops ? 0u : 1u;
            }
            return;
        }
    }
    // STRIPED: tile_sweep_body.inc's stripe loop, carry ordering and BARRIER INVARIANT (every wave executes total_chunks + 1
    // barriers in every stripe but the last and total_chunks in the last, whatever w and the stripe's valid width); the
    // carry holds the last column's stored key AND its F, so a gap that opened left of the stripe's edge extends across it.
    // A local variant's best cell of each stripe is folded into r as in the linear body.
    // (a RAGGED striped kernel's slots differ in len1: each names its carry block, slot.pad, in units of the launch's carry_stride)
    [[maybe_unused]] int2 *const carry_k = !STRIPED ? nullptr
                                           : RAGGED ? carry_hf + (size_t)slot.pad * (size_t)carry_stride
                                                    : carry_hf + k * (size_t)len1;
    unsigned long long r = 0;                           // best cell so far: (H desc, row asc, column asc)
    // A striped kernel without the end rule (a local variant) keeps its best cell so far per wave in red[w], not in r: two VGPRs
    // that it has not got across the sweep.  Only lane 0 of wave w touches red[w] before the last barrier.
    constexpr bool kFoldInLds = STRIPED && !kEndRule<V>;
    if constexpr (kFoldInLds) {
        if (l == 0) red[w] = 0;
    }
    int stripe = 0;
    do {
    // (a striped kernel's per-stripe tid, w and l: opaque_lane, tile_sweep.h; they shadow the workgroup's, which they equal)
    const int tid = opaque_lane<STRIPED>((int)threadIdx.x), w = tid >> 6, l = tid & 63;
    const int G = STRIPED ? stripe * (kStripeCols / kCols) + tid : tid;   // (lanes per stripe: not 64 kMaxWaves, which sizes the ring)
    const int gw = STRIPED ? G >> 6 : w;                // the wave of G in the code layout
    // whether another stripe follows (nothing but len2 and `stripe` is kept across the sweep: the kernels have no SGPRs to spare)
    const bool more_stripes = STRIPED && (stripe + 1) * kStripeCols < len2;
    const int code_waves = STRIPED ? waves(len2) : W;   // the wave count of the code layout: all stripes' waves
    const int jbase = kCols * G;                        // the lane's columns are jbase + 1 .. jbase + 16
    // what a gap along row 0 / column 0 costs: the kernel's, or with the end rule 0 where that border is free
    int open_row0 = gap_open, ext_row0 = gap_extend, open_col0 = gap_open, ext_col0 = gap_extend;
    if constexpr (kEndRule<V>) {
        if (free_ends & kFreeBegin2) open_row0 = ext_row0 = 0;
        if (free_ends & kFreeBegin1) open_col0 = ext_col0 = 0;
    }

    uint32_t prof[kCols];
    int key[kCols], e[kCols];                           // H's stored keys and E of the row the lane computed last
    // (a striped local kernel's row 0 is sixteen constants: made of a 0 that the compiler cannot see through, so that they are
    // set up anew in every stripe and not kept across the sweeps, tile_sweep_body.inc)
    [[maybe_unused]] const int row0_zero = opaque_lane<STRIPED && !kEndRule<V>>(0);
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const int j = jbase + jj + 1;
        if constexpr (WIDE) {
            // the column's letter, for the profile below (PROFILED: the columns have no letters)
            if constexpr (!PROFILED) prof[jj] = s2[j <= len2 ? j - 1 : 0] & 31u;
        } else {
            const uint32_t b = s2[j <= len2 ? j - 1 : 0] & 3u;
            prof[jj] = j > len2 ? 0x80808080u : b == 0 ? cols.c[0] : b == 1 ? cols.c[1] : b == 2 ? cols.c[2] : cols.c[3];
        }
        key[jj] = V::row0(jj, j, open_row0, ext_row0);
        if constexpr (STRIPED && !kEndRule<V>) key[jj] |= row0_zero;
        e[jj] = kMinusInf;
    }
    // WIDE: the lane's 16 bytes of every letter's profile row, from the matrix (columns past len2: -128).  A lane reads back
    // only what it wrote itself, so the profile needs no barrier.
    [[maybe_unused]] const uint4 *const prof_lane = wide_prof + (WIDE ? w * (32 * 64) + l : 0);
    if constexpr (WIDE && PROFILED) {
        // ... or, PROFILED, from the launch's profile in device memory, which the host laid out for exactly this: per letter
        // row one 16-byte load, coalesced over the lanes, and one LDS store; the padding is in the rows already
#pragma unroll 8
        for (int a = 0; a < 32; ++a) wide_prof[(w * 32 + a) * 64 + l] = wide_pssm[a * (64 * W) + 64 * w + l];
    } else if constexpr (WIDE) {
#pragma unroll 1
        for (int a = 0; a < 32; ++a) {
            uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int jj = 0; jj < kCols; ++jj) {
                const uint32_t v = jbase + jj + 1 > len2 ? 0x80u : (uint32_t)(uint8_t)wide_sm[a * 32 + (int)prof[jj]];
                d[jj >> 2] |= v << (8 * (jj & 3));
            }
            wide_prof[(w * 32 + a) * 64 + l] = make_uint4(d[0], d[1], d[2], d[3]);
        }
    }
    // end rule: the border cells (0, len2) and (len1, 0) are closed forms; thread 0 holds them as candidates from here on (in
    // two VGPRs: kept as scalars until after the sweep, the borders' gaps cost SGPRs that the traceback kernel has not got)
    [[maybe_unused]] unsigned long long r_border = 0;
    if constexpr (kEndRule<V>) {
        if (tid == 0) {
            if (free_ends & kFreeEnd1) r_border = end_pack(V::border(len2, open_row0, ext_row0) >> 6, 0, len2, kEndBias);
            if (free_ends & kFreeEnd2)
                r_border = umax64(r_border, end_pack(V::border(len1, open_col0, ext_col0) >> 6, len1, 0, kEndBias));
        }
    }
    const int g_open = -(gap_open << 6);
    const int g_ext = -(gap_extend << 6);
    int diag_in = V::border(jbase, open_row0, ext_row0);   // key(0, jbase)
    int f_last = kMinusInf;                             // F(i, jbase + 16) of the lane's last row, for lane l + 1
    int best = kEndRule<V> ? V::kRowMin : V::kTagH, best_row = 0;   // H = 0 at (0, 0); end rule: no last-column cell yet
    // end rule: the lane that owns column len2 keeps the best cell of that column, if seq1's end is free.  end_sel is that
    // column's jj in the last wave and -1 anywhere else (uniform, made scalar here).  Every lane of the last wave tracks its
    // column jj = end_sel, and only the owner's is read after the sweep, so the loop holds no lane mask.
    [[maybe_unused]] int end_sel = -1;
    if constexpr (kEndRule<V>)
        end_sel = __builtin_amdgcn_readfirstlane((free_ends & kFreeEnd1) && (STRIPED ? gw == (len2 - 1) >> 10 : w == W - 1)
                                                     ? (len2 - 1) & (kCols - 1)
                                                     : -1);

    const int local_chunks = (len1 + 63 + kChunk - 1) / kChunk;
    // a striped kernel's wave with no column in the (last) stripe: no chunk of work, every barrier
    const int my_chunks = STRIPED && jbase - (l << 4) >= len2 ? 0 : local_chunks;
    const int total_chunks = local_chunks + kDelay * (W - 1);
    const int2 *ring_in = ring + (w > 0 ? w - 1 : 0) * kRing;  // read by waves 1.. (wave 0's left column is the border)
    int2 *ring_out = ring + (w < W - 1 ? w : 0) * kRing;       // written by waves ..W-2
    unsigned long long *cw_out = TB ? codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)code_waves * n_trips * 256)) +
                                          ((size_t)gw * n_trips * 64 + l) * 4
                                    : nullptr;

    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) sh_next[t] = WIDE ? wide_row(s1, t - l, len1) : base_shift(s1, t - l, len1);
    // WIDE: sh_next holds the rows' places in the profile, two trips ahead, and pr_next the profile rows themselves, one trip
    // ahead: the LDS read of a row is issued a trip before the row's first cell, behind the load of its letter a trip earlier
    [[maybe_unused]] uint4 pr_next[kUnroll];
    if constexpr (WIDE) {
#pragma unroll
        for (int t = 0; t < kUnroll; ++t) {
            pr_next[t] = prof_lane[sh_next[t]];
            sh_next[t] = wide_row(s1, kUnroll + t - l, len1);
        }
    }

    for (int c = 0; c < total_chunks; ++c) {
        const int lc = c - kDelay * w;
        if (lc >= 0 && lc < my_chunks) {
            for (int q = 0; q < kChunk / kUnroll; ++q) {
                const int s0 = lc * kChunk + q * kUnroll;
                int sh[kUnroll], bound_h[kUnroll], bound_f[kUnroll], edge_h[kUnroll], edge_f[kUnroll];
                uint32_t cw[kUnroll], co[kUnroll];
                [[maybe_unused]] uint4 pr[kUnroll];
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    if constexpr (WIDE) {
                        pr[t] = pr_next[t];
                        pr_next[t] = prof_lane[sh_next[t]];
                        sh_next[t] = wide_row(s1, s0 + 2 * kUnroll + t - l, len1);
                    } else {
                        sh[t] = sh_next[t];
                        sh_next[t] = base_shift(s1, s0 + kUnroll + t - l, len1);
                    }
                    // lane 0's left column for row s0 + t + 1: the ring, or the border's H and F = -inf
                    if (w > 0) {
                        const int2 v = ring_in[(s0 + t) & (kRing - 1)];
                        bound_h[t] = v.x;
                        bound_f[t] = v.y;
                    } else if (STRIPED && stripe > 0) {
                        // ... the previous stripe's last column (carry_row, tile_sweep.h)
                        const int2 v = carry_k[carry_row(s0 + t - l, len1)];
                        bound_h[t] = v.x;
                        bound_f[t] = v.y;
                    } else {
                        bound_h[t] = V::border(s0 + t + 1, open_col0, ext_col0);
                        bound_f[t] = kMinusInf;
                    }
                    cw[t] = 0;
                    co[t] = 0;
                }
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    const int left_in = from_left(bound_h[t], key[kCols - 1]);   // lane l-1's key(i, jbase), one step ago
                    const int f_in = from_left(bound_f[t], f_last);              // ... and its F(i, jbase)
                    const int row = s0 + t - l + 1;
                    if (row >= 1 && row <= len1) {
                        int d = diag_in, lft = left_in, f = f_in, rk = V::kRowMin;
                        if constexpr (kEndRule<V>) {
                            // H(row - 1, len2), read BEFORE the row is computed, while key[] still holds the row above: one
                            // register of one lane through a uniform switch, in a branch that only the last wave takes and
                            // only with kFreeEnd1, so the loop has no chain over the cells.  (Read from the FINISHED row, as
                            // the linear body does it, the old row's keys live on beside the new row's and the traceback
                            // kernel spills 32 VGPRs; a select per cell costs every mask 64 v_cndmask_b32 per trip.  DESIGN.md
                            // section 21.)  Row 0 is read at row 1; row len1's cell is the corner, a candidate of its own
                            if (end_sel >= 0) {
                                int end_key;
                                switch (end_sel) {
                                case 0: end_key = key[0]; break;
                                case 1: end_key = key[1]; break;
                                case 2: end_key = key[2]; break;
                                case 3: end_key = key[3]; break;
                                case 4: end_key = key[4]; break;
                                case 5: end_key = key[5]; break;
                                case 6: end_key = key[6]; break;
                                case 7: end_key = key[7]; break;
                                case 8: end_key = key[8]; break;
                                case 9: end_key = key[9]; break;
                                case 10: end_key = key[10]; break;
                                case 11: end_key = key[11]; break;
                                case 12: end_key = key[12]; break;
                                case 13: end_key = key[13]; break;
                                case 14: end_key = key[14]; break;
                                default: end_key = key[15]; break;
                                }
                                if (end_key > best) {
                                    best = end_key;
                                    best_row = row - 1;
                                }
                            }
                        }
#pragma unroll
                        for (int jj = 0; jj < kCols; ++jj) {
                            const int sc = WIDE ? __builtin_amdgcn_sbfe((int)wide_dword(pr[t], jj >> 2), 8 * (jj & 3), 8)
                                                : __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                            const int ev = imax(key[jj] + g_open, e[jj] + g_ext);
                            const int fv = imax(lft + g_open, f + g_ext);
                            int ec = ev, fc = fv;
                            if constexpr (TB) {
                                ec = (ev & ~63) | V::kTagE;
                                fc = (fv & ~63) | V::kTagF;
                            }
                            const int m = V::floor(max3(d + (sc << 6), ec, fc));
                            const int nk = (m & ~63) | (V::kTagH | (kCols - 1 - jj));
                            if constexpr (TB) {
                                cw[t] |= ((uint32_t)(m >> 4) & 3u) << (2 * jj);
                                co[t] |= (((uint32_t)ev >> V::kOpenBitE) & 1u) << jj;
                                co[t] |= (((uint32_t)fv >> V::kOpenBitF) & 1u) << (16 + jj);
                            }
                            d = key[jj];
                            key[jj] = nk;
                            e[jj] = ec;
                            f = fc;
                            lft = nk;
                            if constexpr (!kEndRule<V>) rk = rk > nk ? rk : nk;
                        }
                        f_last = f;
                        if constexpr (!kEndRule<V>) {
                            if (rk > (best | 63)) {
                                best = rk;
                                best_row = row;
                            }
                        }
                    }
                    edge_h[t] = key[kCols - 1];
                    edge_f[t] = f_last;
                    diag_in = left_in;
                }
                if (w < W - 1 && l == 63) {
#pragma unroll
                    for (int t = 0; t < kUnroll; ++t) {
                        const int row = s0 + t - 62;
                        if (row >= 1 && row <= len1) ring_out[(row - 1) & (kRing - 1)] = make_int2(edge_h[t], edge_f[t]);
                    }
                }
                if constexpr (STRIPED) {
                    // the stripe's last column, for the next stripe's wave 0 (vector stores; every stripe but the last is full)
                    if (more_stripes && w == W - 1 && l == 63) {
#pragma unroll
                        for (int t = 0; t < kUnroll; ++t) {
                            const int row = s0 + t - 62;
                            if (row >= 1 && row <= len1) carry_k[row - 1] = make_int2(edge_h[t], edge_f[t]);
                        }
                    }
                }
                if constexpr (TB) {
                    uint4 *o = reinterpret_cast<uint4 *>(cw_out + (size_t)(s0 >> 2) * 256);
                    o[0] = make_uint4(cw[0], co[0], cw[1], co[1]);
                    o[1] = make_uint4(cw[2], co[2], cw[3], co[3]);
                }
            }
        }
        if (W > 1) __syncthreads();
    }

    // best cell: (H desc, row asc, column asc) over the lanes, then over the waves
    if constexpr (kEndRule<V>) {
        // the lane's candidates (tile_sweep.h): key[] holds row len1 now.  Last row, columns past len2 masked out; the
        // corner; the last column's best over rows 0 .. len1 - 1; thread 0's two border cells.  (STRIPED: a wave that skipped
        // the stripe still holds row 0 in key[], and jbase >= len2 masks all of it)
        const int len2_e = opaque<RAGGED || STRIPED>(len2);   // len2, not before the sweep in a ragged or striped kernel (tile_sweep.h)
        int last = V::kRowMin, corner = V::kRowMin;
#pragma unroll
        for (int jj = 0; jj < kCols; ++jj) {
            const int j = jbase + jj + 1;
            if (j <= len2_e && key[jj] > last) last = key[jj];
            if (j == len2_e) corner = key[jj];
        }
        if ((free_ends & kFreeEnd2) && jbase < len2_e)
            r = umax64(r, end_pack(last >> 6, len1, jbase + (kCols - 1 - (last & 15)) + 1, kEndBias));
        if (G == (len2_e - 1) >> 4) {
            r = umax64(r, end_pack(corner >> 6, len1, len2_e, kEndBias));
            if (end_sel >= 0) r = umax64(r, end_pack(best >> 6, best_row, len2_e, kEndBias));
        }
        r = umax64(r, r_border);
    } else {
        const int h = best >> 6;
        const int col = h > 0 ? jbase + (kCols - 1 - (best & 15)) + 1 : 0;
        const unsigned long long cand = ((unsigned long long)(uint32_t)h << 34) | ((unsigned long long)(0x1FFFF - best_row) << 17) |
                                        (unsigned long long)(0x1FFFF - col);
        // the stripe's best cell joins the earlier stripes' (a wave that skipped the stripe folds (0, 0) with H = 0: harmless)
        if constexpr (kFoldInLds) {
            unsigned long long c = cand;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) c = umax64(c, __shfl_xor(c, o, 64));
            if (l == 0) red[w] = umax64(red[w], c);
        } else {
            r = cand;
        }
    }
    if constexpr (STRIPED) {
        if (more_stripes) {
            // between two stripes: this wave's carry stores have reached L2, every wave is past its last ring read, and the
            // next stripe's carry loads miss this CU's L1, which may hold the rows as the previous stripe left them
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
    }
    } while (STRIPED && ++stripe * kStripeCols < len2);
    if constexpr (!kFoldInLds) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long v = __shfl_xor(r, o, 64);
            r = v > r ? v : r;
        }
        if (l == 0) red[w] = r;
    }
    if constexpr (TB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's code stores have reached L2
    __syncthreads();
    r = red[0];
    for (int x = 1; x < W; ++x) r = red[x] > r ? red[x] : r;
    const int score = kEndRule<V> ? (int)(r >> 34) - kEndBias : (int)(r >> 34);
    const int end_i = kEndRule<V> || score > 0 ? 0x1FFFF - (int)((r >> 17) & 0x1FFFF) : 0;
    const int end_j = kEndRule<V> || score > 0 ? 0x1FFFF - (int)(r & 0x1FFFF) : 0;
    if (tid == 0) {
        scores[k] = score;
        ends[V::kEnds * k + 0] = end_i;
        ends[V::kEnds * k + 1] = end_j;
        if constexpr (!TB)                              // what only a walk finds
            for (int x = 2; x < V::kEnds; ++x) ends[V::kEnds * k + x] = -1;
    }
    if constexpr (TB) {
        constexpr uint32_t kCodeH = V::kTagH >> 4, kCodeE = V::kTagE >> 4;
        const unsigned long long *cd = codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)(STRIPED ? waves(len2) : W) * n_trips * 256));
        unsigned long long *mv = moves + (RAGGED ? (size_t)slot.move_base : k * (size_t)move_words);
        int i = end_i, j = end_j, stopped = 0;
        int state = 0;                                  // 0 = H, 1 = E, 2 = F (thread 0's only)
        uint32_t t = 0;
        unsigned long long acc = 0;
        while ((!V::kWalkStops || !stopped) && i > 0 && j > 0) {   // uniform: every thread holds the same (i, j, stopped)
            const int g1 = (j - 1) >> 4;
            const int i_lo = i - kStageRows + 1 > 1 ? i - kStageRows + 1 : 1;
            const int g_lo = g1 - kStageLanes + 1 > 0 ? g1 - kStageLanes + 1 : 0;
            const int rows = i - i_lo + 1, lanes = g1 - g_lo + 1;
            for (int x = tid; x < rows * lanes; x += blockDim.x) {
                const int rr = x / lanes, gg = x - rr * lanes;
                stage[rr * kStageLanes + gg] = __builtin_nontemporal_load(cd + code_index(i_lo + rr, g_lo + gg, n_trips));
            }
            __syncthreads();
            if (tid == 0) {
                int st = 0;
                while (i > 0 && j > 0 && i >= i_lo && ((j - 1) >> 4) >= g_lo) {
                    const unsigned long long wd = stage[(i - i_lo) * kStageLanes + ((j - 1) >> 4) - g_lo];
                    const int cc = (j - 1) & 15;
                    if (state == 0) {
                        const uint32_t hc = (uint32_t)(wd >> (2 * cc)) & 3u;
                        if (V::kWalkStops && hc == kCodeH + 1) {   // the floor won: the cell holds 0, the start cell
                            st = 1;
                            break;
                        }
                        state = hc == kCodeH ? 0 : hc == kCodeE ? 1 : 2;
                    }
                    uint32_t mvc;
                    if (state == 0) {
                        mvc = 3;                        // diagonal
                        --i;
                        --j;
                    } else if (state == 1) {
                        mvc = 2;                        // up, inside E; back to H where E opened
                        state = (wd >> (32 + cc)) & 1u ? 0 : 1;
                        --i;
                    } else {
                        mvc = 1;                        // left, inside F; back to H where F opened
                        state = (wd >> (48 + cc)) & 1u ? 0 : 2;
                        --j;
                    }
                    acc |= (unsigned long long)mvc << (2 * (t & 31));
                    ++t;
                    if ((t & 31) == 0) {
                        mv[(t >> 5) - 1] = acc;
                        acc = 0;
                    }
                }
                walk_at[0] = i;
                walk_at[1] = j;
                if constexpr (V::kWalkStops) walk_at[2] = st;
            }
            __syncthreads();
            i = walk_at[0];
            j = walk_at[1];
            if constexpr (V::kWalkStops) stopped = walk_at[2];
        }
        if (tid == 0) {
            if constexpr (V::kWalkStops) {
                // the walk ended on its start cell: the count is the moves
                if (t & 31) mv[t >> 5] = acc;
                counts[k] = t;
                ends[V::kEnds * k + 2] = i;
                ends[V::kEnds * k + 3] = j;
            } else if constexpr (kEndRule<V>) {
                // the walk reached a border (in state H): it ends there if that border is free, else it goes on to (0, 0) by
                // forced moves (up along column 0, left along row 0); the count is the moves, the start cell where it ended
                const uint32_t m = i > 0 ? 2u : 1u;
                if (!(free_ends & (i > 0 ? kFreeBegin1 : kFreeBegin2))) {
                    for (; i > 0 || j > 0; ++t) {
                        acc |= (unsigned long long)m << (2 * (t & 31));
                        i -= m == 2u;
                        j -= m == 1u;
                        if (((t + 1) & 31) == 0) {
                            mv[t >> 5] = acc;
                            acc = 0;
                        }
                    }
                }
                if (t & 31) mv[t >> 5] = acc;
                counts[k] = t;
                ends[V::kEnds * k + 2] = i;
                ends[V::kEnds * k + 3] = j;
            } else {
                // the walk goes on to (0, 0), forced on the border: up along column 0, left along row 0; the count is the
                // path's cells, moves + 1
                for (; i > 0 || j > 0; ++t) {
                    const uint32_t mvc = i > 0 ? 2u : 1u;
                    acc |= (unsigned long long)mvc << (2 * (t & 31));
                    i -= mvc == 2u;
                    j -= mvc == 1u;
                    if (((t + 1) & 31) == 0) {
                        mv[t >> 5] = acc;
                        acc = 0;
                    }
                }
                if (t & 31) mv[t >> 5] = acc;
                counts[k] = t + 1;
            }
        }
    }
