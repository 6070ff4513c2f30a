// tile_sweep_body.inc -- the sweep and the walk of a linear-gap tile aligner: the body of its kernel (tile_sweep.h tells
// the mapping and what a variant V supplies).  Included INSIDE the kernel, after `using V = <variant>;` and
// `const V::Gaps gaps{<gap argument>};`, where the kernel's parameters are named seq1s, seq2s, len1, len2, cols, scores,
// ends, codes, moves, counts, move_words, n_trips and its template parameter TB.  A kernel with a ragged form also names
// RAGGED and slot, and then len1, len2 and n_trips are the slot's (tile_sweep.h).  A kernel whose variant has the end rule
// (kEndRule<V>, tile_sweep.h) also names free_ends.  A kernel that sweeps column stripes shadows STRIPED and kEndBias and names
// `carry` (tile_sweep.h; the stripe loop below says what a stripe adds).  Text and not a function on purpose: tile_sweep.h says why.
    __shared__ int ring[(kMaxWaves - 1) * kRing];
    __shared__ unsigned long long red[kMaxWaves];
    __shared__ int walk_at[V::kWalkStops ? 3 : 2];
    __shared__ uint32_t stage[TB ? kStageRows * V::kStageLanes : 1];

    const int W = blockDim.x >> 6;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
    const size_t k = RAGGED ? (size_t)slot.k : (size_t)blockIdx.x;
    const uint8_t *s1 = seq1s + (RAGGED ? (size_t)slot.s1_off : k * (size_t)len1);
    const uint8_t *s2 = seq2s + (RAGGED ? (size_t)slot.s2_off : k * (size_t)len2);
    if constexpr (RAGGED) {
        // a slot with a zero length: the whole workgroup (one wavefront) leaves here, before any barrier and any sequence load
        if (len1 == 0 || len2 == 0) {
            if constexpr (kEndRule<V>) {
                // the end rule's closed form of one border (tile_sweep.h); a linear gap run of L cells costs L gap
                end_rule_zero_length<TB>(len1, len2, free_ends, (len1 + len2) * gaps.gap, k, scores, ends,
                                         TB ? moves + (size_t)slot.move_base : nullptr, counts);
            } else if (V::kWalkStops ? tid == 0 : first_lane()) {   // (first_lane: tile_sweep.h says why)
                scores[k] = 0;
                ends[V::kEnds * k + 0] = 0;
                ends[V::kEnds * k + 1] = 0;
                for (int x = 2; x < V::kEnds; ++x) ends[V::kEnds * k + x] = TB ? 0 : -1;
                // the count the variant's walk would write from (0, 0): its moves (none), or for a walk that no code stops the
                // path's cells, moves + 1 (the one position (0, 0))
                if constexpr (TB) counts[k] = V::kWalkStops ? 0u : 1u;
            }
            return;
        }
    }
    // STRIPED: the workgroup sweeps the stripes of kStripeCols columns one after another over all of seq1.
    // A stripe re-initialises everything from here to the sweep with the lane's GLOBAL index G; wave 0 takes its left column
    // from `carry`, which lane 63 of the previous stripe's last wave wrote (row i at carry[i - 1]: that lane's stored key, what
    // the ring would have carried), and each stripe's candidates are folded into r after it with a 64-bit maximum: the end
    // rule's last-row and last-column cells (end_pack orders them, so a tie between stripes goes to the earlier column), or a
    // local variant's best cell of the stripe (best and best_row start anew in every stripe, the column comes from the lane's
    // GLOBAL jbase; the pack orders H descending, row ascending, column ascending, which is "first in row-major order" over
    // all stripes -- not "the earlier stripe": a later stripe's cell in a lower row beats an equal cell of stripe 0).  ONE carry buffer, in place: row i is read by wave 0 in chunk
    // (i - 1) / 32 of a stripe and overwritten by wave 15 in chunk 45 + (i + 62) / 32 of the SAME stripe, 45 barriers after
    // its value was consumed, and read again only behind the stripe's closing drain, barrier and L1 invalidate.
    // BARRIER INVARIANT: every wave of the workgroup executes total_chunks + 1 barriers in every stripe but the last and
    // total_chunks in the last; total_chunks is made of len1 and blockDim alone, never of w, the stripe or its valid width.  A
    // wave with no column in the last stripe (my_chunks = 0 below) skips the chunk's work, not its barrier.
    [[maybe_unused]] int *const carry_k = STRIPED ? carry + k * (size_t)len1 : nullptr;
    unsigned long long r = 0;                           // best cell so far: (H desc, row asc, column asc)
    // A striped kernel without the end rule (a local variant) keeps its best cell so far per wave in red[w], not in r: two VGPRs
    // that it has not got across the sweep.  Only lane 0 of wave w touches red[w] before the last barrier.
    constexpr bool kFoldInLds = STRIPED && !kEndRule<V>;
    if constexpr (kFoldInLds) {
        if (l == 0) red[w] = 0;
    }
    // the matrix columns, which every stripe's profile needs: a striped kernel keeps them in VGPRs across the sweep (it has
    // some to spare and no SGPR: as scalars they were spilled)
    SmCols pc = cols;
    if constexpr (STRIPED && kEndRule<V>)
        for (int b = 0; b < 4; ++b) pc.c[b] = (uint32_t)opaque_lane<true>((int)pc.c[b]);
    int stripe = 0;
    do {
    // (a striped kernel's per-stripe tid, w and l: opaque_lane, tile_sweep.h; they shadow the workgroup's, which they equal)
    const int tid = opaque_lane<STRIPED>((int)threadIdx.x), w = tid >> 6, l = tid & 63;
    const int G = STRIPED ? stripe * (64 * kMaxWaves) + tid : tid;
    const int gw = STRIPED ? G >> 6 : w;                // the wave of G in the code layout
    // whether another stripe follows (nothing but len2 and `stripe` is kept across the sweep: the kernels have no SGPRs to spare)
    const bool more_stripes = STRIPED && (stripe + 1) * kStripeCols < len2;
    const int code_waves = STRIPED ? waves(len2) : W;   // the wave count of the code layout: all stripes' waves
    const int jbase = kCols * G;                        // the lane's columns are jbase + 1 .. jbase + 16

    uint32_t prof[kCols];
    int key[kCols];                                     // H's stored keys of the row the lane computed last
    // (a striped local kernel's row 0 is sixteen constants, which the compiler would set up once before the stripe loop and keep --
    // spilled -- across every sweep: made of a 0 it cannot see through, they are set up anew in every stripe)
    [[maybe_unused]] const int row0_zero = opaque_lane<STRIPED && !kEndRule<V>>(0);
#pragma unroll
    for (int jj = 0; jj < kCols; ++jj) {
        const int j = jbase + jj + 1;
        const uint32_t b = s2[j <= len2 ? j - 1 : 0] & 3u;
        prof[jj] = j > len2 ? 0x80808080u : b == 0 ? pc.c[0] : b == 1 ? pc.c[1] : b == 2 ? pc.c[2] : pc.c[3];
        key[jj] = V::row0(jj, -j, gaps);
        if constexpr (STRIPED && !kEndRule<V>) key[jj] |= row0_zero;
    }
    V lane(gaps);
    int diag_in = lane.border(-jbase);                   // key(0, jbase)
    int best = kEndRule<V> ? V::kRowMin : V::kZeroKey, best_row = 0;   // H = 0 at (0, 0); end rule: no last-column cell yet
    // (a striped semi-global kernel, whose walk no code stops: with a literal 0 the compiler packs the candidate of a lane that
    // took no row, (0x1FFFF - 0) << 17, once before the stripe loop and keeps the 64-bit constant -- spilled -- across every sweep;
    // the row starts from the stripe's opaque 0 instead)
    if constexpr (STRIPED && !kEndRule<V> && !V::kWalkStops) best_row = row0_zero;
    // end rule: the lane that owns column len2 keeps the best cell of that column, if seq1's end is free
    const int end_jj = (len2 - 1) & (kCols - 1);
    const bool end_col_wave = kEndRule<V> && (free_ends & kFreeEnd1) && (STRIPED ? gw == (len2 - 1) >> 10 : w == W - 1);
    const bool end_col_lane = end_col_wave && G == (len2 - 1) >> 4;

    const int local_chunks = (len1 + 63 + kChunk - 1) / kChunk;
    // a striped kernel's wave with no column in the (last) stripe: no chunk of work, every barrier
    const int my_chunks = STRIPED && jbase - (l << 4) >= len2 ? 0 : local_chunks;
    const int total_chunks = local_chunks + kDelay * (W - 1);
    const int *ring_in = ring + (w > 0 ? w - 1 : 0) * kRing;   // read by waves 1.. (wave 0's left column is the border)
    int *ring_out = ring + (w < W - 1 ? w : 0) * kRing;        // written by waves ..W-2
    uint32_t *cw_out = TB ? codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)code_waves * n_trips * 256)) +
                                ((size_t)gw * n_trips * 64 + l) * 4
                          : nullptr;

    int sh_next[kUnroll];
#pragma unroll
    for (int t = 0; t < kUnroll; ++t) sh_next[t] = base_shift(s1, t - l, len1);

    for (int c = 0; c < total_chunks; ++c) {
        const int lc = c - kDelay * w;
        if (lc >= 0 && lc < my_chunks) {
            for (int q = 0; q < kChunk / kUnroll; ++q) {
                const int s0 = lc * kChunk + q * kUnroll;
                int sh[kUnroll];
                int bound[kUnroll], edge[kUnroll];
                uint32_t cw[kUnroll];
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    sh[t] = sh_next[t];
                    sh_next[t] = base_shift(s1, s0 + kUnroll + t - l, len1);
                    // lane 0's left column for row s0 + t + 1
                    if (STRIPED && stripe > 0)          // ... the previous stripe's last column (carry_row, tile_sweep.h)
                        bound[t] = w > 0 ? ring_in[(s0 + t) & (kRing - 1)] : carry_k[carry_row(s0 + t - l, len1)];
                    else
                        bound[t] = w > 0 ? ring_in[(s0 + t) & (kRing - 1)] : lane.left_border(-(s0 + t + 1));
                    cw[t] = 0;
                }
#pragma unroll
                for (int t = 0; t < kUnroll; ++t) {
                    const int left_in = from_left(bound[t], key[kCols - 1]);   // lane l - 1's key(i, jbase), one step ago
                    const int row = s0 + t - l + 1;
                    if (row >= 1 && row <= len1) {
                        int d = diag_in, lft = left_in, rk = V::kRowMin;
#pragma unroll
                        for (int jj = 0; jj < kCols; ++jj) {
                            const int sc = __builtin_amdgcn_sbfe((int)prof[jj], sh[t], 8);
                            uint32_t code;
                            const int nk = lane.template cell<TB>(jj, sc, d, lft, key[jj], code);
                            if constexpr (TB) cw[t] |= code;
                            if constexpr (!kEndRule<V>) rk = rk > nk ? rk : nk;
                        }
                        if constexpr (kEndRule<V>) {
                            // H(row, len2), read from the finished row: one register of one lane, no chain over the cells
                            // (a uniform switch: an index into key[] would become sixteen selects, more than the chain it replaces)
                            if (end_col_wave) {
                                int end_key;
                                switch (end_jj) {
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
                                if (end_col_lane && end_key > best) {
                                    best = end_key;
                                    best_row = row;
                                }
                            }
                        } else if (rk > (best | 63)) {
                            best = rk;
                            best_row = row;
                        }
                    }
                    edge[t] = key[kCols - 1];
                    diag_in = left_in;
                }
                if (w < W - 1 && l == 63) {
#pragma unroll
                    for (int t = 0; t < kUnroll; ++t) {
                        const int row = s0 + t - 62;
                        if (row >= 1 && row <= len1) ring_out[(row - 1) & (kRing - 1)] = edge[t];
                    }
                }
                if constexpr (STRIPED) {
                    // the stripe's last column, for the next stripe's wave 0 (vector stores; every stripe but the last is full)
                    if (more_stripes && w == W - 1 && l == 63) {
#pragma unroll
                        for (int t = 0; t < kUnroll; ++t) {
                            const int row = s0 + t - 62;
                            if (row >= 1 && row <= len1) carry_k[row - 1] = edge[t];
                        }
                    }
                }
                if constexpr (TB) {
                    *reinterpret_cast<uint4 *>(cw_out + (size_t)(s0 >> 2) * 256) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
                }
            }
        }
        if (W > 1) __syncthreads();
    }

    // best cell: (H desc, row asc, column asc) over the lanes, then over the waves
    if constexpr (kEndRule<V>) {
        // the lane's candidates (tile_sweep.h): key[] holds row len1 now.  Last row, columns past len2 masked out; the
        // corner; the last column's best; thread 0 adds the two border cells, which are closed forms.  (STRIPED: a wave that
        // skipped the stripe still holds row 0 in key[], and jbase >= len2 masks all of it)
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
            if (end_col_lane) r = umax64(r, end_pack(best >> 6, best_row, len2_e, kEndBias));
        }
        if (tid == 0) {
            if (free_ends & kFreeEnd1) r = umax64(r, end_pack(lane.border(-len2_e) >> 6, 0, len2_e, kEndBias));
            if (free_ends & kFreeEnd2) r = umax64(r, end_pack(lane.left_border(-len1) >> 6, len1, 0, kEndBias));
        }
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
        const uint32_t *cd = codes + (RAGGED ? (size_t)slot.code_base : k * ((size_t)(STRIPED ? waves(len2) : W) * n_trips * 256));
        unsigned long long *mv = moves + (RAGGED ? (size_t)slot.move_base : k * (size_t)move_words);
        int i = end_i, j = end_j, stopped = 0;
        uint32_t t = 0;
        unsigned long long acc = 0;
        while ((!V::kWalkStops || !stopped) && i > 0 && j > 0) {            // uniform: every thread holds the same (i, j, stopped)
            const int g1 = (j - 1) >> 4;
            const int i_lo = i - kStageRows + 1 > 1 ? i - kStageRows + 1 : 1;
            const int g_lo = g1 - V::kStageLanes + 1 > 0 ? g1 - V::kStageLanes + 1 : 0;
            const int rows = i - i_lo + 1, lanes = g1 - g_lo + 1;
            for (int e = tid; e < rows * lanes; e += blockDim.x) {
                const int rr = e / lanes, gg = e - rr * lanes;
                stage[rr * V::kStageLanes + gg] = __builtin_nontemporal_load(cd + code_index(i_lo + rr, g_lo + gg, n_trips));
            }
            __syncthreads();
            if (tid == 0) {
                int st = 0;
                while (i > 0 && j > 0 && i >= i_lo && ((j - 1) >> 4) >= g_lo) {
                    const uint32_t wd = stage[(i - i_lo) * V::kStageLanes + ((j - 1) >> 4) - g_lo];
                    const uint32_t m = V::step(wd, (j - 1) & 15);
                    if (V::kWalkStops && m == 0) {
                        st = 1;
                        break;
                    }
                    acc |= (unsigned long long)m << (2 * (t & 31));   // 32 moves to a word
                    i -= m != 1u;
                    j -= m != 2u;
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
                // the walk reached a border: it ends there if that border is free, else it goes on to (0, 0) by forced
                // moves (up along column 0, left along row 0); the count is the moves, the start cell where it ended
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
                // the walk goes on to (0, 0), forced on the border: up along column 0, left along row 0 (the reference's
                // source.cpp:1821-1826); the count is the path's cells, moves + 1
                for (; i > 0 || j > 0; ++t) {
                    const uint32_t m = i > 0 ? 2u : 1u;
                    acc |= (unsigned long long)m << (2 * (t & 31));
                    i -= m == 2u;
                    j -= m == 1u;
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
