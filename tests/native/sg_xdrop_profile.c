/*
 * sg_xdrop_profile.c -- TEST INFRASTRUCTURE ONLY.
 *
 * What the X-drop sweep of oracle/sg_oracle.c goes through on one pair of 16384-mers, window by window: the numbers that
 * tests/test_sg_edges_cpu.py needs to show that the structured batch of tests/sg_edges.py reaches the threshold, the calm
 * predicate's margin and the walk's seams, and that tests/test_sg_edges_gpu.py compares the kernels' own count of calm
 * windows with.  The recurrence is the one of sg_oracle_xdrop / sg_oracle_calm_windows (included below, so that the helpers
 * are shared and a stale liboracle.so cannot lack a symbol); the tests assert that the counts agree with
 * sg_oracle_calm_windows.
 *
 * Per window of SG_WINDOW rounds (rounds 1 + 8 w .. 8 + 8 w), taken at the window's START, before the band's step:
 *   margin[w]        low - (best - 70), low = the lowest of the 32 band cells; -1 when a cell of the band is dropped
 *   score_at[w]      best - 70, the best score so far (the kernels' threshold is max(best - 70, 1): one higher while it is 0)
 *   dropped[w]       cells the rule of source.cpp:1938-1941 sets to 0 inside the window, counted as
 *                    sg_oracle_calm_windows counts them (a cell that is 0 already counts too)
 *   dropped_live[w]  of those, the cells that held a live value
 *   reach[w]         1 when a pad or a byte that is no base is in reach of the window: a row in [pos_y, pos_y + 39] or a
 *                    column in [pos_x - 62, pos_x - 23] outside 1 .. 16384 or with a byte >= 4 (the band's 32 rows and
 *                    columns and the 8 characters each sequence can give in 8 rounds: generous, it feeds a lower bound)
 * Per round r <= rounds: top_y[r] = the row of band cell 31, so that a path step (y, x) sits in band cell
 * 31 - (y - top_y[y + x]).
 * out[0] windows, out[1] rounds run, out[2] live cells that hold exactly best - 70 after the rule while best - 70 >= 1,
 * out[3] best round, out[4] score, out[5] touched_oob (as sg_oracle_xdrop reports it), out[6] 1 when the sweep ended by the
 * rule (a whole round dropped), out[7] the lowest margin of any window.
 */
#include "../../oracle/sg_oracle.c"

#define SG_WINDOW 8
#define SG_WINDOWS ((SG_MAX_ROUND - 1) / SG_WINDOW)

static int sg_no_base1(const uint8_t *seq1, long y) { return sg_base1(seq1, y) >= 4; }
static int sg_no_base2(const uint8_t *seq2, long x) { return sg_base2(seq2, x) >= 4; }

int sg_xdrop_profile(const uint8_t *seq1, const uint8_t *seq2, int32_t *margin, int32_t *score_at, int32_t *dropped,
                     int32_t *dropped_live, uint8_t *reach, int32_t *top_y, long out[8])
{
    int cur[SG_BAND], hor[SG_BAND], ver[SG_BAND], dia[SG_BAND];
    long pos_y = 0, pos_x = 31, windows = 0, at_threshold = 0, lowest = 1 << 20;
    int best = SG_X, best_round = 0, round, oob = 0, by_rule = 0, last = 0;
    memset(cur, 0, sizeof cur); memset(hor, 0, sizeof hor); memset(ver, 0, sizeof ver); memset(dia, 0, sizeof dia);
    cur[31] = SG_X;
    top_y[0] = 0;
    for (round = 1; round < SG_MAX_ROUND; ++round) {
        if ((round - 1) % SG_WINDOW == 0) {
            const long w = windows++;
            int low = cur[0];
            for (int k = 1; k < SG_BAND; ++k) if (cur[k] < low) low = cur[k];
            margin[w] = low != 0 ? low - (best - SG_X) : -1;
            score_at[w] = best - SG_X;
            if (margin[w] < lowest) lowest = margin[w];
            dropped[w] = dropped_live[w] = 0;
            reach[w] = 0;
            for (long y = pos_y; y <= pos_y + 39; ++y) if (sg_no_base1(seq1, y)) reach[w] = 1;
            for (long x = pos_x - 62; x <= pos_x - 23; ++x) if (sg_no_base2(seq2, x)) reach[w] = 1;
        }
        if (cur[0] < cur[31]) {
            for (int k = 0; k < SG_BAND; ++k) dia[k] = ver[k];
            for (int k = 0; k < SG_BAND; ++k) hor[k] = cur[k];
            for (int k = 0; k < SG_BAND - 1; ++k) ver[k] = cur[k + 1];
            ver[31] = 0;
            if (++pos_x > 32 + SG_LEN + 31) break;
        } else {
            for (int k = 0; k < SG_BAND; ++k) dia[k] = hor[k];
            for (int k = 0; k < SG_BAND; ++k) ver[k] = cur[k];
            for (int k = SG_BAND - 1; k > 0; --k) hor[k] = cur[k - 1];
            hor[0] = 0;
            if (++pos_y > 1 + SG_LEN) break;
        }
        if (pos_y + 31 >= 1 + SG_LEN + 31 || pos_x >= 32 + SG_LEN + 31) oob = 1;
        int round_best = 0;
        for (int k = 0; k < SG_BAND; ++k) {
            const long y = pos_y + 31 - k, x = pos_x - 62 + k;
            const int c1 = sg_base1(seq1, y), c2 = sg_base2(seq2, x);
            const int s = (c1 < 4 && c2 < 4 && c1 == c2) ? 1 : -1;
            int v = 0;
            if (dia[k] != 0 && dia[k] + s > v) v = dia[k] + s;
            if (hor[k] != 0 && hor[k] - 1 > v) v = hor[k] - 1;
            if (ver[k] != 0 && ver[k] - 1 > v) v = ver[k] - 1;
            cur[k] = v;
            if (v > round_best) round_best = v;
        }
        if (round_best > best) { best = round_best; best_round = round; }
        for (int k = 0; k < SG_BAND; ++k) {
            if (cur[k] < best - SG_X) {
                ++dropped[windows - 1];
                if (cur[k] != 0) ++dropped_live[windows - 1];
                cur[k] = 0;
            } else if (cur[k] == best - SG_X && best - SG_X >= 1) {
                ++at_threshold;
            }
        }
        top_y[round] = (int32_t)pos_y;
        last = round;
        if (round_best == 0) { by_rule = 1; break; }
    }
    out[0] = windows; out[1] = last; out[2] = at_threshold; out[3] = best_round; out[4] = best - SG_X; out[5] = oob;
    out[6] = by_rule; out[7] = lowest;
    return 0;
}

int sg_xdrop_profile_windows(void) { return SG_WINDOWS; }
int sg_xdrop_profile_rounds(void) { return SG_MAX_ROUND; }
