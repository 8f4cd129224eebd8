// Distances: edlibAlign(TASK_DISTANCE), SHW read off the last column of an NW sweep, and the scores of a pass's last column.
#ifndef RTK_MYERS_DISTANCE_H
#define RTK_MYERS_DISTANCE_H
#include "rtk_myers_pass.h"
#include "rtk_myers_sim.h"

RTK_FN void rtk_myers_column(const uint64_t* fin_pv_, const uint64_t* fin_mv_, int m_, int n_, int32_t* out_, int dlo_ = -RTK_BAND_FULL, int dhi_ = RTK_BAND_FULL, int gran_ = 64);

// End bookkeeping of SHW / HW for a query of qlen characters, from the minimum over the target's columns (colbest, its first and last column, how many hold it):
// edlib pads the query to whole 64-row blocks, so when qlen % 64 != 0 target position -1 is an end location too, with score qlen (edlib.cpp:658-692). It beats the
// columns when qlen < colbest and ties with them when qlen == colbest: it is then the first location and one more than cnt. r.first == -1 says that it counts.
RTK_DEV MyersResult rtk_shw_ends(int colbest, int first, int last, int cnt, int qlen) {
    MyersResult r; int best = colbest; const bool pseudo = (qlen & 63) != 0;
    if (pseudo && qlen < best) best = qlen;
    r.dist = best;
    if (pseudo && qlen == best) { r.first = -1; r.last = (colbest == best) ? last : -1; r.nloc = 1 + ((colbest == best) ? cnt : 0); }
    else { r.first = first; r.last = last; r.nloc = cnt; }
    return r;
}

// edlibAlign(..., TASK_DISTANCE): edit distance (or -1 if above a non-negative k), first and largest end location and
// their number. SHW/HW report target position -1 (score m) when m % 64 != 0, like edlib's padded last block
// (edlib.cpp:658-692). Optionally lists every end location (locs_out, up to cap).
RTK_FN MyersResult rtk_myers_distance(const MyersScratch& sc_, const char* q_, int m_, const char* t_, int n_, int k_, int mode_, bool iupac_,
                                        int32_t* locs_out_ = nullptr, int cap_ = 0) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const char* q = rtk_u(q_); const char* t = rtk_u(t_); const int m = rtk_u(m_), n = rtk_u(n_), k = rtk_u(k_), mode = rtk_u(mode_), cap = rtk_u(cap_);
    const bool iupac = rtk_u(iupac_); int32_t* locs_out = rtk_u(locs_out_);
    MyersResult r; r.dist = -1; r.first = -1; r.last = -1; r.nloc = 0;
    if (m == 0 || n == 0) { // edlib.cpp:161-179
        if (mode == RTK_MODE_NW) { r.dist = m > n ? m : n; r.first = r.last = n - 1; }
        else { r.dist = m; r.first = r.last = -1; }
        r.nloc = 1;
        if (locs_out && cap > 0) locs_out[0] = r.first;
        return r;
    }
    if (mode == RTK_MODE_NW && k >= 0 && k < (n > m ? n - m : m - n)) return r; // edlib.cpp:744-747
    if (static_cast<uint32_t>((m + 63) >> 6) > sc.w_cap || static_cast<uint32_t>(n) > sc.t_cap) { *sc.overflow = 1; return r; }
    if (m <= 4096 && !locs_out) { // one row block: the sweep that keeps the last row's minimum in registers, if the target is plain (the simulator's declines)
        const SweepStat st = (mode == RTK_MODE_NW) ? rtk_myers_fast_any<0, 0>(q, m, t, n, 1, iupac, nullptr) : rtk_myers_fast_any<0, 1>(q, m, t, n, mode == RTK_MODE_HW ? 0 : 1, iupac, nullptr);
        if (st.plain) {
            if (mode == RTK_MODE_NW) { if (k >= 0 && st.final_score > k) return r; r.dist = st.final_score; r.first = r.last = n - 1; r.nloc = 1; return r; }
            const MyersResult e = rtk_shw_ends(st.best, st.first, st.last, st.cnt, m);
            if (k >= 0 && e.dist > k) return r;
            return e;
        }
    }
    if (mode == RTK_MODE_NW && m > 4096 && static_cast<uint32_t>(m) <= sc.r_cap && static_cast<uint64_t>(2 * ((m + 63) >> 6)) <= sc.tb_cap_words) {
        // several row blocks: only the Ukkonen band of k (edlib.cpp:744-775). Unknown distance: a guess instead of edlib's doubling (:199-212) -- a score
        // found inside a band is a real one, so when it exceeds the guess the band of that score holds the optimum and one more pass settles it.
        const int W = (m + 63) >> 6;
        uint64_t* fin = sc.tb; int32_t* col = sc.rowL;
        rtk_tb_written(sc); // the table's memory holds the delta vectors
        int kk = k >= 0 ? k : rtk_band_guess(m, n);
        for (;;) {
            const RtkBand band = rtk_band_nw(m, n, kk);
            const int gran = rtk_myers_pass_banded(sc, rtk_seq(q, m), rtk_seq(t, n), iupac, band.dlo, band.dhi, fin, fin + W);
            rtk_myers_column(fin, fin + W, m, n, col, band.dlo, band.dhi, gran);
            const int d = rtk_ld(col + (m - 1));
            if (d <= kk) { r.dist = d; r.first = r.last = n - 1; r.nloc = 1; if (locs_out && cap > 0) locs_out[0] = n - 1; return r; }
            if (k >= 0) return r; // above k
            kk = d;
        }
    }
    rtk_myers_pass(sc, rtk_seq(q, m), rtk_seq(t, n), mode == RTK_MODE_HW ? 0 : 1, iupac, 0, nullptr, nullptr);
    if (mode == RTK_MODE_NW) {
        const int d = sc.colscore[n - 1];
        if (k >= 0 && d > k) return r;
        r.dist = d; r.first = r.last = n - 1; r.nloc = 1;
        if (locs_out && cap > 0) locs_out[0] = n - 1;
        return r;
    }
    // min over columns, then positions of the minimum (lane-strided, reduced across the wave)
    int best = 0x7fffffff;
    for (int j = rtk_lane(); j < n; j += RTK_WAVE) { const int v = sc.colscore[j]; best = v < best ? v : best; }
    best = rtk_wave_min(best);
    const MyersResult e = rtk_shw_ends(best, 0, 0, 0, m); // the distance, and whether location -1 holds it; the columns that do are listed below
    best = e.dist;
    if (k >= 0 && best > k) return r;
    r.dist = best;
    int cnt = 0, first = 0x7fffffff, last = -2;
    if (e.first == -1) { cnt = 1; first = -1; last = -1; if (locs_out && cap > 0) locs_out[0] = -1; }
    for (int j0 = 0; j0 < n; j0 += RTK_WAVE) {
        const int j = j0 + rtk_lane();
        const bool hit = (j < n) && (sc.colscore[j] == best);
        const uint64_t b = rtk_ballot(hit);
        if (b) {
            const int lo = j0 + rtk_ffs(b) - 1;
            const int hi = j0 + 63 - __builtin_clzll(b);
            if (lo < first) first = lo;
            if (hi > last) last = hi;
            if (locs_out) {
                const int my = cnt + rtk_popc(b & ((1ull << rtk_lane()) - 1ull));
                if (hit && my < cap) locs_out[my] = j;
            }
            cnt += rtk_popc(b);
        }
    }
    rtk_sync();
    r.first = first; r.last = last; r.nloc = cnt;
    return r;
}

// SHW by column: edlibAlign(raw, corr, SHW) with k = -1 -- the MyersResult rtk_myers_distance returns, end locations and the score-|raw| location
// -1 included -- read off the LAST COLUMN of one NW sweep of (corr, raw). Equality is symmetric (rtk_eq_classes), so the SHW matrix of (raw, corr)
// is the transpose of NW(corr, raw) and its score at end j is D[j + 1][|raw|]. Row i of the swept table only depends on rows <= i, so a stored
// sweep (store != 0, table in sc.tb, ncols = |raw|) also holds NW(corr[0, r), raw) for every r <= |corr|: rtk_myers_walk(sc, r, |raw|, |raw|,
// D[r][|raw|], ...) walks it. *at_score (optional) = D[at][|raw|]. The step is the plain NW step, without the last-row tracking of the
// distance call. Returns false, with no result, where the route does not apply: an empty string, |corr| > 4096, a raw byte other than
// A/C/G/T (the sweep's target), the capacities the distance call checks (the caller makes that call: it reports the overflow), and for a
// stored sweep those of the table.
RTK_FN bool rtk_myers_shw_by_column(const MyersScratch& sc_, const char* corr_, int m_, const char* raw_, int n_, bool iupac_, int store_, int at_, MyersResult* out_, int* at_score_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const char* corr = rtk_u(corr_); const char* raw = rtk_u(raw_);
    const int m = rtk_u(m_), n = rtk_u(n_), store = rtk_u(store_), at = rtk_u(at_); const bool iupac = rtk_u(iupac_);
    MyersResult* out = rtk_u(out_); int* at_score = rtk_u(at_score_);
    const long long W = (m + 63) >> 6;
    if (m <= 0 || n <= 0 || m > 4096 || static_cast<uint32_t>((n + 63) >> 6) > sc.w_cap || static_cast<uint32_t>(m) > sc.t_cap) return false;
    if (static_cast<uint32_t>(W) > sc.w_cap || static_cast<uint32_t>(n) > sc.t_cap) return false;
    if (store && static_cast<uint64_t>(4 * W * n) > sc.tb_cap_words) return false;
    if (store) rtk_tb_written(sc);
    const SweepStat st = rtk_myers_sweep_column(sc, corr, m, raw, n, iupac, store, at);
    if (!st.plain) return false;
    if (out) *out = rtk_shw_ends(st.best, st.first, st.last, st.cnt, n); // the query of the SHW call is raw
    if (at_score) *at_score = st.at_score;
    return true;
}

// Scores of the last column of a pass from the vertical deltas it left behind: out[i] = D[i + 1][n] for the rows of the words that are
// inside the band at the last column, RTK_BAND_INF for the others. A word parks its deltas at ITS last column; the row above the band
// then grows by one per column, so the score at the top of word w in the last column is n + the sum of the column totals of the words
// above it, whatever their last columns were (for a pass without a band: the usual prefix sum).
RTK_FN void rtk_myers_column(const uint64_t* fin_pv_, const uint64_t* fin_mv_, int m_, int n_, int32_t* out_, int dlo_, int dhi_, int gran_) {
    const uint64_t* fin_pv = rtk_u(fin_pv_); const uint64_t* fin_mv = rtk_u(fin_mv_); const int m = rtk_u(m_), n = rtk_u(n_); int32_t* out = rtk_u(out_);
    const int dlo = rtk_u(dlo_), dhi = rtk_u(dhi_), gran = rtk_u(gran_);
    const int W = (m + 63) >> 6, Wa = rtk_band_words(m, n, dlo);
    // word prefix: value at the top of word w = n + sum over previous words of (popc(P) - popc(M)) restricted to valid rows
    for (int w0 = 0, base = n; w0 < W; w0 += RTK_WAVE) {
        const int w = w0 + rtk_lane();
        int delta = 0;
        uint64_t pv = 0, mv = 0;
        const bool have = w < Wa; // the word had a column
        if (have) {
            pv = fin_pv[w]; mv = fin_mv[w];
            const int rows = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
            const uint64_t mask = rows == 64 ? ~0ull : ((1ull << rows) - 1ull);
            pv &= mask; mv &= mask;
            delta = rtk_popc(pv) - rtk_popc(mv);
        }
        int total;
        const int excl = rtk_wave_excl_scan(delta, &total);
        if (w < W) {
            const int rows = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
            if (have && rtk_band_chi(w, W, n, dhi, gran) == n - 1) {
                int v = base + excl;
                for (int b = 0; b < rows; ++b) { v += static_cast<int>((pv >> b) & 1ull) - static_cast<int>((mv >> b) & 1ull); out[64 * w + b] = v; }
            } else for (int b = 0; b < rows; ++b) out[64 * w + b] = RTK_BAND_INF;
        }
        base += total;
    }
    rtk_sync();
}
#endif
