// The 1-lane simulator's stand-ins for the device schedules, under the device routines' names and signatures: the matrix column by column.
#ifndef RTK_MYERS_SIM_H
#define RTK_MYERS_SIM_H
#include "rtk_myers_band.h"
#include "rtk_myers_step.h"

#ifdef RTK_SIM

RTK_FN void rtk_myers_pass(const MyersScratch& sc_, MySeq q_, MySeq t_, int top_h_, bool iupac_, int store_, uint64_t* fin_pv_, uint64_t* fin_mv_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    MySeq q, t; q.p = rtk_u(q_.p); q.n = rtk_u(q_.n); q.rev = rtk_u(q_.rev); t.p = rtk_u(t_.p); t.n = rtk_u(t_.n); t.rev = rtk_u(t_.rev);
    const int top_h = rtk_u(top_h_), store = rtk_u(store_); const bool iupac = rtk_u(iupac_); uint64_t* fin_pv = rtk_u(fin_pv_); uint64_t* fin_mv = rtk_u(fin_mv_);
    const int m = q.n, n = t.n, W = (m + 63) >> 6, last_bit = (m - 1) & 63;
    rtk_myers_build_peq(sc, q, W, iupac);
    int score = m;
    // the simulator walks the matrix column by column; per-word state lives in fin arrays or a local buffer
    uint64_t* Pv = fin_pv; uint64_t* Mv = fin_mv;
    uint64_t lpv[64], lmv[64]; // only used when the caller does not want the final vectors and W <= 64
    uint64_t* heapPv = nullptr; uint64_t* heapMv = nullptr;
    if (!Pv) { if (W <= 64) { Pv = lpv; Mv = lmv; } else { heapPv = new uint64_t[W]; heapMv = new uint64_t[W]; Pv = heapPv; Mv = heapMv; } }
    for (int w = 0; w < W; ++w) { Pv[w] = ~0ull; Mv[w] = 0; }
    for (int j = 0; j < n; ++j) {
        const unsigned char tc = rtk_seq_at(t, j);
        int hin = top_h;
        for (int w = 0; w < W; ++w) {
            uint64_t Ph, Mh;
            const uint64_t Eq = rtk_myers_eq_word(sc, q, W, w, tc);
            hin = rtk_myers_step(Pv[w], Mv[w], Eq, hin, (w == W - 1) ? last_bit : 63, Ph, Mh);
            if (store) { rtk_tb_put(sc.tb + 4ull * RTK_TB(j, w, n), Pv[w], Mv[w], Ph, Mh); }
        }
        score += hin;
        sc.colscore[j] = score;
    }
    delete[] heapPv; delete[] heapMv;
    rtk_sync();
}

RTK_FN int rtk_myers_pass_banded(const MyersScratch& sc_, MySeq q_, MySeq t_, bool iupac_, int dlo_, int dhi_, uint64_t* fin_pv_, uint64_t* fin_mv_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    MySeq q, t; q.p = rtk_u(q_.p); q.n = rtk_u(q_.n); q.rev = rtk_u(q_.rev); t.p = rtk_u(t_.p); t.n = rtk_u(t_.n); t.rev = rtk_u(t_.rev);
    const bool iupac = rtk_u(iupac_); uint64_t* fin_pv = rtk_u(fin_pv_); uint64_t* fin_mv = rtk_u(fin_mv_);
    RtkBand band; band.dlo = rtk_u(dlo_); band.dhi = rtk_u(dhi_);
    const int m = q.n, n = t.n, W = (m + 63) >> 6;
    const int gran = rtk_band_gran(m, band.dlo, band.dhi);
    // the simulator walks the band column by column with the same column ranges per word as the device schedules
    const int last_bit = (m - 1) & 63, Wa = rtk_band_words(m, n, band.dlo);
    rtk_myers_build_peq(sc, q, W, iupac);
    for (int w = 0; w < Wa; ++w) { fin_pv[w] = ~0ull; fin_mv[w] = 0; }
    for (int j = 0; j < n; ++j) {
        const unsigned char tc = rtk_seq_at(t, j);
        int hin = 1;
        for (int w = 0; w < Wa; ++w) {
            if (j < rtk_band_clo(w, band.dlo, gran) || j > rtk_band_chi(w, W, n, band.dhi, gran)) continue;
            if (w > 0 && j > rtk_band_chi(w - 1, W, n, band.dhi, gran)) hin = 1; // nothing above any more: the row above the band grows by one per column
            uint64_t Ph, Mh;
            const uint64_t Eq = rtk_myers_eq_word(sc, q, W, w, tc);
            hin = rtk_myers_step(fin_pv[w], fin_mv[w], Eq, hin, (w == W - 1) ? last_bit : 63, Ph, Mh);
        }
    }
    return gran;
}

// The device's one-row-block sweeps (rtk_myers_sweep.h) decline a target with a byte other than A/C/G/T; the simulator's declines every target, so that its
// callers take the route they take on the device for such a target: the generic pass.
template <int STORE, int TRACK>
inline SweepStat rtk_myers_fast_any(const char*, int m, const char*, int, int, bool, uint64_t*, int = 0) {
    SweepStat st; st.final_score = m; st.best = 0x7fffffff; st.first = -1; st.last = -1; st.cnt = 0; st.plain = false; st.at_score = 0;
    return st;
}
// The level-by-level Hirschberg driver (rtk_myers_lvl.h) is a device schedule: every problem is left to the explicit stack of rtk_myers_alignment.
inline bool rtk_myers_alignment_lvl(const MyersScratch&, const char*, int, const char*, int, int, bool, uint32_t*, int*) { return false; }

inline bool rtk_sim_plain(const char* t, int n) { // the device sweeps' own test of their target
    for (int j = 0; j < n; ++j) { const char ch = t[j]; if (!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T')) return false; }
    return true;
}

// The two sweeps that DO have a simulator route, so that both builds make, and count, the same alignments: the same pairs (a target of A/C/G/T only), the same
// stored table, through the generic pass.
RTK_DEV SweepStat rtk_myers_sweep_column(const MyersScratch& sc, const char* corr, int m, const char* raw, int n, bool iupac, int store, int at) {
    SweepStat st; st.final_score = m; st.best = 0x7fffffff; st.first = -1; st.last = -1; st.cnt = 0; st.plain = rtk_sim_plain(raw, n); st.at_score = n;
    if (!st.plain) return st;
    const long long W = (m + 63) >> 6;
    uint64_t* fin = new uint64_t[2 * W];
    rtk_myers_pass(sc, rtk_seq(corr, m), rtk_seq(raw, n), 1, iupac, store ? 1 : 0, fin, fin + W);
    if (store == 2) { // what the device sweep leaves behind: the entries of the last column at the start of the table, and no other entry that can be read
        uint64_t* const tb = rtk_ld(&sc.tb); uint64_t* const lastc = new uint64_t[4 * W];
        for (long long w = 0; w < W; ++w) memcpy(lastc + 4 * w, tb + 4ull * RTK_TB(n - 1, w, n), 32);
        memset(tb, 0xA5, 32ull * static_cast<uint64_t>(W) * static_cast<uint64_t>(n));
        memcpy(tb, lastc, 32ull * static_cast<uint64_t>(W));
        delete[] lastc;
    }
    for (int i = 0, v = n; i < m; ++i) { // the last column, from the vertical deltas the pass left (rtk_last_column_stat on the device)
        v += static_cast<int>((fin[i >> 6] >> (i & 63)) & 1ull) - static_cast<int>((fin[W + (i >> 6)] >> (i & 63)) & 1ull);
        if (v < st.best) { st.best = v; st.first = st.last = i; st.cnt = 1; } else if (v == st.best) { st.last = i; ++st.cnt; }
        if (i + 1 == at) st.at_score = v;
    }
    delete[] fin;
    return st;
}
RTK_DEV SweepStat rtk_myers_sweep_saved(const MyersScratch& sc, const char* q, int m, const char* t, int n, bool iupac, uint32_t* gen) {
    SweepStat st; st.final_score = m; st.best = 0x7fffffff; st.first = -1; st.last = -1; st.cnt = 0; st.plain = rtk_sim_plain(t, n); st.at_score = 0;
    if (!st.plain) return st;
    *gen = rtk_tb_written(sc);
    rtk_myers_pass(sc, rtk_seq(q, m), rtk_seq(t, n), 1, iupac, 1, nullptr, nullptr);
    st.final_score = sc.colscore[n - 1]; // the last row, read off colscore
    for (int j = 0; j < n; ++j) { const int v = sc.colscore[j]; if (v < st.best) { st.best = v; st.first = st.last = j; st.cnt = 1; } else if (v == st.best) { st.last = j; ++st.cnt; } }
    return st;
}

// The walk (rtk_myers_walk.h), one cell at a time: each move read from the table entries around its cell.
RTK_FN void rtk_myers_walk(const MyersScratch& sc_, int m_, int n_, int ncols_, int cur_, uint32_t* n_moves_) {
    const MyersScratch& sc = *rtk_u(&sc_); uint32_t* n_moves = rtk_u(n_moves_);
    const int ncols = rtk_u(ncols_);
    int i = rtk_u(m_), j = rtk_u(n_), cur = rtk_u(cur_);
    uint32_t nt = 0; // moves are produced backwards into moves_tmp, from its end
    uint8_t* tmp = rtk_ld(&sc.moves_tmp);
    const uint32_t cap = rtk_ld(&sc.mv_cap);
    uint64_t* const tbp = rtk_ld(&sc.tb);
    while (i > 0 && j > 0) {
        const int r = i - 1, c = j - 1, w = r >> 6, b = r & 63;
        uint64_t a0, a1, a2, a3; rtk_tb_get(tbp + 4ull * RTK_TB(c, w, ncols), a0, a1, a2, a3);
        uint64_t l0 = 0, l1 = 0;
        if (c > 0) { uint64_t l2, l3; rtk_tb_get(tbp + 4ull * RTK_TB(c - 1, w, ncols), l0, l1, l2, l3); }
        const uint8_t mv = rtk_walk_cell(a0, a1, a2, a3, l0, l1, b, c, i, j, cur);
        ++nt; tmp[cap - nt] = mv;
    }
    // whatever is left is a run of inserts (query only) or deletes (target only)
    if (i > 0) { rtk_wfill(tmp + (cap - nt - static_cast<uint32_t>(i)), 1, static_cast<uint64_t>(i)); nt += static_cast<uint32_t>(i); i = 0; }
    if (j > 0) { rtk_wfill(tmp + (cap - nt - static_cast<uint32_t>(j)), 2, static_cast<uint64_t>(j)); nt += static_cast<uint32_t>(j); j = 0; }
    rtk_wcopy(rtk_ld(&sc.moves) + *n_moves, tmp + (cap - nt), nt);
    *n_moves += nt;
    { MyersScratch& msc = const_cast<MyersScratch&>(sc); msc.walk_moves += nt; msc.walk_calls += 1; } // the walk's profile: no cycles, reloads or fall-backs to count here
}
#endif
#endif
