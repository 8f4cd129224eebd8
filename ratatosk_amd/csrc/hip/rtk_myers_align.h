// Alignments: obtainAlignment with the Hirschberg driver on an explicit stack, edlibAlign(TASK_PATH), and the saved-sweep pair.
#ifndef RTK_MYERS_ALIGN_H
#define RTK_MYERS_ALIGN_H
#include "rtk_myers_distance.h"
#include "rtk_myers_walk.h"
#include "rtk_myers_lvl.h"

// obtainAlignment (edlib.cpp:1164-1216) with the Hirschberg split of edlib.cpp:1234-1399 restated canonically:
// target halved at n/2; the FIRST query row (ascending) whose left + right scores add up to the optimum, then the
// row -1 boundary, then the last row. Iterative (explicit stack), emits moves in order into sc.moves.
// best < 0: the distance is not known yet. A problem that is split learns it from the split itself (the optimum is the smallest sum of a
// left and a right score), one that fits the in-memory traceback does not need it; *best_out (optional) receives it either way
// (-1 when the traceback branch was taken without it). Saves the separate distance pass of a Hirschberg-sized problem.
RTK_FN void rtk_myers_alignment(const MyersScratch& sc_, const char* q_, int m_, const char* t_, int n_, int best_, bool iupac_, uint32_t* n_moves_, int* best_out_ = nullptr) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const char* q = rtk_u(q_); const char* t = rtk_u(t_); const int m = rtk_u(m_), n = rtk_u(n_), best = rtk_u(best_);
    const bool iupac = rtk_u(iupac_); uint32_t* n_moves = rtk_u(n_moves_); int* best_out = rtk_u(best_out_);
    if (best_out) *best_out = best;
    *n_moves = 0;
    rtk_tb_written(sc);
    if (static_cast<uint32_t>(m + n) > sc.mv_cap || static_cast<uint32_t>((m + 63) >> 6) > sc.w_cap || static_cast<uint32_t>(n) > sc.t_cap || static_cast<uint32_t>(m) > sc.r_cap) { *sc.overflow = 1; return; }
    if (rtk_myers_alignment_lvl(sc, q, m, t, n, best, iupac, n_moves, best_out)) return; // level by level, the half passes of a level side by side in the lanes (rtk_myers_lvl.h; never on the simulator)
    int32_t* st = sc.hstack;
    int sp = 0;
    MyersScratch& prof = const_cast<MyersScratch&>(sc); const unsigned long long t_all0 = rtk_clock();
    st[0] = 0; st[1] = m; st[2] = 0; st[3] = n; st[4] = best; sp = 1;
    uint64_t* fin = sc.tb; // Hirschberg passes do not store the table, so its memory holds the final delta vectors (2 x 2 x W words)
    while (sp > 0) {
        --sp;
        const int q0 = st[5 * sp], qm = st[5 * sp + 1], t0 = st[5 * sp + 2], tn = st[5 * sp + 3], bs_in = st[5 * sp + 4];
        if (qm == 0 || tn == 0) { // edlib.cpp:1171-1178
            rtk_wfill(sc.moves + *n_moves, qm == 0 ? 2 : 1, static_cast<uint64_t>(qm + tn));
            *n_moves += static_cast<uint32_t>(qm + tn);
            continue;
        }
        if (bs_in >= 0 && sc.need_bm && rtk_need_none(sc.need_bm, t0, t0 + tn)) { // (MyersScratch::need_bm: nobody looks at the moves of this stretch)
            rtk_wfill(sc.moves + *n_moves, 2, static_cast<uint64_t>(tn)); rtk_wfill(sc.moves + *n_moves + tn, 1, static_cast<uint64_t>(qm));
            *n_moves += static_cast<uint32_t>(qm + tn);
            continue;
        }
        const long long W = (qm + 63) >> 6;
        if (rtk_tb_in_memory(qm, tn)) {
            if (static_cast<uint64_t>(4 * W * tn) > sc.tb_cap_words) { *sc.overflow = 1; return; }
            { const unsigned long long t0_ = rtk_clock(); rtk_myers_traceback(sc, rtk_seq(q + q0, qm), rtk_seq(t + t0, tn), iupac, n_moves); prof.hb_leaf += rtk_clock() - t0_; }
            continue;
        }
        const int lh = tn / 2, rh = tn - lh;
        if (lh == 0 || static_cast<uint64_t>(4 * W) > sc.tb_cap_words || sp + 2 > 60) { *sc.overflow = 1; return; }
        // The two half passes only sweep the Ukkonen band of the sub-problem's distance (the right one is the same band seen from the other
        // corner: the band is symmetric under d -> (tn - qm) - d). The distance of the whole problem may be unknown (bs_in < 0): a guess,
        // and a second round with the score the first one found when that score is above the guess.
        int kk = bs_in >= 0 ? bs_in : rtk_band_guess(qm, tn);
        int bs_known = bs_in;
        for (;;) {
            const RtkBand band = rtk_band_nw(qm, tn, kk);
            const int gran = rtk_band_gran(qm, band.dlo, band.dhi);
            bool both = false;
            const unsigned long long t_p0 = rtk_clock();
#ifdef RTK_MULTIWAVE
            { const MySeq qa = rtk_seq(q + q0, qm), ta = rtk_seq(t + t0, lh), qb = rtk_seq(q + q0, qm, 1), tb_ = rtk_seq(t + t0 + lh, rh, 1); // the two half passes side by side on the waves of the workgroup
              both = static_cast<uint32_t>(lh + rh) <= sc.t_cap && rtk_myers_pass_coop(sc, qa, ta, 1, iupac, band, fin, fin + W, &qb, &tb_, fin + 2 * W, fin + 3 * W);
              if (both) rtk_sync(); }
#endif
            if (!both) rtk_myers_pass_banded(sc, rtk_seq(q + q0, qm), rtk_seq(t + t0, lh), iupac, band.dlo, band.dhi, fin, fin + W);
            if (!both) rtk_myers_pass_banded(sc, rtk_seq(q + q0, qm, 1), rtk_seq(t + t0 + lh, rh, 1), iupac, band.dlo, band.dhi, fin + 2 * W, fin + 3 * W);
            const unsigned long long t_p1 = rtk_clock(); prof.hb_pass += t_p1 - t_p0;
            rtk_myers_column(fin, fin + W, qm, lh, sc.rowL, band.dlo, band.dhi, gran);
            rtk_myers_column(fin + 2 * W, fin + 3 * W, qm, rh, sc.rowR, band.dlo, band.dhi, gran);
            prof.hb_split += rtk_clock() - t_p1;
            if (bs_in >= 0) break;
            // R(i) = cost of aligning q[i..qm) with the right half = rowR[qm-1-i]
            // the optimum = the smallest left + right sum over every split point (rows 0 .. qm-2, the row -1 boundary, the last row)
            int mn = 0x7fffffff;
            for (int b0 = 0; b0 + 1 < qm; b0 += RTK_WAVE) { const int qi = b0 + rtk_lane(); if (qi + 1 < qm) { const int v = sc.rowL[qi] + sc.rowR[qm - 2 - qi]; mn = v < mn ? v : mn; } }
            mn = rtk_u(rtk_wave_min(mn));
            const int e0 = lh + sc.rowR[qm - 1], e1 = sc.rowL[qm - 1] + rh;
            mn = e0 < mn ? e0 : mn; mn = e1 < mn ? e1 : mn;
            if (mn <= kk) { bs_known = mn; if (best_out) *best_out = mn; break; }
            kk = mn; // a real score, above the guess: its band holds the optimum
        }
        const unsigned long long t_p1 = rtk_clock();
        const int bs = bs_known;
        int split = -2;
        for (int b0 = 0; b0 + 1 < qm && split == -2; b0 += RTK_WAVE) {
            const int qi = b0 + rtk_lane();
            const bool ok = (qi + 1 < qm) && (sc.rowL[qi] + sc.rowR[qm - 2 - qi] == bs);
            const uint64_t bal = rtk_ballot(ok);
            if (bal) split = b0 + rtk_ffs(bal) - 1;
        }
        int ls, rs;
        if (split >= 0) { ls = sc.rowL[split]; rs = sc.rowR[qm - 2 - split]; }
        else if (lh + sc.rowR[qm - 1] == bs) { split = -1; ls = lh; rs = sc.rowR[qm - 1]; }
        else if (sc.rowL[qm - 1] + rh == bs) { split = qm - 1; ls = sc.rowL[qm - 1]; rs = rh; }
        else { *sc.overflow = 2; return; } // inconsistent optimum: cannot happen for a correct distance
        const int ul = split + 1;
        // push right then left so that the left half is emitted first
        st[5 * sp] = q0 + ul; st[5 * sp + 1] = qm - ul; st[5 * sp + 2] = t0 + lh; st[5 * sp + 3] = rh; st[5 * sp + 4] = rs; ++sp;
        st[5 * sp] = q0; st[5 * sp + 1] = ul; st[5 * sp + 2] = t0; st[5 * sp + 3] = lh; st[5 * sp + 4] = ls; ++sp;
        prof.hb_split += rtk_clock() - t_p1;
    }
    prof.hb_total += rtk_clock() - t_all0;
}

// edlibAlign(..., k = -1, NW or SHW, TASK_PATH): result and moves. When the whole table fits the in-memory traceback branch of
// obtainAlignment (edlib.cpp:1191-1193) ONE stored sweep serves both the distance and the traceback: an SHW matrix restricted to
// columns [0, end] IS the NW matrix of the truncated target edlib re-aligns (same top row, same left column), so the table
// entries, the walk and the moves are the same. Anything else (IUPAC/N in the target, long queries, Hirschberg-sized tables)
// takes the two-pass route.
RTK_FN MyersResult rtk_myers_path(const MyersScratch& sc_, const char* q_, int m_, const char* t_, int n_, int mode_, bool iupac_, uint32_t* n_moves_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const char* q = rtk_u(q_); const char* t = rtk_u(t_); const int m = rtk_u(m_), n = rtk_u(n_), mode = rtk_u(mode_);
    const bool iupac = rtk_u(iupac_); uint32_t* n_moves = rtk_u(n_moves_);
    *n_moves = 0;
    rtk_tb_written(sc);
    MyersResult r; bool have = false;
    if (m > 0 && n > 0 && m <= 4096 && static_cast<uint32_t>(m) <= sc.r_cap && rtk_fits_stored_sweep(sc, m, n)) { // (r_cap: the routes below, when the walk is not taken)
        const SweepStat st = (mode == RTK_MODE_NW) ? rtk_myers_fast_any<1, 0>(q, m, t, n, 1, iupac, rtk_ld(&sc.tb)) : rtk_myers_fast_any<1, 1>(q, m, t, n, 1, iupac, rtk_ld(&sc.tb)); // (the simulator's declines)
        rtk_sync();
        if (st.plain) {
            if (mode == RTK_MODE_NW) { r.dist = st.final_score; r.first = r.last = n - 1; r.nloc = 1; }
            else r = rtk_shw_ends(st.best, st.first, st.last, st.cnt, m);
            have = true;
            const long long tn = (mode == RTK_MODE_NW) ? n : (r.first + 1);
            if (tn > 0 && rtk_tb_in_memory(m, tn)) { rtk_myers_walk(sc, m, static_cast<int>(tn), n, r.dist, n_moves); return r; }
        }
    }
    if (!have && mode == RTK_MODE_NW && m > 0 && n > 0 && !rtk_tb_in_memory(m, n)) {
        // Hirschberg-sized NW problem: the first split yields the distance, no separate distance pass
        int d = -1;
        rtk_myers_alignment(sc, q, m, t, n, -1, iupac, n_moves, &d);
        r.dist = d; r.first = r.last = n - 1; r.nloc = 1;
        return r;
    }
    if (!have) r = rtk_myers_distance(sc, q, m, t, n, -1, mode, iupac);
    if (m > 0 && n > 0) rtk_myers_alignment(sc, q, m, t, (mode == RTK_MODE_NW) ? n : (r.first + 1), r.dist, iupac, n_moves);
    return r;
}

// NW distance and SHW path alignment of the SAME pair from ONE stored sweep. An SHW matrix (top row 0..n, left column 0..m) is the NW
// matrix; its bottom-right cell is the NW distance, the minimum of its last row the SHW result. getScorePath scores a terminal path
// with NW (src/GraphTraversal.cpp:880) and, if it survives, aligns the same two strings again with SHW + path for its quality string
// (:727): rtk_myers_nw_and_save answers the first call and keeps what the second one needs; rtk_myers_path_from_saved then only walks.
RTK_FN bool rtk_myers_nw_and_save(const MyersScratch& sc_, const char* q_, int m_, const char* t_, int n_, bool iupac_, MyersSaved* out_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const char* q = rtk_u(q_); const char* t = rtk_u(t_); const int m = rtk_u(m_), n = rtk_u(n_); const bool iupac = rtk_u(iupac_); MyersSaved* out = rtk_u(out_);
    out->valid = 0;
    if (!(m > 0 && n > 0 && m <= 4096 && static_cast<uint32_t>(m) <= sc.r_cap && rtk_fits_stored_sweep(sc, m, n))) return false; // the pairs rtk_myers_path sweeps once
    uint32_t gen = 0;
    const SweepStat st = rtk_myers_sweep_saved(sc, q, m, t, n, iupac, &gen); // the last row of the sweep: its minimum, where it lies, and D[m][n]
    if (!st.plain) return false;
    const MyersResult r = rtk_shw_ends(st.best, st.first, st.last, st.cnt, m);
    out->m = m; out->n = n; out->nw_dist = st.final_score; out->shw = r; out->gen = gen;
    const long long tn = r.first + 1;
    out->valid = (tn > 0 && rtk_tb_in_memory(m, tn)) ? 1u : 0u; // the walk is the in-memory traceback branch of obtainAlignment
    return true;
}
RTK_FN bool rtk_myers_path_from_saved(const MyersScratch& sc_, const MyersSaved& sv_, uint32_t* n_moves_, MyersResult* r_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); const MyersSaved& sv = *rtk_u(&sv_); uint32_t* n_moves = rtk_u(n_moves_); MyersResult* r = rtk_u(r_);
    *n_moves = 0;
    if (sv.valid == 2u) { *r = sv.shw; rtk_wcopy(rtk_ld(&sc.moves), sv.stash, sv.stash_n); *n_moves = sv.stash_n; return true; } // walked when it was swept
    if (!sv.valid || sv.gen != rtk_ld(&sc.tb_gen)) return false; // the table has been written again since
    *r = sv.shw;
    rtk_myers_walk(sc, sv.m, sv.shw.first + 1, sv.n, sv.shw.dist, n_moves);
    return true;
}
#endif
