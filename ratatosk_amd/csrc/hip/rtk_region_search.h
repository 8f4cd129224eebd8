// Region stage, path search (reference: src/Alignment.cpp selectBest*Alignment :3-147, :967-1015; src/GraphTraversal.cpp getScorePath
// :722-772 and :867-909, exploreSubGraph :456-587, explore :41-93 and :251-304, explorePathsBFS :3-210, explorePathsBFS2 :212-454,
// fixRepeats :1149-1334; src/Correction.cpp extractSemiWeakPaths :3-157). The reference's queue, stack and candidate vectors are small
// handle lists (RtkList); canonical tie rules [D1] (oracle/oracle_correct.hpp) stand where the reference depends on heap addresses.
#ifndef RTK_REGION_SEARCH_H
#define RTK_REGION_SEARCH_H

#include "rtk_region_align.h"
#include "rtk_region_paths.h"
#include "rtk_sets.h"
#include "rtk_seeds.h"

// ------------------------------------------------------------------------------------------------ candidate selection (src/Alignment.cpp:3-147, 967-1015)
// handles[] are committed paths; strings are materialised into str[RTK_STR_CAND].
RTK_FN void rtk_select_best(const RCtx& c, const uint64_t* handles_, uint32_t n_, const char* ref_, uint32_t ref_len_, int mode_, double cut_, int* best_id, int* best_end) {
    RegionScratch& s = *rtk_u(c.sc); const uint64_t* handles = rtk_u(handles_); const uint32_t n = rtk_u(n_), ref_len = rtk_u(ref_len_); const char* ref = rtk_u(ref_);
    const int mode = rtk_u(mode_); const double cut = rtk_u(cut_);
    double best = 0.0; int bid = -1, bend = -1;
    char* const str0 = rtk_ld(&s.str[RTK_STR_CAND]);
    for (uint32_t i = 0; i < n && !rtk_failed(s); ++i) {
        const uint32_t sl = rtk_rec_to_string(c, rtk_ld(handles + i), str0);
        if (sl == 0xFFFFFFFFu) break;
        const uint32_t norm = (mode == RTK_MODE_NW) ? (sl > ref_len ? sl : ref_len) : sl;
        if (i == 0) {
            const MyersResult a = rtk_align(c, str0, sl, ref, ref_len, -1, mode);
            best = static_cast<double>(rtk_u(a.dist)) / static_cast<double>(norm); bend = rtk_u(a.first); bid = 0;
        } else {
            const int kk = static_cast<int>(best * static_cast<double>(norm) + 1.0); // G5: double -> int as edlibNewAlignConfig receives it
            const MyersResult a = rtk_align(c, str0, sl, ref, ref_len, kk, mode);
            const int ad = rtk_u(a.dist);
            if (ad >= 0 && (static_cast<double>(ad) / static_cast<double>(norm)) < best) { best = static_cast<double>(ad) / static_cast<double>(norm); bend = rtk_u(a.first); bid = static_cast<int>(i); }
        }
    }
    if (mode != RTK_MODE_NW && cut > 0.0 && best > cut) { bid = -1; bend = -1; }
    *best_id = bid; *best_end = bend;
}

// ------------------------------------------------------------------------------------------------ scoring (src/GraphTraversal.cpp:867-909, 722-772)
// path string must already be in str[RTK_STR_PATH] (length sl)
RTK_FN_HOT double rtk_score_path(const RCtx& c, uint32_t sl_, const char* ref_, uint32_t ref_len_, bool terminal_) {
    RegionScratch& s = *rtk_u(c.sc); const uint32_t sl = rtk_u(sl_), ref_len = rtk_u(ref_len_); const char* ref = rtk_u(ref_); const bool terminal = rtk_u(terminal_);
    double score = 0.0;
    if (sl != 0) {
        const char* const str1 = rtk_ld(&s.str[RTK_STR_PATH]);
        if (terminal) { RTK_SITE(RTK_SITE_SCORE_TERMINAL); const MyersResult a = rtk_align(c, str1, sl, ref, ref_len, -1, RTK_MODE_NW); score = 1.0 - (static_cast<double>(rtk_u(a.dist)) / static_cast<double>(sl)); }
        else if (sl >= ref_len) { RTK_SITE(RTK_SITE_SCORE_REF_IN_PATH); const MyersResult a = rtk_align(c, ref, ref_len, str1, sl, -1, RTK_MODE_HW); score = 1.0 - (static_cast<double>(rtk_u(a.dist)) / static_cast<double>(ref_len)); }
        else {
            const uint64_t cap = static_cast<uint64_t>(static_cast<double>(sl) * (1.0 + rtk_u(c.o.weak_region_len_factor)));
            const uint32_t l_ref_len = ref_len < cap ? ref_len : static_cast<uint32_t>(cap);
            RTK_SITE(RTK_SITE_SCORE_PATH_IN_REF); const MyersResult a = rtk_align(c, str1, sl, ref, l_ref_len, -1, RTK_MODE_HW);
            score = 1.0 - (static_cast<double>(rtk_u(a.dist)) / static_cast<double>(sl));
        }
        score = score > 0.0 ? score : 0.0; score = score < 1.0 ? score : 1.0;
    }
    return score;
}

// quality string of a path (SHW path alignment against ref) written to qout[0..sl); path string in str[RTK_STR_PATH]
RTK_FN void rtk_score_path_qual(const RCtx& c, uint32_t sl_, const char* ref_, uint32_t ref_len_, double score_best_, double score_second_, char* qout_, const MyersSaved* saved_ = nullptr) {
    RegionScratch& s = *rtk_u(c.sc); const uint32_t sl = rtk_u(sl_), ref_len = rtk_u(ref_len_); const char* ref = rtk_u(ref_); char* qout = rtk_u(qout_); const MyersSaved* saved = rtk_u(saved_);
    const double score_best = rtk_u(score_best_), score_second = rtk_u(score_second_);
    const unsigned long long tq0 = rtk_clock();
    const double score_comp = score_best * ((score_best == 0.0) ? 0.0 : (1.0 - (score_second / score_best)));
    const char* const str1 = rtk_ld(&s.str[RTK_STR_PATH]);
    uint32_t nm = 0;
    bool resumed = false;
    if (saved && saved->valid && static_cast<uint32_t>(saved->m) == sl && static_cast<uint32_t>(saved->n) == ref_len) { // the sweep that scored this very path is still in the table
        MyersResult r0; const unsigned long long t0 = rtk_clock();
        resumed = rtk_myers_path_from_saved(s.my, *saved, &nm, &r0);
        s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t0;
    }
    if (!resumed) { RTK_SITE(RTK_SITE_PATH_QUAL); rtk_align_path(c, str1, sl, ref, ref_len, RTK_MODE_SHW, &nm); }
    nm = rtk_u(nm);
    const char c_best = rtk_get_qual(score_best, 0, static_cast<uint64_t>(rtk_u(c.o.max_qual)));
    rtk_wfill(qout, rtk_get_qual(score_comp, static_cast<uint64_t>(rtk_u(c.o.out_qual)), static_cast<uint64_t>(rtk_u(c.o.max_qual))), sl);
    // walk the moves: a base gets the best-score quality when it sits on an identical reference base in an M run.
    // query/reference positions of every move come from a prefix count of the moves (chunked wave scan).
    uint32_t qp = 0, rp = 0;
    const uint8_t* mv = rtk_ld(&s.my.moves);
    for (uint32_t i0 = 0; i0 < nm; i0 += RTK_WAVE) {
        const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
        const uint8_t m = i < nm ? mv[i] : 255;
        const bool isq = (m == 0 || m == 3 || m == 1), isr = (m == 0 || m == 3 || m == 2);
        const uint64_t bq = rtk_ballot(isq), br = rtk_ballot(isr);
        const uint64_t lt = (1ull << rtk_lane()) - 1ull;
        const uint32_t myq = qp + static_cast<uint32_t>(rtk_popc(bq & lt)), myr = rp + static_cast<uint32_t>(rtk_popc(br & lt));
        if ((m == 0 || m == 3) && str1[myq] == ref[myr]) qout[myq] = c_best;
        qp += static_cast<uint32_t>(rtk_popc(bq)); rp += static_cast<uint32_t>(rtk_popc(br));
    }
    rtk_sync();
    s.cnt[RTK_RC_CYC_PATHQUAL] += rtk_clock() - tq0;
}

// ------------------------------------------------------------------------------------------------ colour memo (src/GraphTraversal.cpp:485-487)
RTK_FN_HOT bool rtk_colour_ok(const RCtx& c, uint32_t u_, const uint32_t* all_pids_, uint32_t n_all_) {
    RegionScratch& s = *rtk_u(c.sc); const unsigned long long tk0 = rtk_clock(); const uint32_t u = rtk_u(u_), n_all = rtk_u(n_all_); const uint32_t* all_pids = rtk_u(all_pids_);
    const uint32_t mn = rtk_ld(&s.memo_n); const uint32_t* mu = rtk_ld(&s.memo_u); uint8_t* mvv = rtk_ld(&s.memo_v);
    for (uint32_t i0 = 0; i0 < mn; i0 += RTK_WAVE) { // 64 memo entries per step
        const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
        const uint64_t hit = rtk_ballot(i < mn && mu[i] == u);
        if (hit) { s.cnt[RTK_RC_CYC_COLOUR_OK] += rtk_clock() - tk0; return rtk_ld(mvv + i0 + static_cast<uint32_t>(rtk_ffs(hit) - 1)) != 0; }
    }
    const uint32_t mcv = static_cast<uint32_t>(rtk_u(c.o.min_cov_vertices));
    const bool ok = (n_all == 0) || (rtk_u(rtk_shared_with_set(c.g, u, all_pids, n_all, mcv)) >= mcv);
    s.cnt[RTK_RC_COLOUR] += rtk_ld(c.g.card.get() + u) + n_all;
    if (mn < rtk_ld(&s.memo_cap)) { const_cast<uint32_t*>(mu)[mn] = u; mvv[mn] = ok ? 1 : 0; s.memo_n = mn + 1; rtk_sync(); }
    s.cnt[RTK_RC_CYC_COLOUR_OK] += rtk_clock() - tk0;
    return ok;
}

RTK_DEV bool rtk_edge_bit(const GraphView& g, uint32_t u, uint32_t strand, int base) { // UnitigData::getSharedPids (UnitigData.hpp:275-284)
    const uint32_t idx = 1u << base;
    return strand ? ((g.flags[u] & (idx << 4)) != 0) : ((g.flags[u] & idx) != 0);
}
RTK_DEV int rtk_nb_successors(const GraphView& g, const UMap& um) {
    const uint32_t* a = g.adj.get() + 8ull * um.unitig + (um.strand ? 0 : 4);
    int n = 0; for (int b = 0; b < 4; ++b) n += (rtk_ld(a + b) != RTK_NONE32) ? 1 : 0; return n;
}

// ------------------------------------------------------------------------------------------------ DFS (src/GraphTraversal.cpp:456-587)
// Results: handles of terminal / non-terminal paths (arena level RTK_ARENA_DFS) in list[RTK_L_DFS_T] / list[RTK_L_DFS_NT]; returns counts and best scores.
struct DfsOut { uint32_t n_t, n_nt; double t1, nt1, nt2; uint32_t nt_score_deferred, nt_qual_deferred; };
// What the caller needs to finish a non-terminal sub-path later (lazy evaluation, see rtk_explore_subgraph): where its reference
// window starts, its scores (or "not scored yet") and whether its quality string is still to be written.
struct NtPending { uint32_t e; double nt1, nt2; uint32_t score_deferred, qual_deferred; };

RTK_FN_SEARCH DfsOut rtk_explore_subgraph(const RCtx& c, const uint32_t* all_pids_, uint32_t n_all_, const char* ref_, uint32_t ref_len_, uint32_t max_len_path_,
                                    const UMap& um_, const UMap& um_e_, uint32_t level_) {
    // LAZY NON-TERMINAL PATHS. In explorePathsBFS2 a non-terminal sub-path of a DFS call is only used when the queue entry built from
    // it is popped while still shorter than max_len_path (src/GraphTraversal.cpp:364-366, 393-411); its score (HW alignment of the
    // reference window inside a path of four whole unitigs) and its quality string (SHW path alignment + traceback) are consumed by
    // nothing else when it is the ONLY non-terminal candidate of the call: the >= / > bookkeeping of :540-549 has nobody to compare it
    // with, `nt1 < min_score` (:295) cannot hold for min_score <= 0, selectBestSubstringAlignment (:297-300) needs two candidates.
    // So with an end anchor the candidates are collected first; several candidates are scored as the reference does, a single one is
    // handed back unscored, and in both cases the quality string is left to the caller (rtk_explore_paths), which computes score and
    // quality -- same inputs, same values -- only if the path is really extended. Without end anchor (explorePathsBFS) every
    // extension is a candidate at once (:165-172): everything stays eager there.
    RegionScratch& s = *rtk_u(c.sc);
    const uint32_t* all_pids = rtk_u(all_pids_); const char* ref = rtk_u(ref_);
    const uint32_t n_all = rtk_u(n_all_), ref_len = rtk_u(ref_len_), max_len_path = rtk_u(max_len_path_), level = rtk_u(level_);
    const UMap um = rtk_u(um_), um_e = rtk_u(um_e_);
    DfsOut out; out.n_t = 0; out.n_nt = 0; out.t1 = 0.0; out.nt1 = 0.0; out.nt2 = 0.0; out.nt_score_deferred = 0; out.nt_qual_deferred = 0;
    double score_t1 = 0.0, score_nt1 = 0.0, score_t2 = 0.0, score_nt2 = 0.0;
    uint32_t n_t = 0, n_nt = 0;
    s.top[RTK_ARENA_DFS] = 0;
    uint64_t* T = rtk_ld(&s.list[RTK_L_DFS_T]); uint64_t* NT = rtk_ld(&s.list[RTK_L_DFS_NT]);
    uint64_t* stk = rtk_ld(&s.list[RTK_L_DFS_STACK]); uint32_t sp = 0; // entries: handle (0 = empty path) and level, two words each
    const uint32_t list_cap = rtk_ld(&s.list_cap);
    char* const str1 = rtk_ld(&s.str[RTK_STR_PATH]); char* const str2 = rtk_ld(&s.str[RTK_STR_QUAL]);
    const uint32_t* const g_adj = c.g.adj.get(); const uint32_t* const g_flags = c.g.flags.get();
    stk[0] = ~0ull; stk[1] = level; sp = 1;
    WPath& w = s.wp[RTK_WP_DFS];
    const bool has_end = !rtk_um_is_empty(um_e);
    const bool lazy_nt = has_end && !(rtk_u(c.o.min_score) > 0.0);
    const bool lrc = rtk_u(c.o.long_read_correct) != 0;
    const uint32_t max_len_subpath = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<double>(rtk_u(c.k)) * rtk_u(c.o.large_k_factor)));
    uint32_t n_nt_live = 0, n_t_scored = 0;
    MyersSaved& t_saved = s.loc.saved; t_saved.stash = reinterpret_cast<uint8_t*>(rtk_ld(&s.str[RTK_STR_SWEEP_STASH])); t_saved.stash_cap = rtk_ld(&s.str_cap); t_saved.stash_n = 0; t_saved.valid = 0; t_saved.gen = 0; t_saved.m = 0; t_saved.n = 0; t_saved.nw_dist = 0; t_saved.shw.dist = -1; t_saved.shw.first = -1; t_saved.shw.last = -1; t_saved.shw.nloc = 0;
    unsigned long long n_exp = 0;
    const unsigned long long td0 = rtk_clock(); const unsigned long long my0 = s.cnt[RTK_RC_CYC_MYERS];
#ifdef RTK_SIM
    const unsigned long long dfs_al0 = s.cnt[RTK_RC_ALIGN];
#endif
    // Walk 0 prunes (lazy mode only): an extension already longer than max_len_path can neither reach a terminal path that passes the
    // length test of :511 nor a non-terminal leaf that would ever be looked at again, so its subtree is skipped -- unless a LIVE
    // non-terminal candidate turns up, in which case the skipped candidates' scores can decide the survivor and walk 1 repeats the
    // reference's full walk for the non-terminal candidates only (terminal ones are complete after walk 0).
    uint32_t n_pruned = 0;
    for (int walk = 0; walk < 2 && !rtk_failed(s); ++walk) {
    const bool prune = lazy_nt && walk == 0, do_terminal = walk == 0;
    if (walk == 1) { if (!(lazy_nt && n_nt_live > 0 && n_pruned > 0)) break;
#ifdef RTK_SIM
        rtk_sim_site_stat[28][0] += 1;
#endif
        n_nt = 0; n_nt_live = 0; stk[0] = ~0ull; stk[1] = level; sp = 1; }
    while (sp > 0 && !rtk_failed(s)) {
        --sp;
        RTK_PL(s, RTK_LAP_DFS_NT_REST);
        const uint64_t hp = rtk_ld(stk + 2 * sp); const uint32_t lvl = static_cast<uint32_t>(rtk_ld(stk + 2 * sp + 1));
        const UMap um_start = (hp == ~0ull) ? um : rtk_rec_back(s, hp);
        const uint32_t* adj = g_adj + 8ull * um_start.unitig + (um_start.strand ? 0 : 4);
        ++n_exp;
        // the four neighbour slots and the edge bits of this unitig, fetched together
        const uint32_t a4[4] = { rtk_ld(adj), rtk_ld(adj + 1), rtk_ld(adj + 2), rtk_ld(adj + 3) };
        const uint32_t eb = (rtk_ld(g_flags + um_start.unitig) >> (um_start.strand ? 4 : 0)) & 0xFu; // UnitigData::getSharedPids (UnitigData.hpp:275-284)
        const bool rev_order = rtk_u(c.o.a3_strand_order) != 0 && !um_start.strand; // [A3] switch: slot = base appended in walk direction (A,C,G,T)
        RTK_PL(s, RTK_LAP_DFS_POP);
        for (int bi = 0; bi < 4 && !rtk_failed(s); ++bi) {
            const int b = rev_order ? 3 - bi : bi;
            const uint32_t ab = a4[b];
            if (ab == RTK_NONE32) continue;
            UMap sc; sc.unitig = ab >> 1; sc.strand = ab & 1u; sc.dist = 0; sc.len = rtk_nkm_u(c, sc.unitig);
            const bool col_ok = rtk_u(rtk_colour_ok(c, sc.unitig, all_pids, n_all));
            RTK_PL(s, RTK_LAP_DFS_COLOUR_OK);
            if (!(((eb >> b) & 1u) && col_ok)) continue;
            if (do_terminal && has_end && sc.unitig == um_e.unitig && um_e.strand == sc.strand) { // terminal
                if (hp == ~0ull) rtk_wp_clear(w); else rtk_wp_load(s, w, hp);
                UMap pref = sc;
                if (pref.strand) { pref.dist = 0; pref.len = um_e.dist + 1; } else { pref.dist = um_e.dist; pref.len = sc.len - um_e.dist; }
                rtk_wp_extend(c, w, pref);
                RTK_PL(s, RTK_LAP_DFS_T_EXTEND);
                if (rtk_ld(&w.l) <= max_len_path && !rtk_failed(s)) {
                    const uint32_t sl = rtk_u(rtk_ums_to_string(c, rtk_ld(&w.ums), rtk_ld(&w.n), str1));
                    if (sl == 0xFFFFFFFFu) break;
                    RTK_PL(s, RTK_LAP_DFS_T_STRING);
                    // the first terminal candidate of a call -- usually the only one -- is scored by a stored sweep that its quality
                    // string can be read from afterwards (rtk_myers_nw_and_save); further candidates overwrite nothing
                    double sco;
                    ++n_t_scored;
                    if (n_t_scored == 1 && sl != 0 && rtk_myers_nw_and_save(s.my, str1, static_cast<int>(sl), ref, static_cast<int>(ref_len), true, &t_saved)) {
                        s.cnt[RTK_RC_ALIGN] += 1; s.cnt[RTK_RC_CELLS] += static_cast<unsigned long long>((sl + 63) / 64) * ref_len;
                        sco = 1.0 - (static_cast<double>(rtk_u(t_saved.nw_dist)) / static_cast<double>(sl));
                        sco = sco > 0.0 ? sco : 0.0; sco = sco < 1.0 ? sco : 1.0;
                    } else sco = rtk_u(rtk_score_path(c, sl, ref, ref_len, true));
                    RTK_PL(s, RTK_LAP_DFS_T_SWEEP);
                    if (sco >= score_t1) {
                        if (sco > score_t1) n_t = 0;
                        if (n_t >= list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                        T[n_t++] = rtk_wp_commit(s, w, RTK_ARENA_DFS);
                        score_t2 = score_t1; score_t1 = sco;
                    } else if (sco > score_t2) score_t2 = sco;
                    RTK_PL(s, RTK_LAP_DFS_T_COMMIT);
                }
            }
            { // non-terminal
                if (prune) { // length of the extension (Path::extend, Path.hpp:319-330) before building it
                    const uint32_t l_new = (hp == ~0ull) ? (sc.len + static_cast<uint32_t>(rtk_u(c.k)) - 1u) : (rtk_rec_l(s, hp) + sc.len);
                    if (l_new > max_len_path) { ++n_pruned; continue; }
                }
                if (hp == ~0ull) rtk_wp_clear(w); else rtk_wp_load(s, w, hp);
                rtk_wp_extend(c, w, sc);
                if (rtk_failed(s)) break;
                RTK_PL(s, RTK_LAP_DFS_NT_EXTEND);
#ifdef RTK_SIM
                rtk_sim_site_stat[20][0] += 1; rtk_sim_site_stat[20][1] += sc.len + ((hp == ~0ull) ? static_cast<uint32_t>(rtk_u(c.k)) - 1 : 0); // DFS tree nodes and the columns they add
#endif
                // exploreSubGraph descends `level` unitigs (:531-535), exploreSubGraphLong (pass 2) until the sub-path spans k * large_k_factor (:594, :669-671)
                const bool deeper = lrc ? (rtk_ld(&w.l) < max_len_subpath) : (lvl != 0);
                if (deeper) {
                    if (2 * (sp + 1) > list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                    stk[2 * sp] = rtk_wp_commit(s, w, RTK_ARENA_DFS); stk[2 * sp + 1] = lvl ? lvl - 1 : 0; ++sp;
                } else if (rtk_nb_successors(c.g, sc) > 0) {
                    if (lazy_nt) { // candidate kept in discovery order, scored after the walk (or never)
                        if (n_nt >= list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                        NT[n_nt++] = rtk_wp_commit(s, w, RTK_ARENA_DFS);
                        // P (+) Q is looked at again only if it is shorter than the caller's max_len_path (:364-366); in terms of this call's
                        // arguments (max_len_path here = the caller's minus the characters of P before its last unitig `um`): l(Q) + um.len < max_len_path
                        if (rtk_ld(&w.l) + um.len < max_len_path) ++n_nt_live;
                    } else {
                        const uint32_t sl = rtk_u(rtk_ums_to_string(c, rtk_ld(&w.ums), rtk_ld(&w.n), str1));
                        if (sl == 0xFFFFFFFFu) break;
                        const double sco = rtk_u(rtk_score_path(c, sl, ref, ref_len, false));
                        if (sco >= score_nt1) {
                            if (sco > score_nt1) n_nt = 0;
                            if (n_nt >= list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                            NT[n_nt++] = rtk_wp_commit(s, w, RTK_ARENA_DFS);
                            score_nt2 = score_nt1; score_nt1 = sco;
                        } else if (sco > score_nt2) score_nt2 = sco;
                    }
                }
            }
        }
    }
    } // walk
#ifdef RTK_SIM
    { const unsigned long long na = s.cnt[RTK_RC_ALIGN] - dfs_al0; const unsigned b = na > 15 ? 15 : static_cast<unsigned>(na); rtk_sim_site_stat[21][0] += 1; rtk_sim_site_stat[22 + (b >> 3)][b & 7] += 1; rtk_sim_site_stat[24 + (b >> 3)][b & 7] += na; }
#endif
    RTK_PL(s, RTK_LAP_DFS_NT_REST);
    s.cnt[RTK_RC_EXPAND] += n_exp; RTK_HIST_ADD(s, RTK_H_DFS_RUNNING, 1);
    s.cnt[RTK_RC_CYC_DFS] += (rtk_clock() - td0) - (s.cnt[RTK_RC_CYC_MYERS] - my0); // DFS bookkeeping: loop time minus the alignments inside it
    bool nt_score_deferred = false;
    if (lazy_nt && !rtk_failed(s)) {
        // whichever candidate survives the scoring is only re-queued; if none of them can pass the length test of the pop, the queue
        // ends empty whatever the scores are: nothing to compute (a mix of short and long candidates still needs every score)
        if (n_nt_live == 0) n_nt = 0;
        if (n_nt == 1) nt_score_deferred = true; // nobody to compare it with: scored by the caller if the path is ever extended
        else if (n_nt > 1) { // the reference's bookkeeping (:540-549) over the candidates in discovery order
            const uint32_t n_cand = n_nt; n_nt = 0;
            for (uint32_t i = 0; i < n_cand && !rtk_failed(s); ++i) {
                const uint64_t hc = rtk_ld(NT + i);
                rtk_wp_load(s, w, hc);
                const uint32_t sl = rtk_u(rtk_ums_to_string(c, rtk_ld(&w.ums), rtk_ld(&w.n), str1));
                if (sl == 0xFFFFFFFFu) break;
                const double sco = rtk_u(rtk_score_path(c, sl, ref, ref_len, false));
                if (sco >= score_nt1) {
                    if (sco > score_nt1) n_nt = 0;
                    NT[n_nt++] = hc; // n_nt <= i: survivors move towards the front
                    score_nt2 = score_nt1; score_nt1 = sco;
                } else if (sco > score_nt2) score_nt2 = sco;
            }
        }
    }
    RTK_PL(s, RTK_LAP_DFS_POST_SCORE);
    // qualities (:556-584): re-commit every surviving path with its quality string (non-terminal ones: left to the caller when lazy)
    for (int which = 0; which < (lazy_nt ? 1 : 2) && !rtk_failed(s); ++which) {
        uint64_t* L = which ? NT : T; const uint32_t nL = which ? n_nt : n_t;
        for (uint32_t i = 0; i < nL && !rtk_failed(s); ++i) {
            rtk_wp_load(s, w, rtk_ld(L + i));
            const uint32_t sl = rtk_u(rtk_ums_to_string(c, rtk_ld(&w.ums), rtk_ld(&w.n), str1));
            if (sl == 0xFFFFFFFFu || sl > rtk_ld(&s.str_cap)) { rtk_fail_ovf(s, RTK_OVF_STRING); break; }
            RTK_PL(s, RTK_LAP_DFS_POST_STRING);
            rtk_score_path_qual(c, sl, ref, ref_len, which ? score_nt1 : score_t1, which ? score_nt2 : score_t2, str2, (which == 0 && n_t_scored == 1) ? &t_saved : nullptr);
            RTK_PL(s, RTK_LAP_DFS_POST_QUAL);
            if (sl == rtk_ld(&w.l)) { rtk_wcopy(rtk_ld(&w.qual), str2, sl); w.qlen = sl; } // Path::setQuality only accepts q.length() == l
            L[i] = rtk_wp_commit(s, w, RTK_ARENA_DFS);
            RTK_PL(s, RTK_LAP_DFS_POST_COMMIT);
        }
    }
    out.n_t = n_t; out.n_nt = n_nt; out.t1 = score_t1; out.nt1 = score_nt1; out.nt2 = score_nt2;
    out.nt_score_deferred = nt_score_deferred ? 1u : 0u; out.nt_qual_deferred = (lazy_nt && n_nt != 0) ? 1u : 0u;
    return out;
}

// explore() (src/GraphTraversal.cpp:41-93, 251-304). p = committed path (RTK_ARENA_BFS). Results stay in list[RTK_L_DFS_T] / list[RTK_L_DFS_NT] (arena level RTK_ARENA_DFS).
RTK_FN_SEARCH void rtk_explore(const RCtx& c_, const uint32_t* all_pids_, uint32_t n_all_, const char* ref_, uint32_t ref_len_, const UMap& um_e_, uint64_t hp_, uint32_t max_len_path_, uint32_t* n_t_, uint32_t* n_nt_, NtPending* pend_) {
    const RCtx& c = *rtk_u(&c_); const uint32_t* all_pids = rtk_u(all_pids_); uint32_t n_all = rtk_u(n_all_); const char* ref = rtk_u(ref_); uint32_t ref_len = rtk_u(ref_len_); const UMap um_e = rtk_u(um_e_); uint64_t hp = rtk_u(hp_); uint32_t max_len_path = rtk_u(max_len_path_); uint32_t* n_t = rtk_u(n_t_); uint32_t* n_nt = rtk_u(n_nt_); NtPending* pend = rtk_u(pend_);
    RegionScratch& s = rtk_hdr(c);
    *n_t = 0; *n_nt = 0; pend->e = 0; pend->nt1 = 0.0; pend->nt2 = 0.0; pend->score_deferred = 0; pend->qual_deferred = 0;
    const UMap um = rtk_rec_back(s, hp);
    const uint32_t path_len = rtk_rec_l(s, hp);
    const uint32_t k = static_cast<uint32_t>(c.k);
    const bool non_empty_path = (path_len > (um.len + k - 1)) && !rtk_um_is_empty(um);
    const uint32_t path_len_prefix = non_empty_path ? (path_len - um.len - k + 1) : 0;
    uint32_t end_pos_ref = 0;
    if (non_empty_path) {
        const uint32_t sl = rtk_rec_to_string(c, hp, s.str[RTK_STR_CAND]);
        if (sl == 0xFFFFFFFFu) return;
        RTK_SITE(RTK_SITE_EXPLORE_PREFIX); const MyersResult a = rtk_align(c, s.str[RTK_STR_CAND], path_len_prefix, ref, ref_len, -1, RTK_MODE_SHW);
        end_pos_ref = static_cast<uint32_t>(a.first + 1);
    }
    RTK_PL(s, RTK_LAP_EXPLORE_PREFIX);
    if ((ref_len - end_pos_ref) != 0 && path_len < max_len_path) {
        DfsOut o = rtk_explore_subgraph(c, all_pids, n_all, ref + end_pos_ref, ref_len - end_pos_ref, max_len_path - path_len_prefix, um, um_e, 3);
        if (rtk_failed(s)) return;
        if (o.n_t && o.t1 < c.o.min_score) o.n_t = 0;
        if (o.n_nt && !o.nt_score_deferred && o.nt1 < c.o.min_score) o.n_nt = 0; // a deferred score only exists for min_score <= 0: never below it
        pend->e = end_pos_ref; pend->nt1 = o.nt1; pend->nt2 = o.nt2; pend->score_deferred = o.nt_score_deferred; pend->qual_deferred = o.nt_qual_deferred;
        if (o.n_nt > 1) {
            int bid, bend;
            RTK_SITE(RTK_SITE_SELECT_NT); rtk_select_best(c, s.list[RTK_L_DFS_NT], o.n_nt, ref + end_pos_ref, ref_len - end_pos_ref, RTK_MODE_HW, -1.0, &bid, &bend);
            s.list[RTK_L_DFS_NT][0] = s.list[RTK_L_DFS_NT][bid]; o.n_nt = 1;
        }
        *n_t = o.n_t; *n_nt = o.n_nt;
    }
}

// P (+) Q: w = copy of p extended by every mapping of sub with its quality slice (src/GraphTraversal.cpp:379-390)
RTK_FN_LEAF void rtk_extend_by(const RCtx& c_, WPath& w_, uint64_t hsub_, uint32_t upto_) {
    const RCtx& c = *rtk_u(&c_); WPath& w = *rtk_u(&w_); RTK_ASSUME_LDS(&w); uint64_t hsub = rtk_u(hsub_); uint32_t upto = rtk_u(upto_);
    RegionScratch& s = rtk_hdr(c);
    const int lv = rtk_h_lvl(hsub); const uint64_t oo = rtk_h_off(hsub);
    const PathHdr* h = rtk_path_hdr(s, lv, oo); const UMap* ums = rtk_path_ums(s, lv, oo); const char* q = rtk_path_qual(s, lv, oo);
    uint32_t j = 0;
    for (uint32_t i = 0; i < h->n && i < upto && !rtk_failed(s); ++i) {
        const uint32_t want = ums[i].len + static_cast<uint32_t>(c.k) - 1;
        uint32_t qn = 0;
        if (j <= h->qlen) qn = (h->qlen - j) < want ? (h->qlen - j) : want; // std::string::substr clamps
        rtk_wp_extend_q(c, w, ums[i], q + j, qn);
        j += ums[i].len;
    }
}

RTK_FN void rtk_resize_to_best(const RCtx& c_, uint64_t* v_, uint32_t* n_, const char* ref_, uint32_t ref_len_) {
    const RCtx& c = *rtk_u(&c_); uint64_t* v = rtk_u(v_); uint32_t* n = rtk_u(n_); const char* ref = rtk_u(ref_); uint32_t ref_len = rtk_u(ref_len_); // resizeVector
    if (*n <= 1) return;
    int bid, bend;
    RTK_SITE(RTK_SITE_RESIZE_BEST); rtk_select_best(c, v, *n, ref, ref_len, RTK_MODE_SHW, -1.0, &bid, &bend);
    if (rtk_failed(*c.sc)) return;
    v[0] = v[bid]; *n = 1;
}

RTK_DEV UMap rtk_start_suffix(const RCtx& c, const UMap& um_s) { // src/GraphTraversal.cpp:113-125, 325-338
    UMap t = um_s;
    if (t.strand) { t.dist += t.len - 1; t.len = rtk_nkm(c.g, um_s.unitig) - t.dist; }
    else { t.len = um_s.dist + 1; t.dist = 0; }
    return t;
}

// explorePathsBFS2 / explorePathsBFS. Returns a handle (RTK_ARENA_BFS) of the single resulting path, or ~0 if none.
// ------------------------------------------------------------------------------------------------ fixRepeats (src/GraphTraversal.cpp:1149-1334)
// For every unitig of the path that lies on a short cycle (micro / mini-satellite motif) the stored compact cycles are tried as one
// more turn through it: prefix + [unitig to its end, cycle unitigs, unitig from its start] + suffix; a turn is kept when it lowers the
// NW distance to the read window (bounded by the distance so far). Identity when no unitig of the path is flagged.
// is any unitig of the path on a short cycle? (the fast way out of fixRepeats, tested by the caller so that the common case costs no call)
RTK_DEV bool rtk_path_has_short_cycle(const RCtx& c, uint64_t hp) {
    RegionScratch& s = rtk_hdr(c); const GraphView& g = c.g;
    const int lv = rtk_h_lvl(hp); const uint64_t oo = rtk_h_off(hp);
    const UMap* pu = rtk_path_ums(s, lv, oo); const uint32_t pn = rtk_rec_n(s, hp);
    bool any = false;
    for (uint32_t i0 = 0; i0 < pn && !any; i0 += RTK_WAVE) { const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane()); any = rtk_ballot(i < pn && (g.flags[pu[i].unitig] & RTK_F_SHORT_CYCLE)) != 0ull; }
    return any;
}
RTK_FN uint64_t rtk_fix_repeats(const RCtx& c_, uint64_t hp_, const char* ref_, uint32_t ref_len_) {
    const RCtx& c = *rtk_u(&c_); const uint64_t hp = rtk_u(hp_); const char* ref = rtk_u(ref_); const uint32_t ref_len = rtk_u(ref_len_);
    RegionScratch& s = rtk_hdr(c);
    const GraphView& g = c.g;
    const uint32_t k = static_cast<uint32_t>(c.k);
    WPath& P = s.wp[RTK_WP_REPEATS_PATH]; WPath& E = s.wp[RTK_WP_REPEATS_TRIAL]; UMap* R = s.wp[RTK_WP_REPEATS_CYCLE].ums;
    rtk_wp_load(s, P, hp);
    if (rtk_failed(s)) return ~0ull;
    const char q_max = rtk_get_qual(1.0, 0, static_cast<uint64_t>(c.o.max_qual));
    int ed;
    { const uint32_t sl = rtk_ums_to_string(c, P.ums, P.n, s.str[RTK_STR_CAND]); if (sl == 0xFFFFFFFFu) return ~0ull; RTK_SITE(RTK_SITE_REPEATS_PATH); ed = rtk_u(rtk_align(c, s.str[RTK_STR_CAND], sl, ref, ref_len, -1, RTK_MODE_NW).dist); }
    for (uint32_t i = 0; i < P.n && !rtk_failed(s); ++i) {
        const UMap um_path = rtk_u(P.ums[i]);
        if (!(g.flags[um_path.unitig] & RTK_F_SHORT_CYCLE)) continue;
        uint64_t best_h = ~0ull;
        UMap um_start = um_path, um_end = um_path; // the unitig from the mapped start to its end / from its beginning to the mapped end, both forward (:1213-1224)
        um_start.len = rtk_nkm(g, um_path.unitig) - um_path.dist; um_start.strand = 1;
        um_end.dist = 0; um_end.len = um_path.dist + um_path.len; um_end.strand = 1;
        const char* cyc = g.cyc; const uint64_t c_lo = g.cycoff[um_path.unitig], c_hi = g.cycoff[um_path.unitig + 1];
        for (uint64_t a = c_lo; a < c_hi && !rtk_failed(s);) {
            // Path(um_start, cycle, um_end) (Path.hpp:109-152) as an explicit unitig list R
            uint32_t nR = 0, rep_l = um_start.len + k - 1; bool ok = true;
            if (s.um_cap < 4) { rtk_fail_ovf(s, RTK_OVF_PATH_UNITIGS); break; }
            R[nR++] = um_start;
            UMap curr = um_start;
            uint64_t e = a;
            for (; e < c_hi; ++e) {
                const char ch = rtk_ld(cyc + e);
                if (ch == 0) break;
                const uint32_t nb = rtk_ld(g.adj + 8ull * curr.unitig + (curr.strand ? 0 : 4) + (((static_cast<uint32_t>(ch) >> 1) & 3u) ^ (((static_cast<uint32_t>(ch) >> 1) & 3u) >> 1))); // A,C,G,T -> 0..3
                if (nb == RTK_NONE32) { ok = false; continue; }
                if (!ok) continue;
                curr.unitig = nb >> 1; curr.strand = nb & 1u; curr.dist = 0; curr.len = rtk_nkm(g, curr.unitig);
                if (nR + 2 > s.um_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_UNITIGS); break; }
                R[nR++] = curr; rep_l += curr.len;
            }
            a = e + 1;
            if (rtk_failed(s)) break;
            if (ok) { R[nR++] = um_end; rep_l += um_end.len; } else { nR = 0; rep_l = 0; }
            rtk_sync();
            if (!um_path.strand) { // rev_comp (Path.hpp:208-262): reversed order, flipped strands
                for (uint32_t x = 0; x < nR / 2; ++x) { const UMap t = rtk_u(R[x]); R[x] = R[nR - 1 - x]; R[nR - 1 - x] = t; }
                rtk_sync();
                for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < nR; x += RTK_WAVE) R[x].strand ^= 1u;
                rtk_sync();
            }
            // evaluatePath (:1167-1201)
            rtk_wp_clear(E);
            uint32_t len_prefix = 0;
            for (uint32_t j = 0; j < i; ++j) { const UMap u = rtk_u(P.ums[j]); rtk_wp_extend(c, E, u); len_prefix += u.len; }
            for (uint32_t x = 0; x < nR; ++x) { const UMap u = rtk_u(R[x]); rtk_wp_extend(c, E, u); }
            for (uint32_t j = i + 1; j < P.n; ++j) { const UMap u = rtk_u(P.ums[j]); rtk_wp_extend(c, E, u); }
            if (rtk_failed(s)) break;
            const uint32_t qn = P.qlen;
            if (len_prefix > qn) { rtk_fail_ovf(s, RTK_OVF_REPEAT_QUAL); break; } // std::string::replace would throw in the reference: a path without qualities never gets here
            const uint32_t cut = (um_path.len + k - 1) < (qn - len_prefix) ? (um_path.len + k - 1) : (qn - len_prefix);
            const uint32_t new_len = qn - cut + rep_l;
            E.qlen = 0;
            if (new_len == E.l) { // Path::setQuality
                if (new_len > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_QUAL); break; }
                rtk_wcopy(E.qual, P.qual, len_prefix);
                rtk_wfill(E.qual + len_prefix, q_max, rep_l);
                rtk_wcopy(E.qual + len_prefix + rep_l, P.qual + len_prefix + cut, qn - len_prefix - cut);
                E.qlen = new_len;
            }
            const uint32_t sl = rtk_ums_to_string(c, E.ums, E.n, s.str[RTK_STR_CAND]); if (sl == 0xFFFFFFFFu) break;
            RTK_SITE(RTK_SITE_REPEATS_TURN); const int d = rtk_u(rtk_align(c, s.str[RTK_STR_CAND], sl, ref, ref_len, ed, RTK_MODE_NW).dist);
            if (d >= 0 && d < ed) { ed = d; best_h = rtk_wp_commit(s, E, RTK_ARENA_BFS); }
        }
        if (rtk_failed(s)) break;
        if (best_h != ~0ull) { // a better aligning path: go on behind the inserted unitigs (:1283-1292)
            const uint32_t diff = rtk_rec_n(s, best_h) - P.n;
            rtk_wp_load(s, P, best_h);
            i += diff - 1;
        } else {
            while (i + 1 < P.n && rtk_u(P.ums[i + 1]).unitig == um_path.unitig) ++i;
        }
    }
    if (rtk_failed(s)) return ~0ull;
    return rtk_wp_commit(s, P, RTK_ARENA_BFS);
}

RTK_FN_SEARCH uint64_t rtk_explore_paths(const RCtx& c_, const uint32_t* all_pids_, uint32_t n_all_, const char* ref_, uint32_t ref_len_, const UMap& um_s_, const UMap& um_e_, bool has_end_) {
    const RCtx& c = *rtk_u(&c_); const uint32_t* all_pids = rtk_u(all_pids_); uint32_t n_all = rtk_u(n_all_); const char* ref = rtk_u(ref_); uint32_t ref_len = rtk_u(ref_len_); const UMap um_s = rtk_u(um_s_); const UMap um_e = rtk_u(um_e_); bool has_end = rtk_u(has_end_);
    RegionScratch& s = rtk_hdr(c);
    const uint32_t k = static_cast<uint32_t>(c.k);
    s.top[RTK_ARENA_BFS] = 0; s.memo_n = 0;
    uint64_t* v = s.list[RTK_L_BFS_PATHS]; uint64_t* v_tmp = s.list[RTK_L_BFS_NEW];
    uint32_t nv = 0, nvt = 0;
    const char q_max = rtk_get_qual(1.0, 0, static_cast<uint64_t>(c.o.max_qual));
    const bool ok_start = !rtk_um_is_empty(um_s) && ((c.g.flags[um_s.unitig] & RTK_F_EDGE_MASK) != 0);
    const bool ok_end = !has_end || (!rtk_um_is_empty(um_e) && ((c.g.flags[um_e.unitig] & RTK_F_EDGE_MASK) != 0));
    if (ok_start && ok_end) {
        const uint32_t level = 4;
        const bool lrc = c.o.long_read_correct != 0;
        const uint32_t max_len_subpath = static_cast<uint32_t>(static_cast<uint64_t>(static_cast<double>(c.k) * c.o.large_k_factor));
        uint64_t mn, mx; rtk_min_max_len(ref_len - k, c.o.weak_region_len_factor, &mn, &mx);
        const uint32_t min_len_path = static_cast<uint32_t>(mn) + k;
        const uint32_t max_len_path = static_cast<uint32_t>(mx > 10 ? mx : 10) + k;
        const uint32_t max_paths = 1024;
        WPath& w = s.wp[RTK_WP_BFS];
        const UMap ust = rtk_start_suffix(c, um_s);
        if (has_end) {
            if (um_s.unitig == um_e.unitig && um_s.strand == um_e.strand && ust.dist <= um_e.dist) { // :340-358
                const uint32_t len = (ust.len + k - 1) - (um_e.strand ? (rtk_ulen(c.g, um_e.unitig) - um_e.dist - k) : um_e.dist);
                if (len >= min_len_path && len <= max_len_path) {
                    UMap bt = ust;
                    if (bt.strand) bt.len = um_e.dist - bt.dist + 1; else { bt.dist = um_e.dist; bt.len -= um_e.dist; }
                    rtk_wp_start(c, w, bt, q_max);
                    if (nv < s.list_cap) v[nv++] = rtk_wp_commit(s, w, RTK_ARENA_BFS); else rtk_fail_ovf(s, RTK_OVF_LIST);
                }
            }
        } else if ((ust.len + k - 1) >= min_len_path) { // :127-140
            UMap back = ust;
            if ((back.len + k - 1) > max_len_path) { if (!back.strand) back.dist = back.len - (max_len_path - k + 1); back.len = max_len_path - k + 1; }
            rtk_wp_start(c, w, back, q_max);
            v[nv++] = rtk_wp_commit(s, w, RTK_ARENA_BFS);
        }
        rtk_wp_start(c, w, ust, q_max);
        uint64_t qh = rtk_wp_commit(s, w, RTK_ARENA_BFS); bool q_has = true; // the queue never holds more than one path (each pop pushes <= 1)
        // a queue entry P (+) Q whose non-terminal sub-path Q has not been given its score / quality string yet (see rtk_explore_subgraph)
        bool q_pending = false; uint64_t pend_hp = 0, pend_hq = 0; NtPending pend; pend.e = 0; pend.nt1 = 0.0; pend.nt2 = 0.0; pend.score_deferred = 0; pend.qual_deferred = 0;
        RTK_PL(s, RTK_LAP_PATHS_PROLOGUE);
        while (q_has && !rtk_failed(s)) {
            if (q_pending) { // the pop of src/GraphTraversal.cpp:364-366: only a path shorter than max_len_path is ever looked at again
                q_pending = false;
                const int lv = rtk_h_lvl(pend_hq); const uint64_t oo = rtk_h_off(pend_hq);
                const UMap* qu = rtk_path_ums(s, lv, oo); const uint32_t qn = rtk_rec_n(s, pend_hq);
                uint32_t l_ext = rtk_rec_l(s, pend_hp);
                for (uint32_t i = 0; i < qn; ++i) l_ext += rtk_u(qu[i].len); // Path::extend adds um.len per unitig (Path.hpp:319-330)
                if (!(l_ext < max_len_path)) break;
                WPath& wq = s.wp[RTK_WP_DFS];
                rtk_wp_load(s, wq, pend_hq);
                const uint32_t sl = rtk_u(rtk_ums_to_string(c, rtk_ld(&wq.ums), rtk_ld(&wq.n), s.str[RTK_STR_PATH]));
                if (sl == 0xFFFFFFFFu || sl > rtk_ld(&s.str_cap)) { rtk_fail_ovf(s, RTK_OVF_STRING); break; }
                double nt1 = pend.nt1; const double nt2 = pend.nt2;
                if (pend.score_deferred) nt1 = rtk_u(rtk_score_path(c, sl, ref + pend.e, ref_len - pend.e, false));
                rtk_score_path_qual(c, sl, ref + pend.e, ref_len - pend.e, nt1, nt2, s.str[RTK_STR_QUAL]);
                if (sl == rtk_ld(&wq.l)) { rtk_wcopy(rtk_ld(&wq.qual), s.str[RTK_STR_QUAL], sl); wq.qlen = sl; } // Path::setQuality only accepts q.length() == l
                const uint64_t hq = rtk_wp_commit(s, wq, RTK_ARENA_BFS);
                if (rtk_failed(s)) break;
                rtk_wp_load(s, w, pend_hp); rtk_extend_by(c, w, hq, 0xFFFFFFFFu);
                qh = rtk_wp_commit(s, w, RTK_ARENA_BFS);
                if (rtk_failed(s)) break;
            }
            const uint64_t hp = qh; q_has = false;
            if (rtk_rec_l(s, hp) < max_len_path) {
                uint32_t n_t, n_nt;
                RTK_PL(s, RTK_LAP_PATHS_AFTER_EXPLORE);
                rtk_explore(c, all_pids, n_all, ref, ref_len, has_end ? um_e : rtk_um_empty(), hp, max_len_path, &n_t, &n_nt, &pend);
                if (rtk_failed(s)) break;
                if (has_end) {
                    for (uint32_t i = 0; i < n_t && !rtk_failed(s); ++i) {
                        rtk_wp_load(s, w, hp); rtk_extend_by(c, w, s.list[RTK_L_DFS_T][i], 0xFFFFFFFFu);
                        if (nvt >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                        v_tmp[nvt++] = rtk_wp_commit(s, w, RTK_ARENA_BFS);
                    }
                    for (uint32_t i = 0; i < n_nt && !rtk_failed(s); ++i) {
                        if (lrc ? (rtk_rec_l(s, s.list[RTK_L_DFS_NT][i]) >= max_len_subpath) : (rtk_rec_n(s, s.list[RTK_L_DFS_NT][i]) == level)) { // :395
                            if (pend.qual_deferred) { // keep what is needed to finish Q when (if) the entry is popped: its unitigs move to the BFS-level arena
                                rtk_wp_load(s, s.wp[RTK_WP_DFS], s.list[RTK_L_DFS_NT][i]);
                                pend_hq = rtk_wp_commit(s, s.wp[RTK_WP_DFS], RTK_ARENA_BFS); pend_hp = hp; q_pending = true; q_has = true;
                            } else {
                                rtk_wp_load(s, w, hp); rtk_extend_by(c, w, s.list[RTK_L_DFS_NT][i], 0xFFFFFFFFu);
                                qh = rtk_wp_commit(s, w, RTK_ARENA_BFS); q_has = true; // queue size 1 < 512: resizeQueue never fires
                            }
                        }
                    }
                    if (nvt >= max_paths) {
                        for (uint32_t i = 0; i < nvt && !rtk_failed(s); ++i) {
                            const uint32_t l = rtk_rec_l(s, v_tmp[i]);
                            if (l >= min_len_path && l <= max_len_path) { if (nv + 1 >= max_paths) rtk_resize_to_best(c, v, &nv, ref, ref_len); if (nv >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; } v[nv++] = v_tmp[i]; }
                        }
                        nvt = 0;
                    }
                } else { // BFS without end anchor: every extension inside the length window is a candidate (:158-191)
                    for (uint32_t i = 0; i < n_nt && !rtk_failed(s); ++i) {
                        const uint64_t hs = s.list[RTK_L_DFS_NT][i];
                        const uint32_t nsub = rtk_rec_n(s, hs);
                        for (uint32_t u = 1; u <= nsub && !rtk_failed(s); ++u) {
                            rtk_wp_load(s, w, hp); rtk_extend_by(c, w, hs, u);
                            if (w.l >= min_len_path && w.l <= max_len_path) { if (nvt >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; } v_tmp[nvt++] = rtk_wp_commit(s, w, RTK_ARENA_BFS); }
                            if (u == nsub && (lrc ? (rtk_rec_l(s, hs) >= max_len_subpath) : (nsub == level))) { qh = rtk_wp_commit(s, w, RTK_ARENA_BFS); q_has = true; } // :174
                        }
                    }
                    if (nvt >= max_paths) {
                        for (uint32_t i = 0; i < nvt && !rtk_failed(s); ++i) {
                            rtk_wp_load(s, w, v_tmp[i]); rtk_wp_prune_prefix(c, w, max_len_path);
                            if (nv >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                            v[nv++] = rtk_wp_commit(s, w, RTK_ARENA_BFS);
                        }
                        nvt = 0;
                    }
                }
            }
        }
        if (!rtk_failed(s)) { // final flush
            if (has_end) {
                for (uint32_t i = 0; i < nvt && !rtk_failed(s); ++i) {
                    const uint32_t l = rtk_rec_l(s, v_tmp[i]);
                    if (l >= min_len_path && l <= max_len_path) { if (nv + 1 >= max_paths) rtk_resize_to_best(c, v, &nv, ref, ref_len); if (nv >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; } v[nv++] = v_tmp[i]; }
                }
            } else {
                for (uint32_t i = 0; i < nvt && !rtk_failed(s); ++i) {
                    rtk_wp_load(s, w, v_tmp[i]); rtk_wp_prune_prefix(c, w, max_len_path);
                    if (nv >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
                    v[nv++] = rtk_wp_commit(s, w, RTK_ARENA_BFS);
                }
            }
        }
    }
    RTK_PL(s, RTK_LAP_PATHS_AFTER_EXPLORE);
    if (rtk_failed(s) || nv == 0) return ~0ull;
    if (nv > 1) { int bid, bend; RTK_SITE(RTK_SITE_SELECT_BFS); rtk_select_best(c, v, nv, ref, ref_len, RTK_MODE_NW, -1.0, &bid, &bend); if (rtk_failed(s)) return ~0ull; v[0] = v[bid]; }
    { const uint64_t r_ = rtk_path_has_short_cycle(c, v[0]) ? rtk_fix_repeats(c, v[0], ref, ref_len) : v[0]; RTK_PL(s, RTK_LAP_PATHS_SELECT); return r_; }
}

// ------------------------------------------------------------------------------------------------ extractSemiWeakPaths (src/Correction.cpp:3-157)
// BFS results never hold more than one path, so `paths1` is a single running path (RTK_ARENA_REGION). Dead ends are appended to
// `partial` (list[RTK_L_PARTIAL]). Returns the complete path handle or ~0.
RTK_FN_SEARCH uint64_t rtk_extract_semi_weak(const RCtx& c_, const char* s_read_, uint32_t s_len_, const uint32_t* all_pids_, uint32_t n_all_, uint32_t start_pos_, const UMap& start_um_, uint32_t end_pos_in_, const UMap& end_um_, const Anchors& lvw_, uint32_t lvw_lo_, uint32_t lvw_hi_, uint32_t i_weak_, uint32_t* n_partial_) {
    const RCtx& c = *rtk_u(&c_); const char* s_read = rtk_u(s_read_); uint32_t s_len = rtk_u(s_len_); const uint32_t* all_pids = rtk_u(all_pids_); uint32_t n_all = rtk_u(n_all_); uint32_t start_pos = rtk_u(start_pos_); const UMap start_um = rtk_u(start_um_); uint32_t end_pos_in = rtk_u(end_pos_in_); const UMap end_um = rtk_u(end_um_); const Anchors& lvw = *rtk_u(&lvw_); uint32_t lvw_lo = rtk_u(lvw_lo_); uint32_t lvw_hi = rtk_u(lvw_hi_); uint32_t i_weak = rtk_u(i_weak_); uint32_t* n_partial = rtk_u(n_partial_);
    RegionScratch& s = rtk_hdr(c);
    const uint32_t k = static_cast<uint32_t>(c.k);
    const bool no_end = rtk_um_is_empty(end_um);
    const uint32_t pos2 = no_end ? s_len - k : end_pos_in;
    const uint32_t max_len_weak_region = c.o.long_read_correct ? c.o.max_len_weak_region2 : c.o.max_len_weak_region1; // :23
    uint32_t next_weak_pos = 0;
    bool begin = true, end = false;
    WPath& w0 = s.wp[RTK_WP_REGION];
    rtk_wp_start(c, w0, start_um, rtk_get_qual(1.0, 0, static_cast<uint64_t>(c.o.max_qual)));
    uint64_t cur = rtk_wp_commit(s, w0, RTK_ARENA_REGION); uint32_t cur_pos = start_pos; bool have = true;
    const uint32_t nw = lvw_hi - lvw_lo; // weak anchors of the region are lvw[lvw_lo + i], i in [0, nw)
    if (i_weak < nw) i_weak = rtk_an_first_ge(lvw, lvw_lo + i_weak, lvw_lo + nw, start_pos) - lvw_lo; // the reference's forward walks over the weak anchors, as searches
    if (i_weak < nw) { const uint32_t wp = rtk_u(rtk_an_pos(lvw, lvw_lo + i_weak)); next_weak_pos = wp > start_pos + k ? wp : start_pos + k; }
    while (have && !end && !rtk_failed(s)) {
        if (i_weak < nw) { const uint64_t lim_a = static_cast<uint64_t>(pos2 - k), lim_b = next_weak_pos; i_weak = rtk_an_first_ge(lvw, lvw_lo + i_weak, lvw_lo + nw, lim_a < lim_b ? lim_a : lim_b) - lvw_lo; }
        else i_weak = nw;
        end = (i_weak == nw) || (static_cast<uint64_t>(rtk_u(rtk_an_pos(lvw, lvw_lo + i_weak))) >= static_cast<uint64_t>(pos2 - k));
        const uint32_t target_pos = end ? pos2 : rtk_u(rtk_an_pos(lvw, lvw_lo + i_weak));
        const uint32_t l_len = (target_pos - cur_pos) + k;
        const UMap um_start = begin ? start_um : rtk_rec_back(s, cur);
        uint64_t res = ~0ull; bool called = false;
        { // one call site for the three cases: to the end of the read (:61-72), to the right solid anchor (:74-78), to the next weak anchor (:110-114)
            UMap um_to = rtk_um_empty(); bool with_end = false;
            if (end) { if (no_end) called = l_len <= (max_len_weak_region / 2); else { called = l_len <= max_len_weak_region; um_to = end_um; with_end = true; } }
            else if (l_len <= max_len_weak_region) { called = true; um_to = rtk_u(rtk_an_um(lvw, lvw_lo + i_weak)); with_end = true; }
            RTK_PL(s, RTK_LAP_SEMIWEAK_GLUE);
            if (called) res = rtk_explore_paths(c, all_pids, n_all, s_read + cur_pos, l_len, um_start, um_to, with_end);
        }
        if (rtk_failed(s)) break;
        if (called && res != ~0ull) {
            rtk_wp_load(s, w0, cur); rtk_wp_merge(c, w0, res);
            cur = rtk_wp_commit(s, w0, RTK_ARENA_REGION); cur_pos = target_pos;
        } else {
            if (*n_partial >= s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); break; }
            s.list[RTK_L_PARTIAL][(*n_partial)++] = cur; have = false;
        }
        if (!end) next_weak_pos = rtk_u(rtk_an_pos(lvw, lvw_lo + i_weak)) + k;
        begin = false;
    }
    RTK_PL(s, RTK_LAP_SEMIWEAK_MERGE);
    return (have && !rtk_failed(s)) ? cur : ~0ull;
}

#endif
