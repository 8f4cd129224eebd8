// Region stage of the per-read correction on the device: one wavefront owns one weak region of one long read
// (reference: src/Correction.cpp:159-958 correctSequence and its `correct` lambda :431-753). This file is the region program itself: the
// `correct` lambda (rtk_correct_region), the rule that spares a gap region its second strand, and the driver rtk_region_program. What they
// call is in the headers it includes, in the order of the program; the names of the work buffers, and who owns which when, are in rtk_region_types.h.
//
// The program is wave-uniform: every lane executes the same control flow on the same values; the lanes split up
// only inside the bulk primitives (2-bit decode of unitig substrings, bit-parallel Myers with one query word per
// lane, sorted-set algebra with __ballot compaction, copies). Paths live as immutable records in per-wave bump
// arenas in HBM (three nesting levels: region / BFS call / DFS call); the reference's queue, stack and candidate
// vectors become small handle lists. Canonical tie rules [D1] (see oracle/oracle_correct.hpp) are applied where the
// reference depends on heap addresses. Index annotations that our index producer never emits (short cycles, SNP
// ambiguities) are handled by rtk_fix_repeats and rtk_ambiguity.h.
#ifndef RTK_REGION_H
#define RTK_REGION_H

#include "rtk_region_types.h"
#include "rtk_region_paths.h"
#include "rtk_sim_census.h"
#include "rtk_region_align.h"
#include "rtk_ambiguity.h"
#include "rtk_region_search.h"
#include "rtk_colours.h"
#include "rtk_region_result.h"
#include "rtk_consensus.h"

// Bifrost Kmer(const char*) 2-bit code of any character (end k-mer test, src/Correction.cpp:720-724)
RTK_DEV int rtk_bifrost_code(char ch) { const int x = (ch & 4) >> 1; return x + ((x ^ (ch & 2)) >> 1); }

// Visits anchors x = start, start+step, ... while `in_range(pos)` holds (positions are sorted, so the condition is a prefix
// property), calling fn(um) once per RUN of consecutive anchors on the same unitig. Repeated visits of one unitig are no-ops for
// the side lists (first insertion wins, the branching quota only grows), so skipping them is exact. Lanes fetch 64 anchors at a time.
template <class Cond, class Fn>
RTK_DEV void rtk_scan_anchor_runs(const Anchors& a, int64_t start, int step, Cond in_range, Fn fn) {
    uint32_t prev_unitig = RTK_NONE32; bool first = true;
    for (int64_t b = 0;; b += RTK_WAVE) {
        const int64_t x = start + static_cast<int64_t>(step) * (b + rtk_lane());
        bool ok = false; UMap um = rtk_um_empty();
        if (x >= 0 && x < static_cast<int64_t>(a.n)) { ok = in_range(rtk_an_pos(a, static_cast<uint32_t>(x))); if (ok) um = rtk_an_um(a, static_cast<uint32_t>(x)); }
        const uint64_t okm = rtk_ballot(ok);
        const int lead = (~okm == 0ull) ? RTK_WAVE : (rtk_ffs(~okm) - 1); // anchors of this chunk that are visited
        if (lead == 0) break;
        uint32_t left_unitig = rtk_shfl_up1(um.unitig, prev_unitig);
        const bool run_start = ok && rtk_lane() < lead && (um.unitig != left_unitig || (first && rtk_lane() == 0));
        uint64_t rs = rtk_ballot(run_start);
        while (rs) {
            const int l = rtk_ffs(rs) - 1; rs &= rs - 1ull;
            UMap u; u.unitig = rtk_shfl(um.unitig, l); u.dist = rtk_shfl(um.dist, l); u.len = 1; u.strand = rtk_shfl(um.strand, l);
            fn(u);
        }
        prev_unitig = rtk_shfl(um.unitig, lead - 1); first = false;
        if (lead < RTK_WAVE) break;
    }
}

// ------------------------------------------------------------------------------------------------ the `correct` lambda (src/Correction.cpp:431-753)
// s_read: read in the orientation of this call; v_s / v_w: anchors in that orientation. Result strings go to res.seq / res.qual.
// q_read: pass 2 only, the quality string that goes with s_read in this call (the reference passes q_fw, q_bw or -- for the head region --
// q_fw next to the reverse-complemented read, :787 G17); uncorrected stretches keep their qualities instead of getting q_min.

// park: the trim's sweep is stored and the consensus's forward alignment walked from it (rtk_trim_by_column): the forward strand of a gap region
RTK_FN_REGION void rtk_correct_region(const RCtx& c_, const char* s_read_, uint32_t s_len_, const Anchors& v_s_, const Anchors& v_w_, uint32_t i_s_, uint32_t i_w_, const ResCorr* rc_, ResCorr& res_, const char* q_read_ = nullptr, bool park_ = false) {
    const RCtx& c = *rtk_u(&c_); const char* s_read = rtk_u(s_read_); const char* q_read = rtk_u(q_read_); const bool park = rtk_u(park_);
    const bool lrc = rtk_u(c.o.long_read_correct) != 0 && q_read != nullptr; uint32_t s_len = rtk_u(s_len_); const Anchors& v_s = *rtk_u(&v_s_); const Anchors& v_w = *rtk_u(&v_w_); RTK_ASSUME_LDS(&v_s); RTK_ASSUME_LDS(&v_w); uint32_t i_s = rtk_u(i_s_); uint32_t i_w = rtk_u(i_w_); const ResCorr* rc = rtk_u(rc_); ResCorr& res = *rtk_u(&res_); RTK_ASSUME_LDS(&res);
    RegionScratch& s = rtk_hdr(c);
    const uint32_t k = static_cast<uint32_t>(c.k);
    const GraphView& g = c.g;
    const bool has_end_pt = (i_s + 1) < v_s.n;
    // (values that live across the calls below are made scalar on purpose: a wave-uniform value in a vector register costs a 256-byte row
    // every time it is saved around a call, in a scalar register it is one lane of a spill register)
    uint32_t p1 = rtk_u(rtk_an_pos(v_s, i_s)); UMap um1 = rtk_u(rtk_an_um(v_s, i_s));
    const uint32_t p2 = rtk_u(has_end_pt ? rtk_an_pos(v_s, i_s + 1) : (s_len - k));
    const UMap um2 = rtk_u(has_end_pt ? rtk_an_um(v_s, i_s + 1) : rtk_um_empty());
    const uint32_t first_pos = p1;
    uint32_t len_weak_region = p2 - p1 + k;
    const uint64_t u_min_start = static_cast<uint64_t>(p1) - static_cast<uint64_t>(c.o.insert_sz); // wraps below insert_sz (G1)
    const uint64_t u_min_end = static_cast<uint64_t>(p2) + static_cast<uint64_t>(c.o.insert_sz);
    res.old_len = len_weak_region; res.is_corrected = false; res.seq_len = 0; res.qual_len = 0; res.n_all = 0;
    if ((len_weak_region + 63) / 64 + 1 > s.bm_words) { rtk_fail_ovf(s, RTK_OVF_BITMAP); return; }
    for (uint32_t w = static_cast<uint32_t>(rtk_lane()); w < (len_weak_region + 63) / 64 + 1; w += RTK_WAVE) res.bm[w] = 0;
    rtk_sync();
    const char q_min = rtk_get_qual(0.0, 0, static_cast<uint64_t>(c.o.max_qual));
    const uint32_t max_len_weak_anchors = c.o.long_read_correct ? c.o.max_len_weak_region2 : c.o.max_len_weak_region1; // :177
    // weak anchors inside the region: l_v_w = v_w[lw_lo .. lw_hi)
    uint32_t lw_lo = 0, lw_hi = 0;
    {
        const uint32_t v_w_sz = v_w.n;
        if (v_w_sz) {
            const uint32_t pos_end = has_end_pt ? p2 : s_len;
            const uint32_t x = i_w - (((i_w != 0) && (i_w >= v_w_sz)) ? 1u : 0u);
            lw_lo = rtk_u(rtk_an_first_ge(v_w, x, v_w_sz, first_pos));
            lw_hi = rtk_u(rtk_an_first_ge(v_w, lw_lo, v_w_sz, pos_end));
        }
    }
    uint32_t n_all = 0;
    RTK_PL(s, RTK_LAP_REGION_PROLOGUE);
    if (rc == nullptr) {
        const unsigned long long t_side0 = rtk_clock();
        // side lists live in list[RTK_L_SIDE_*] memory (u32 unitig + flag bytes)
        SideList& sl = s.loc.side[RTK_SIDE_LEFT]; SideList& sr = s.loc.side[RTK_SIDE_RIGHT]; SideList& sm = s.loc.side[RTK_SIDE_MIDDLE];
        const uint32_t cap = s.list_cap;
        sl.u = reinterpret_cast<uint32_t*>(s.list[RTK_L_SIDE_LEFT].get()); sl.nb = reinterpret_cast<uint8_t*>(s.list[RTK_L_SIDE_LEFT].get() + cap / 2); sl.n = 0; sl.cap = cap;
        sr.u = reinterpret_cast<uint32_t*>(s.list[RTK_L_SIDE_RIGHT].get()); sr.nb = reinterpret_cast<uint8_t*>(s.list[RTK_L_SIDE_RIGHT].get() + cap / 2); sr.n = 0; sr.cap = cap;
        sm.u = reinterpret_cast<uint32_t*>(s.list[RTK_L_SIDE_MIDDLE].get()); sm.nb = reinterpret_cast<uint8_t*>(s.list[RTK_L_SIDE_MIDDLE].get() + cap / 2); sm.n = 0; sm.cap = cap;
        auto consider = [&](SideList& m, const UMap& um, uint32_t& nb_branching) {
            const uint32_t u = um.unitig; const bool br = rtk_is_branching(g, u);
            if (g.kcov[u] < c.o.max_km_cov && (!br || nb_branching < 5)) { const bool unseen = rtk_side_insert(m, u, !br); nb_branching += (unseen && br) ? 1u : 0u; }
        };
        { // left (:476-516)
            uint32_t nbb = 0;
            rtk_scan_anchor_runs(v_s, static_cast<int64_t>(i_s), -1, [&](uint32_t p) { return static_cast<uint64_t>(p) > u_min_start; }, [&](const UMap& um) { consider(sl, um, nbb); });
            const uint32_t v_w_sz = v_w.n;
            if (v_w_sz) {
                const uint32_t x0 = i_w - (((i_w != 0) && (i_w >= v_w_sz)) ? 1u : 0u);
                // the reference walks back while pos > u_min_start and index > 0: it lands on the last anchor at or below u_min_start (or on 0)
                const uint32_t f = rtk_an_first_gt(v_w, 0, x0 + 1, u_min_start);
                const uint32_t x = f > 0 ? f - 1 : 0;
                rtk_scan_anchor_runs(v_w, static_cast<int64_t>(x), +1, [&](uint32_t p) { return p < first_pos; }, [&](const UMap& um) { consider(sl, um, nbb); });
            }
        }
        if (has_end_pt) { // right (:518-561)
            uint32_t nbb = 0;
            rtk_scan_anchor_runs(v_s, static_cast<int64_t>(i_s) + 1, +1, [&](uint32_t p) { return static_cast<uint64_t>(p) < u_min_end; }, [&](const UMap& um) { consider(sr, um, nbb); });
            const uint32_t v_w_sz = v_w.n;
            if (v_w_sz) {
                const uint32_t x0 = i_w - (((i_w != 0) && (i_w >= v_w_sz)) ? 1u : 0u);
                const uint32_t x = rtk_an_first_ge(v_w, x0, v_w_sz, p2);
                rtk_scan_anchor_runs(v_w, static_cast<int64_t>(x), +1, [&](uint32_t p) { return static_cast<uint64_t>(p) < u_min_end; }, [&](const UMap& um) { consider(sr, um, nbb); });
            }
        }
        if (lw_hi > lw_lo) { // middle (:563-585)
            const uint32_t pos_end_m = has_end_pt ? p2 : s_len;
            rtk_scan_anchor_runs(v_w, static_cast<int64_t>(lw_lo), +1, [&](uint32_t p) { return p < pos_end_m; }, [&](const UMap& um) { const uint32_t u = um.unitig; if (g.kcov[u] < c.o.max_km_cov) rtk_side_insert(sm, u, !rtk_is_branching(g, u)); });
        }
        if (sl.n >= cap / 2 || sr.n >= cap / 2 || sm.n >= cap / 2) { rtk_fail_ovf(s, RTK_OVF_LIST); return; }
        s.fine[RTK_FINE_SIDE_LISTS] += rtk_clock() - t_side0;
        RTK_PL(s, RTK_LAP_REGION_SIDE_LISTS);
        { const unsigned long long t0 = rtk_clock(); n_all = rtk_u(rtk_choose_colors(c, sl, sr, sm)); s.cnt[RTK_RC_CYC_COLOUR] += rtk_clock() - t0; }
        RTK_PL(s, RTK_LAP_REGION_COLOURS);
        if (rtk_failed(s)) return;
        // keep all_pids for the reverse-complement call (rc = &fw): set[RTK_SET_ALL_PIDS] is preserved by everything below (hand-over H5, rtk_region_types.h)
    } else n_all = rtk_u(rc->n_all);
    res.n_all = n_all;
    const uint32_t* all_pids = s.set[RTK_SET_ALL_PIDS];
    // ---- paths ---- (from here on list[0 .. 5] belong to the path search: hand-over H4)
    s.top[RTK_ARENA_REGION] = 0;
    uint32_t n_partial = 0, n_amb = 0; // n_amb: size of v_ambiguity (list[RTK_L_AMB])
    uint64_t complete = ~0ull;
    char* s_corr = res.seq; char* q_corr = res.qual; uint32_t& sl_ = s.loc.len[RTK_LEN_CORR_SEQ]; uint32_t& ql_ = s.loc.len[RTK_LEN_CORR_QUAL]; sl_ = 0; ql_ = 0; // (lengths that rtk_app updates through a pointer: LDS words)
    const Anchors& lvw = v_w;
    const uint32_t nlw = lw_hi - lw_lo;
    auto clamp_len = [&](uint32_t pos, uint32_t len) -> uint32_t { return (pos + len <= s_len) ? len : (pos < s_len ? s_len - pos : 0); }; // std::string::substr
    auto add_uncorrected = [&](uint32_t pos, uint32_t len, char q) { rtk_app(s, s_corr, &sl_, s_read + pos, clamp_len(pos, len));
        if (lrc) rtk_app(s, q_corr, &ql_, q_read + pos, clamp_len(pos, len)); else rtk_app_fill(s, q_corr, &ql_, q, len_weak_region); }; // :459-469
    // extractSemiWeakPaths from the left solid anchor (:613), then again from a weak anchor behind the best partial path as long as
    // there is one (:619-651): ONE call site, so that the whole search can be compiled into this function
    bool first_call = true, found_first = false, do_call = n_all >= c.o.min_cov_vertices;
    uint32_t i_w_s = 0;
    for (;;) {
        if (do_call) { const unsigned long long t0 = rtk_clock(); complete = rtk_u(rtk_extract_semi_weak(c, s_read, s_len, all_pids, n_all, p1, um1, p2, um2, lvw, lw_lo, lw_hi, first_call ? 0u : i_w_s, &n_partial)); n_partial = rtk_u(n_partial); s.cnt[RTK_RC_CYC_PATHS] += rtk_clock() - t0; }
        if (rtk_failed(s)) return;
        RTK_PL(s, RTK_LAP_SEMIWEAK_MERGE);
        if (first_call && complete != ~0ull) found_first = true;
        first_call = false;
        if (!(complete == ~0ull && n_partial != 0 && nlw != 0 && n_all >= c.o.min_cov_vertices)) break;
        { // :619-651
            int& aid = s.loc.best[RTK_BEST_ID]; int& aend = s.loc.best[RTK_BEST_END];
            RTK_SITE(RTK_SITE_SELECT_PARTIAL_RETRY); rtk_select_best(c, s.list[RTK_L_PARTIAL], n_partial, s_read + p1, len_weak_region, RTK_MODE_SHW, c.o.weak_region_len_factor, &aid, &aend);
            if (rtk_failed(s) || aid == -1) break;
            {
                const uint32_t next_pos = p1 + static_cast<uint32_t>(aend) + k;
                while (i_w_s < nlw && rtk_an_pos(lvw, lw_lo + i_w_s) < next_pos) ++i_w_s;
                if (i_w_s >= nlw || static_cast<uint64_t>(rtk_an_pos(lvw, lw_lo + i_w_s)) >= static_cast<uint64_t>(p2) - k || (rtk_an_pos(lvw, lw_lo + i_w_s) - p1) >= max_len_weak_anchors) break;
            }
            const uint64_t hb = rtk_u(s.list[RTK_L_PARTIAL][aid]);
            const uint32_t wpos = rtk_u(rtk_an_pos(lvw, lw_lo + i_w_s));
            const uint32_t pl = rtk_rec_to_string(c, hb, s.str[RTK_STR_CAND]); if (pl == 0xFFFFFFFFu) break;
            n_amb = rtk_amb_collect(c, hb, sl_, n_amb);
            rtk_app(s, s_corr, &sl_, s.str[RTK_STR_CAND], pl);
            rtk_app(s, s_corr, &sl_, s_read + p1 + aend + 1, wpos - p1 - static_cast<uint32_t>(aend) - 1);
            rtk_app(s, q_corr, &ql_, rtk_path_qual(s, rtk_h_lvl(hb), rtk_h_off(hb)), rtk_path_hdr(s, rtk_h_lvl(hb), rtk_h_off(hb))->qlen);
            if (lrc) rtk_app(s, q_corr, &ql_, q_read + p1 + aend + 1, clamp_len(p1 + static_cast<uint32_t>(aend) + 1, wpos - p1 - static_cast<uint32_t>(aend) - 1)); // :642
            else rtk_app_fill(s, q_corr, &ql_, q_min, wpos - p1 - static_cast<uint32_t>(aend) - 1);
            rtk_bm_add_range(res.bm, p1 - first_pos, p1 + static_cast<uint32_t>(aend) + 1 - first_pos);
            p1 = wpos; um1 = rtk_u(rtk_an_um(lvw, lw_lo + i_w_s));
            len_weak_region = p2 - p1 + k;
            s.top[RTK_ARENA_REGION] = 0; n_partial = 0; // paths of the previous attempt are dead
            do_call = true;
        }
    }
    if (rtk_failed(s)) return;
    RTK_PL(s, RTK_LAP_REGION_RESTART);
    if (!found_first) {
        if (complete != ~0ull) {
            const uint32_t pl = rtk_rec_to_string(c, complete, s.str[RTK_STR_CAND]); if (pl == 0xFFFFFFFFu) return;
            n_amb = rtk_amb_collect(c, complete, sl_, n_amb);
            rtk_app(s, s_corr, &sl_, s.str[RTK_STR_CAND], pl);
            rtk_app(s, q_corr, &ql_, rtk_path_qual(s, rtk_h_lvl(complete), rtk_h_off(complete)), rtk_path_hdr(s, rtk_h_lvl(complete), rtk_h_off(complete))->qlen);
            rtk_bm_add_range(res.bm, p1 - first_pos, p2 - first_pos + k);
        } else if (n_partial != 0) {
            int& aid = s.loc.best[RTK_BEST_ID]; int& aend = s.loc.best[RTK_BEST_END];
            RTK_SITE(RTK_SITE_SELECT_PARTIAL); rtk_select_best(c, s.list[RTK_L_PARTIAL], n_partial, s_read + p1, len_weak_region, RTK_MODE_SHW, c.o.weak_region_len_factor, &aid, &aend);
            if (rtk_failed(s)) return;
            if (aid == -1) add_uncorrected(p1, len_weak_region, q_min);
            else {
                const uint64_t hb = s.list[RTK_L_PARTIAL][aid];
                const uint32_t pl = rtk_rec_to_string(c, hb, s.str[RTK_STR_CAND]); if (pl == 0xFFFFFFFFu) return;
                n_amb = rtk_amb_collect(c, hb, sl_, n_amb);
                rtk_app(s, s_corr, &sl_, s.str[RTK_STR_CAND], pl);
                const uint32_t rest = len_weak_region - static_cast<uint32_t>(aend) - 1;
                rtk_app(s, s_corr, &sl_, s_read + p1 + aend + 1, rest);
                rtk_app(s, q_corr, &ql_, rtk_path_qual(s, rtk_h_lvl(hb), rtk_h_off(hb)), rtk_path_hdr(s, rtk_h_lvl(hb), rtk_h_off(hb))->qlen);
                if (lrc) rtk_app(s, q_corr, &ql_, q_read + p1 + aend + 1, clamp_len(p1 + static_cast<uint32_t>(aend) + 1, rest)); // :684
                else rtk_app_fill(s, q_corr, &ql_, q_min, rest);
                rtk_bm_add_range(res.bm, p1 - first_pos, p1 + static_cast<uint32_t>(aend) + 1 - first_pos);
            }
        } else if (sl_ != 0) add_uncorrected(p1, len_weak_region, q_min);
        else { sl_ = 0; ql_ = 0; add_uncorrected(first_pos, len_weak_region, q_min); } // setUncorrected
    } else {
        const uint32_t pl = rtk_rec_to_string(c, complete, s.str[RTK_STR_CAND]); if (pl == 0xFFFFFFFFu) return;
        sl_ = 0; ql_ = 0;
        n_amb = rtk_amb_collect(c, complete, 0, n_amb);
        rtk_app(s, s_corr, &sl_, s.str[RTK_STR_CAND], pl);
        rtk_app(s, q_corr, &ql_, rtk_path_qual(s, rtk_h_lvl(complete), rtk_h_off(complete)), rtk_path_hdr(s, rtk_h_lvl(complete), rtk_h_off(complete))->qlen);
        rtk_bm_add_range(res.bm, 0, len_weak_region);
    }
    if (rtk_failed(s)) return;
    RTK_PL(s, RTK_LAP_REGION_ASSEMBLE);
    if (n_amb != 0) { const unsigned long long ta0 = rtk_clock(); rtk_fix_ambiguity(c, s_corr, sl_, q_corr, ql_, s_read + first_pos, res.old_len, n_amb); s.fine[RTK_FINE_FIX_AMBIGUITY] += rtk_clock() - ta0; if (rtk_failed(s)) return; } // :716
    RTK_PL(s, RTK_LAP_REGION_FIX_AMBIGUITY);
    if (rtk_bm_card(res.bm, res.old_len) == res.old_len) { // :718-725 (G20): last k-mer of the WHOLE read vs last k-mer of the corrected region
        bool same = sl_ >= k && s_len >= k;
        for (uint32_t i = 0; same && i < k; ++i) same = rtk_bifrost_code(s_read[s_len - k + i]) == rtk_bifrost_code(s_corr[sl_ - k + i]);
        if (same) res.is_corrected = true;
    }
    if (!res.is_corrected) { // :727-747 trim the corrected string to the largest SHW end location of the raw region
        const unsigned long long tt0 = rtk_clock();
        MyersResult& a = s.loc.trim;
        if (!rtk_trim_by_column(c, s_read + first_pos, p2 - first_pos + k, s_corr, sl_, park, &a)) {
            s.cnt[RTK_RC_TRIM_FALLBACK] += 1;
            RTK_SITE(RTK_SITE_TRIM_FALLBACK); a = rtk_align(c, s_read + first_pos, p2 - first_pos + k, s_corr, sl_, -1, RTK_MODE_SHW);
        }
        s.fine[RTK_FINE_TRIM] += rtk_clock() - tt0;
        if (a.dist >= 0) {
            const uint32_t keep = (a.first == -1) ? 0u : static_cast<uint32_t>(a.last + 1); // endLocations[0] == -1 wraps to SIZE_MAX in the reference
            if (keep < sl_) sl_ = keep;
            if (keep < ql_) ql_ = keep;
        }
    }
    res.seq_len = sl_; res.qual_len = ql_;
    RTK_PL(s, RTK_LAP_REGION_TRIM);
}

// ------------------------------------------------------------------------------------------------ region driver (src/Correction.cpp:776-957)
RTK_FN void rtk_emit_segment(const RCtx& c_, RegionDesc* rd_, const char* sq_, uint32_t sl_, const char* ql_, uint32_t qll_) {
    const RCtx& c = *rtk_u(&c_); RegionDesc* rd = rtk_u(rd_); const char* sq = rtk_u(sq_); uint32_t sl = rtk_u(sl_); const char* ql = rtk_u(ql_); uint32_t qll = rtk_u(qll_);
    unsigned long long off = 0;
    if (rtk_lane() == 0) off = rtk_atomic_add(c.rb.seg_top, static_cast<unsigned long long>(sl) + qll);
    off = rtk_shfl(off, 0);
    if (off + sl + qll > c.rb.seg_cap) { rtk_fail_ovf(*c.sc, RTK_OVF_SEG_POOL); return; }
    rtk_wcopy(c.rb.seg_pool + off, sq, sl);
    rtk_wcopy(c.rb.seg_pool + off + sl, ql, qll);
    rd->seg_off = off; rd->seq_len = sl; rd->qual_len = qll;
}

// ------------------------------------------------------------------------------------------------ the second strand of a gap region
// A gap region that its forward strand does not settle alone (is_corrected, G20) is corrected again on the reverse complement, and the two results are merged
// by rtk_generate_consensus. When the forward strand corrected every old position, the second strand can change the emitted bytes in two ways only: by coming
// back is_corrected, or through one of the exits of the consensus that do not take the forward strings. rtk_strand2_skippable decides from the forward
// result, the read and the graph that neither can happen; the region then emits the forward strings and runs neither the second strand nor the consensus.
//
// Lane-local. A corrected string of the second strand with a full bitmap ends in the graph k-mer behind one of the read's anchors (proof: DESIGN.md). Could
// that be the anchor with mapping `um` (in the FORWARD read's orientation), and the string then pass the end test of rtk_correct_region, which compares it
// with f = the forward read's first k-mer (A C G T only) reverse-complemented? false: surely not -- the two k-mers differ in a character that no annotation
// can have rewritten. true: cannot be excluded.
// Which characters of the k-mer fixAmbiguity can rewrite: those that an annotation of a unitig of the path covers (rtk_amb_collect). These are the unitig's
// own annotations and, in the k - 1 characters that two consecutive unitigs of a path share, the neighbour's. The second strand's path reaches the k-mer
// from the side that lies behind the anchor in the forward read, through `beyond` further k-mers of the unitig: a neighbour N on that side shares its first
// k - 1 characters with the unitig's last, which are the k-mer's characters from beyond + 1 on; and where N holds fewer k-mers than that leaves uncovered, the
// unitig before N reaches the k-mer too, and every character from there on counts as rewritable.
RTK_DEV uint64_t rtk_strand2_amb_mask(const GraphView& g, uint32_t u, uint32_t lo, uint32_t n, bool fwd, uint32_t first_bit, uint32_t k) {
    // bit first_bit + x for every annotation of unitig u at character lo + x (fwd) / lo + n - 1 - x (!fwd), x in [0, n), that falls below bit k
    const uint64_t* ent = g.amb.get() + (static_cast<uint64_t>(g.n_unitigs) + 1);
    uint64_t m = 0;
    for (uint64_t e = g.amb[u]; e < g.amb[u + 1]; ++e) {
        const uint32_t pos = static_cast<uint32_t>(ent[e] >> 4);
        if (pos < lo || pos >= lo + n) continue;
        const uint32_t bit = first_bit + (fwd ? (pos - lo) : (lo + n - 1u - pos));
        if (bit < k) m |= 1ull << bit;
    }
    return m;
}
RTK_DEV bool rtk_strand2_end_may_match(const RCtx& c, const UMap& um, const char* f) {
    const GraphView& g = c.g; const uint32_t k = static_cast<uint32_t>(c.k); // k <= 63: one bit per character of the k-mer, in the forward read's orientation
    uint64_t soft = 0; // characters that may have been rewritten
    if (g.n_amb != 0) {
        soft = rtk_strand2_amb_mask(g, um.unitig, um.dist, k, um.strand != 0, 0, k);
        const uint32_t beyond = um.strand ? (rtk_nkm(g, um.unitig) - 1u - um.dist) : um.dist;
        if (beyond < k - 1u) {
            const uint32_t* adj = g.adj.get() + 8ull * um.unitig + (um.strand ? 0 : 4);
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t nb = adj[b];
                if (nb == RTK_NONE32) continue;
                const uint32_t v = nb >> 1, ul = rtk_ulen(g, v), nkm = ul - k + 1u;
                const uint32_t shared = (k - 1u) < ul ? (k - 1u) : ul;
                soft |= rtk_strand2_amb_mask(g, v, (nb & 1u) ? 0u : (ul - shared), shared, (nb & 1u) != 0, beyond + 1u, k);
                if (beyond + 1u + nkm < k) soft |= ~0ull << (beyond + 1u + nkm);
            }
        }
    }
    for (uint32_t j = 0; j < k; ++j) {
        if ((soft >> j) & 1ull) continue;
        const char uc = rtk_unitig_char(g, um.unitig, um.strand ? (um.dist + j) : (um.dist + k - 1u - j));
        if ((um.strand ? uc : rtk_comp(uc)) != f[j]) return false;
    }
    return true;
}

// Wave-uniform. fw: the forward result of gap region [pa, pb + k) of read s_fw, made with park = true and not is_corrected; so, i: the read's solid anchors and
// the index of the one at pa; we, i_weak: the read's weak anchors and the first one at or after pa. (Anchors and indices, not the mappings: a UMap handed on by
// reference would have to live on the caller's stack.) The conditions R1 .. R5 are those of DESIGN.md §3.2 (f).
RTK_FN bool rtk_strand2_skippable(const RCtx& c_, const ResCorr& fw_, const char* s_fw_, uint32_t pa_, uint32_t pb_, const Anchors& so_, uint32_t i_, const Anchors& we_, uint32_t i_weak_) {
    const RCtx& c = *rtk_u(&c_); const ResCorr& fw = *rtk_u(&fw_); RTK_ASSUME_LDS(&fw); const char* s_fw = rtk_u(s_fw_); const uint32_t pa = rtk_u(pa_), pb = rtk_u(pb_);
    const Anchors& so = *rtk_u(&so_); RTK_ASSUME_LDS(&so); const uint32_t i = rtk_u(i_); const Anchors& we = *rtk_u(&we_); RTK_ASSUME_LDS(&we); const uint32_t i_weak = rtk_u(i_weak_);
    RegionScratch& s = rtk_hdr(c);
    const uint32_t k = static_cast<uint32_t>(c.k), ref_len = pb - pa + k;
    const uint32_t fsl = rtk_u(fw.seq_len), fql = rtk_u(fw.qual_len);
    // R1: every old position corrected -- the consensus does not swap the strands and its merge is one forward step over the whole raw region
    if (rtk_bm_card(fw.bm, fw.old_len) != fw.old_len || fw.old_len != ref_len) return false;
    // R2: the forward trim parked the alignment of exactly this string (what `parked()` of the consensus asks); the merge then copies fw.qual up to fw.seq_len
    const TrimPark pk = s.loc.park;
    if ((pk.nm == 0 && !pk.pending) || fsl == 0 || pk.len != fsl || fql > fsl) return false; // (a pending park stands for nm != 0: its walk makes at least one move)
    // R3: the forward string passes the norm test of the consensus (the same doubles)
    const double max_norm = c.o.weak_region_len_factor;
    if (max_norm > 0.0 && static_cast<double>(pk.dist) / static_cast<double>(fsl > ref_len ? fsl : ref_len) > max_norm) return false;
    // R4: the parked moves do not end in an insert (the merge stops at the end of the raw region and would leave trailing inserted characters out); the last
    // move is known from the trim, whether the path has been walked or not
    if (pk.last_move == 1u) return false;
    // R5: the second strand cannot come back is_corrected. Its fixAmbiguity rewrites annotated positions only when the raw region is plain, and the end test
    // is a comparison of characters when the read's first k-mer is.
    if (!rtk_all_acgt(s_fw, k) || !rtk_all_acgt(s_fw + pa, ref_len)) return false;
    if (rtk_strand2_end_may_match(c, rtk_u(rtk_an_um(so, i)), s_fw) || rtk_strand2_end_may_match(c, rtk_u(rtk_an_um(so, i + 1)), s_fw)) return false;
    const uint32_t w_hi = rtk_u(rtk_an_first_gt(we, i_weak, we.n, pb)); // the weak anchors of the second strand's region lie in (pa, pb]
    for (uint32_t x0 = i_weak; x0 < w_hi; x0 += RTK_WAVE) {
        const uint32_t x = x0 + static_cast<uint32_t>(rtk_lane());
        const bool may = x < w_hi && rtk_strand2_end_may_match(c, rtk_an_um(we, x), s_fw);
        if (rtk_ballot(may) != 0ull) return false;
    }
    return true;
}

RTK_FN_DRIVER void rtk_region_program(const RCtx& c_, RegionDesc* rd_) {
    const RCtx& c = *rtk_u(&c_); RegionDesc* rd = rtk_u(rd_);
    RegionScratch& s = rtk_hdr(c);
    s.loc.park.nm = 0; s.loc.park.pending = 0; // nothing parked for this region yet
    const uint32_t r = rtk_u(rd->read), k = static_cast<uint32_t>(c.k);
    const uint64_t base = rtk_u(c.bv.roff[r]);
    const uint32_t L = rtk_u(static_cast<uint32_t>(c.bv.roff[r + 1] - base));
    const char* s_fw = c.bv.seq + base; const char* s_bw = c.rb.seq_rc + base;
    const char q_min = rtk_get_qual(0.0, 0, static_cast<uint64_t>(c.o.max_qual)), q_max = rtk_get_qual(1.0, 0, static_cast<uint64_t>(c.o.max_qual));
    char* out_s = s.rbuf[RTK_RB_OUT_SEQ]; char* out_q = s.rbuf[RTK_RB_OUT_QUAL]; uint32_t& osl = s.loc.len[RTK_LEN_OUT_SEQ]; uint32_t& oql = s.loc.len[RTK_LEN_OUT_QUAL]; osl = 0; oql = 0;
    Anchors& so = s.loc.an[RTK_AN_SOLID]; Anchors& we = s.loc.an[RTK_AN_WEAK]; Anchors& so_r = s.loc.an[RTK_AN_SOLID_RC]; Anchors& we_r = s.loc.an[RTK_AN_WEAK_RC];
    so.pos = c.bv.s_pos + base; so.hit = nullptr; so.hits_by_pos = c.bv.hits + base; so.n = c.bv.n_solid[r]; so.L = L; so.rev = 0; so.k = c.k;
    we.pos = c.bv.wk_pos + c.bv.w_off[r]; we.hit = c.bv.wk_hit + c.bv.w_off[r]; we.hits_by_pos = nullptr; we.n = c.bv.w_cnt[r]; we.L = L; we.rev = 0; we.k = c.k;
    so_r = so; so_r.rev = 1; we_r = we; we_r.rev = 1;
    rtk_sync();
    ResCorr& fw = s.loc.rc[RTK_RES_FW]; ResCorr& bw = s.loc.rc[RTK_RES_BW];
    fw.seq = s.rbuf[RTK_RB_FW_SEQ]; fw.qual = s.rbuf[RTK_RB_FW_QUAL]; fw.bm = s.bm[RTK_BM_FW]; bw.seq = s.rbuf[RTK_RB_BW_SEQ]; bw.qual = s.rbuf[RTK_RB_BW_QUAL]; bw.bm = s.bm[RTK_BM_BW];
    if (L + 64 > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return; }
    // pass 2 (long_read_correct): the read's own qualities are carried wherever pass 1 writes q_max / q_min, and a stretch whose bases all
    // have the maximum quality already is left alone (hasMinQual, src/Correction.hpp:45-52; :779, :808, :941)
    const bool lrc = c.o.long_read_correct != 0 && c.bv.qual.get() != nullptr;
    const char* q_fw = lrc ? c.bv.qual + base : nullptr; const char* q_bw = lrc ? c.rb.qual_rev + base : nullptr;
    auto has_min_qual = [&](uint32_t start, uint32_t end) -> bool {
        for (uint32_t i0 = start; i0 < end; i0 += RTK_WAVE) {
            const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
            bool bad = false;
            if (i < end) { const char ch = s_fw[i]; bad = (q_fw[i] < q_max) && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
            if (rtk_ballot(bad) != 0ull) return false;
        }
        return true;
    };
    auto app_q = [&](uint32_t pos, uint32_t n, char fill) { if (lrc) rtk_app(s, out_q, &oql, q_fw + pos, n); else rtk_app_fill(s, out_q, &oql, fill, n); }; // q_fw.substr(pos, n) | string(n, fill)
    const uint32_t kind = rtk_u(rd->kind);
    RTK_PL(s, RTK_LAP_DEQUEUE);
    if (kind == RTK_RG_WHOLE_MAX || kind == RTK_RG_WHOLE_MIN) { // :165-171
        rtk_app(s, out_s, &osl, s_fw, L); app_q(0, L, kind == RTK_RG_WHOLE_MAX ? q_max : q_min);
    } else if (kind == RTK_RG_HEAD) { // :776-797
        if (!lrc || !has_min_qual(0, so.pos[0] + k)) {
            const uint32_t i_solid_rev = so.n - 1;
            uint32_t i_weak_rev = we.n;
            i_weak_rev = rtk_an_first_gt(we_r, 0, i_weak_rev, rtk_an_pos(so_r, i_solid_rev)); // the reference steps back while the previous weak anchor lies after the solid one
            rtk_correct_region(c, s_bw, L, so_r, we_r, i_solid_rev, i_weak_rev, nullptr, bw, q_fw); // q_fw next to s_bw: as the reference writes it (:787, G17)
            if (rtk_failed(s)) return;
            rtk_rc_reverse_complement(s, bw, s.bm[RTK_BM_RC_TMP], s.rbuf[RTK_RB_RC_TMP]);
            rtk_app(s, out_s, &osl, bw.seq, bw.seq_len >= k ? bw.seq_len - k : bw.seq_len); // substr(0, length - k): wraps to "everything" below k
            rtk_app(s, out_q, &oql, bw.qual, bw.qual_len >= k ? bw.qual_len - k : bw.qual_len);
        } else { rtk_app(s, out_s, &osl, s_fw, so.pos[0]); app_q(0, so.pos[0], q_min); }
    } else if (kind == RTK_RG_GAP) { // :803-935
        const uint32_t i = rtk_u(rd->i_solid), prev_pos = rtk_u(rd->prev_pos);
        const uint32_t pa = rtk_u(so.pos[i]), pb = rtk_u(so.pos[i + 1]);
        const UMap ua = rtk_u(rtk_an_um(so, i)), ub = rtk_u(rtk_an_um(so, i + 1));
        const uint32_t i_weak = rtk_u(rtk_an_first_ge(we, 0, we.n, pa)); // first weak anchor at or after the left solid anchor (:801)
        bool isUncorrected = false;
        bool sameUnitig = (ua.unitig == ub.unitig) && (ua.strand == ub.strand);
        if (lrc && has_min_qual(pa, pb + k)) isUncorrected = true; // :808
        else if (sameUnitig && !(c.g.flags[ua.unitig] & RTK_F_SHORT_CYCLE)) { // same-unitig shortcut (:814-858)
            const uint32_t min_pos = ua.dist < ub.dist ? ua.dist : ub.dist, max_pos = ua.dist < ub.dist ? ub.dist : ua.dist;
            const uint32_t len_query_km = pb - pa, len_unitig_km = max_pos - min_pos;
            uint64_t mn, mx; rtk_min_max_len(len_unitig_km, c.o.weak_region_len_factor, &mn, &mx);
            sameUnitig = sameUnitig && ((ua.strand && (ua.dist < ub.dist)) || (!ua.strand && (ua.dist > ub.dist)));
            sameUnitig = sameUnitig && (len_query_km >= mn) && (len_query_km <= mx);
            RTK_PL(s, RTK_LAP_DRIVER_DISPATCH);
            if (sameUnitig) {
                UMap sub = ua; sub.dist = min_pos; sub.len = len_unitig_km + 1;
                const uint32_t sl = rtk_ums_to_string(c, &sub, 1, s.str[RTK_STR_CAND]); if (sl == 0xFFFFFFFFu) return;
                rtk_app(s, out_s, &osl, s_fw + prev_pos, pa - prev_pos);
                rtk_app(s, out_s, &osl, s.str[RTK_STR_CAND], sl >= k ? sl - k : sl);
                if (lrc) { // :847-853
                    const uint32_t buff = (sl >= 2 * k) ? k : (sl - k);
                    rtk_app(s, out_q, &oql, q_fw + prev_pos, pa - prev_pos + buff);
                    if (sl - buff - k > 0) rtk_app_fill(s, out_q, &oql, q_max, sl - buff - k);
                } else rtk_app_fill(s, out_q, &oql, q_max, (pa - prev_pos) + (sl - k));
                RTK_PL(s, RTK_LAP_DRIVER_SAME_UNITIG);
            } else isUncorrected = true;
        } else if (pb >= pa + k) {
            RTK_PL(s, RTK_LAP_DRIVER_DISPATCH);
            rtk_correct_region(c, s_fw, L, so, we, i, i_weak, nullptr, fw, q_fw, /*park=*/true);
            if (rtk_failed(s)) return;
            const uint32_t l_solid = pa - prev_pos;
            auto emit_minus_k = [&](const char* seq, uint32_t sl, const char* q, uint32_t ql) { // (prefix + x).substr(0, len - k)
                const uint32_t ts = l_solid + sl, tq = l_solid + ql;
                const uint32_t ks = ts >= k ? ts - k : ts, kq = tq >= k ? tq - k : tq;
                rtk_app(s, out_s, &osl, s_fw + prev_pos, ks < l_solid ? ks : l_solid); if (ks > l_solid) rtk_app(s, out_s, &osl, seq, ks - l_solid);
                app_q(prev_pos, kq < l_solid ? kq : l_solid, q_max); if (kq > l_solid) rtk_app(s, out_q, &oql, q, kq - l_solid);
            };
            // 0: the second strand is skipped where the forward result decides the bytes alone (rtk_strand2_skippable); 1: it always runs; 2: it runs there too, and
            // the full route's result is emitted and compared with the forward one (rtk_knobs.h: RTK_STRAND2_ALWAYS, RTK_STRAND2_AUDIT)
            const uint32_t s2_mode = rtk_u(c.o.strand2_mode);
            const bool skippable = !fw.is_corrected && s2_mode != 1u && rtk_strand2_skippable(c, fw, s_fw, pa, pb, so, i, we, i_weak);
            if (fw.is_corrected) emit_minus_k(fw.seq, fw.seq_len, fw.qual, fw.qual_len);
            else if (skippable && s2_mode == 0u) {
                s.cnt[RTK_RC_STRAND2_SKIPPED] += 1;
                s.cnt[RTK_RC_CONS_RESUMED] += 1; // the consensus of this region is decided from the stored sweep of the forward trim alone (R2 .. R4): counted as the call it replaces
                emit_minus_k(fw.seq, fw.seq_len, fw.qual, fw.qual_len);
            } else {
                s.cnt[skippable ? RTK_RC_STRAND2_SKIPPED : RTK_RC_STRAND2_RUN] += 1; // (the audit counts the rule's verdicts and runs both kinds)
                rtk_park_walk(c, fw.seq, s_fw + pa); // the consensus may run now (rbuf[RTK_RB_PARK_MOVES], hand-over H2): the forward alignment is swept again, stored, and walked before the second strand overwrites the table
                auto audit = [&](const char* seq, uint32_t sl, const char* q, uint32_t ql) { // what the full route is about to emit against the forward strings
                    if (skippable && !(sl == fw.seq_len && ql == fw.qual_len && rtk_str_equal(seq, fw.seq, sl) && rtk_str_equal(q, fw.qual, ql))) s.cnt[RTK_RC_STRAND2_AUDIT_MISMATCH] += 1;
                };
                const uint32_t i_solid_bw = so.n - i - 2;
                uint32_t i_weak_bw = we.n - i_weak;
                i_weak_bw = rtk_an_first_gt(we_r, 0, i_weak_bw, rtk_an_pos(so_r, i_solid_bw));
                RTK_PL(s, RTK_LAP_DRIVER_STRAND2);
                { const uint32_t gl_ = pb - pa; RTK_HIST_ADD(s, RTK_H_STRAND2 + rtk_gap_class(gl_), 1); }
                rtk_correct_region(c, s_bw, L, so_r, we_r, i_solid_bw, i_weak_bw, &fw, bw, q_bw);
                if (rtk_failed(s)) return;
                RTK_PL(s, RTK_LAP_DRIVER_STRAND2);
                rtk_rc_reverse_complement(s, bw, s.bm[RTK_BM_RC_TMP], s.rbuf[RTK_RB_RC_TMP]);
                if (bw.is_corrected) {
                    // l_solid = (|s_bw| - rev_pos(i_solid_bw + 1) - k) - prev_pos == pa - prev_pos
                    audit(bw.seq, bw.seq_len, bw.qual, bw.qual_len);
                    emit_minus_k(bw.seq, bw.seq_len, bw.qual, bw.qual_len);
                } else {
                    const uint32_t ref_len = pb - pa + k;
                    uint32_t& csl = s.loc.len[RTK_LEN_CONS_SEQ]; uint32_t& cql = s.loc.len[RTK_LEN_CONS_QUAL]; csl = 0; cql = 0;
                    const unsigned long long tc0 = rtk_clock();
                    const bool ok = rtk_generate_consensus(c, &fw, &bw, s_fw + pa, ref_len, c.o.weak_region_len_factor, s.rbuf[RTK_RB_CONS_SEQ], &csl, s.rbuf[RTK_RB_CONS_QUAL], &cql);
                    s.cnt[RTK_RC_CYC_CONSENSUS] += rtk_clock() - tc0;
                    RTK_PL(s, RTK_LAP_CONS_FINAL);
                    if (rtk_failed(s)) return;
                    if (!ok || csl == 0) { // raw region, k solid qualities then minimum quality (:898-904)
                        csl = 0; cql = 0;
                        rtk_app(s, s.rbuf[RTK_RB_CONS_SEQ], &csl, s_fw + pa, ref_len);
                        if (lrc) rtk_app(s, s.rbuf[RTK_RB_CONS_QUAL], &cql, q_fw + pa, ref_len); // :902
                        else { rtk_app_fill(s, s.rbuf[RTK_RB_CONS_QUAL], &cql, q_max, k); rtk_app_fill(s, s.rbuf[RTK_RB_CONS_QUAL], &cql, q_min, pb - pa); }
                    }
                    audit(s.rbuf[RTK_RB_CONS_SEQ], csl, s.rbuf[RTK_RB_CONS_QUAL], cql);
                    emit_minus_k(s.rbuf[RTK_RB_CONS_SEQ], csl, s.rbuf[RTK_RB_CONS_QUAL], cql);
                }
            }
        } else isUncorrected = true;
        if (isUncorrected) { // :920-932
            rtk_app(s, out_s, &osl, s_fw + prev_pos, pb - prev_pos);
            if (lrc) rtk_app(s, out_q, &oql, q_fw + prev_pos, pb - prev_pos); // :924
            else {
                rtk_app_fill(s, out_q, &oql, q_max, pa - prev_pos);
                if (pb < pa + k) rtk_app_fill(s, out_q, &oql, q_max, pb - pa);
                else { rtk_app_fill(s, out_q, &oql, q_max, k); rtk_app_fill(s, out_q, &oql, q_min, pb - pa - k); }
            }
        }
    } else if (kind == RTK_RG_TAIL) { // :940-950
        const uint32_t i = rd->i_solid, prev_pos = rd->prev_pos;
        const uint32_t pa = so.pos[i];
        const uint32_t i_weak = rtk_an_first_ge(we, 0, we.n, pa);
        if (lrc && has_min_qual(pa, L)) { // :941: nothing to do, the else branch of :951-955
            rtk_app(s, out_s, &osl, s_fw + prev_pos, L - prev_pos); rtk_app(s, out_q, &oql, q_fw + prev_pos, L - prev_pos);
        } else {
            rtk_correct_region(c, s_fw, L, so, we, i, i_weak, nullptr, fw, q_fw);
            if (rtk_failed(s)) return;
            const uint32_t l_solid = pa - prev_pos;
            rtk_app(s, out_s, &osl, s_fw + prev_pos, l_solid); rtk_app(s, out_s, &osl, fw.seq, fw.seq_len);
            app_q(prev_pos, l_solid, q_max); rtk_app(s, out_q, &oql, fw.qual, fw.qual_len);
        }
    } else { // RTK_RG_TAIL_COPY (:951-955)
        const uint32_t i = rd->i_solid, prev_pos = rd->prev_pos;
        const uint32_t pa = so.pos[i];
        rtk_app(s, out_s, &osl, s_fw + prev_pos, L - prev_pos);
        if (lrc) rtk_app(s, out_q, &oql, q_fw + prev_pos, L - prev_pos);
        else { rtk_app_fill(s, out_q, &oql, q_max, pa - prev_pos + k); rtk_app_fill(s, out_q, &oql, q_min, L - pa - k); }
    }
    if (rtk_failed(s)) return;
    RTK_PL(s, RTK_LAP_DRIVER_EMIT_PREP);
    rtk_emit_segment(c, rd, out_s, osl, out_q, oql);
    RTK_PL(s, RTK_LAP_EMIT);
}

#endif
