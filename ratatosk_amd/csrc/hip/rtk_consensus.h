// Region stage, generateConsensus (reference: src/Alignment.cpp:309-470, moveIntoCIGAR :354-411): the merge of the two strands' corrections
// of a gap region along their NW alignments against the raw region. The forward strand's alignment comes from its trim's stored sweep where
// there is one (TrimPark; rtk_region_align.h).
#ifndef RTK_CONSENSUS_H
#define RTK_CONSENSUS_H

#include "rtk_region_align.h"
#include "rtk_region_result.h"

// ------------------------------------------------------------------------------------------------ generateConsensus (src/Alignment.cpp:309-470)
struct CigCur { const uint8_t* mv; uint32_t n, idx, qpos, rpos; }; // op-granular cursor over an alignment (moves 0/3 = M, 1 = I, 2 = D)
RTK_DEV char rtk_mv_op(uint8_t m) { return (m == 1) ? 'I' : (m == 2 ? 'D' : 'M'); }
RTK_DEV uint32_t rtk_op_len(const CigCur& cc) { // length of the run of equal ops at the cursor; 64 moves per step
    const uint8_t* mv = rtk_u(cc.mv); const uint32_t n = rtk_u(cc.n), idx = rtk_u(cc.idx);
    const char op = rtk_mv_op(rtk_ld(mv + idx));
    for (uint32_t j0 = idx; j0 < n; j0 += RTK_WAVE) {
        const uint32_t j = j0 + static_cast<uint32_t>(rtk_lane());
        const uint64_t diff = rtk_ballot(j < n && rtk_mv_op(mv[j]) != op);
        if (diff) return j0 + static_cast<uint32_t>(rtk_ffs(diff) - 1) - idx;
    }
    return n - idx;
}

RTK_FN void rtk_move_into_cigar(uint32_t start_, uint32_t end_, CigCur& cc_, uint32_t* rs_, uint32_t* re_, uint32_t* ref_out_) {
    uint32_t start = rtk_u(start_); uint32_t end = rtk_u(end_); CigCur& cc = *rtk_u(&cc_); uint32_t* rs = rtk_u(rs_); uint32_t* re = rtk_u(re_); uint32_t* ref_out = rtk_u(ref_out_); // moveIntoCIGAR (:354-411)
    uint32_t read_pos_start = cc.qpos, read_pos_end;
    while (cc.idx != cc.n && cc.rpos < start) {
        const uint32_t l = rtk_op_len(cc); const char op = rtk_mv_op(cc.mv[cc.idx]);
        if (op == 'M') { if (cc.rpos + l > start) { read_pos_start = cc.qpos + (start - cc.rpos); break; } cc.qpos += l; cc.rpos += l; }
        else if (op == 'I') cc.qpos += l; else cc.rpos += l;
        cc.idx += l; read_pos_start = cc.qpos;
    }
    read_pos_end = read_pos_start;
    while (cc.idx != cc.n && cc.rpos < end) {
        const uint32_t l = rtk_op_len(cc); const char op = rtk_mv_op(cc.mv[cc.idx]);
        if (op == 'M') { if (cc.rpos + l > end) { *rs = read_pos_start; *re = cc.qpos + (end - cc.rpos); *ref_out = end; return; } cc.qpos += l; cc.rpos += l; }
        else if (op == 'I') cc.qpos += l; else cc.rpos += l;
        cc.idx += l; read_pos_end = cc.qpos;
    }
    *rs = read_pos_start; *re = read_pos_end; *ref_out = cc.rpos;
}

// writes the consensus into out_s/out_q; returns false when the result is "empty" (caller falls back to the raw region)
// lane-parallel string predicates (wave-uniform results)
RTK_DEV bool rtk_str_equal(const char* a, const char* b, uint32_t n) {
    for (uint32_t i0 = 0; i0 < n; i0 += RTK_WAVE) { const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane()); if (rtk_ballot(i < n && a[i] != b[i]) != 0ull) return false; }
    return true;
}
RTK_DEV bool rtk_all_acgt(const char* p, uint32_t n) {
    for (uint32_t i0 = 0; i0 < n; i0 += RTK_WAVE) { const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane()); const char ch = i < n ? p[i] : 'A'; if (rtk_ballot(!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T')) != 0ull) return false; }
    return true;
}

RTK_FN bool rtk_generate_consensus(const RCtx& c_, const ResCorr* fw_, const ResCorr* bw_, const char* ref_, uint32_t ref_len_, double max_norm_, char* out_s_, uint32_t* out_sl_, char* out_q_, uint32_t* out_ql_) {
    const RCtx& c = *rtk_u(&c_); const ResCorr* fw = rtk_u(fw_); const ResCorr* bw = rtk_u(bw_); RTK_ASSUME_LDS(fw); RTK_ASSUME_LDS(bw); const char* ref = rtk_u(ref_); uint32_t ref_len = rtk_u(ref_len_); double max_norm = rtk_u(max_norm_); char* out_s = rtk_u(out_s_); uint32_t* out_sl = rtk_u(out_sl_); char* out_q = rtk_u(out_q_); uint32_t* out_ql = rtk_u(out_ql_);
    RegionScratch& s = rtk_hdr(c);
    *out_sl = 0; *out_ql = 0;
    RTK_PL(s, RTK_LAP_CONS_ENTRY);
    const uint32_t nfw = rtk_bm_card(fw->bm, fw->old_len), nbw = rtk_bm_card(bw->bm, bw->old_len);
    auto take = [&](const ResCorr* r) { rtk_app(s, out_s, out_sl, r->seq, r->seq_len); rtk_app(s, out_q, out_ql, r->qual, r->qual_len); return true; };
    if (nbw == 0 && nfw != 0) return take(fw);
    else if (nfw == 0 && nbw != 0) return take(bw);
    else if (nfw + nbw == 0) return false;
    if (nbw > nfw) { const ResCorr* t = fw; fw = bw; bw = t; }
    // NW path alignments of both corrections against the raw region; the moves are parked in str[RTK_STR_CONS_MOVES_FW] and str[RTK_STR_CONS_MOVES_BW]. The alignment of the
    // forward strand's string was walked from its trim's sweep already (rtk_trim_by_column, rtk_park_walk: s.loc.park, moves in rbuf[RTK_RB_PARK_MOVES], which is written below only: it is out_q, RTK_RB_CONS_QUAL).
    const TrimPark pk = s.loc.park;
    auto parked = [&](const ResCorr* x) { return pk.nm != 0 && x->seq_len == pk.len && (x->seq == s.rbuf[RTK_RB_FW_SEQ].get() || rtk_str_equal(x->seq, s.rbuf[RTK_RB_FW_SEQ], pk.len)); };
    auto resume = [&](char* dst, uint32_t* nm) { MyersResult r; r.dist = pk.dist; r.first = r.last = static_cast<int32_t>(ref_len) - 1; r.nloc = 1; *nm = pk.nm; rtk_wcopy(dst, s.rbuf[RTK_RB_PARK_MOVES], pk.nm); return r; };
    uint32_t nm_fw = 0, nm_bw = 0;
    MyersResult afw;
    const bool fw_parked = parked(fw);
    if (fw_parked) afw = resume(s.str[RTK_STR_CONS_MOVES_FW], &nm_fw);
    else {
        RTK_SITE(RTK_SITE_CONS_FW); afw = rtk_align_path(c, fw->seq, fw->seq_len, ref, ref_len, RTK_MODE_NW, &nm_fw);
        if (rtk_failed(s) || nm_fw > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return false; }
        rtk_wcopy(s.str[RTK_STR_CONS_MOVES_FW], s.my.moves, nm_fw);
    }
    RTK_PL(s, RTK_LAP_CONS_FW_PATH);
    // Both directions usually arrive at the same corrected string: its alignment against the raw region is then the one just computed
    const bool same_strings = bw->seq_len == fw->seq_len && rtk_str_equal(bw->seq, fw->seq, fw->seq_len);
    MyersResult abw = afw;
    bool bw_parked = false;
    if (same_strings) { nm_bw = nm_fw; rtk_wcopy(s.str[RTK_STR_CONS_MOVES_BW], s.str[RTK_STR_CONS_MOVES_FW], nm_fw); }
    else if ((bw_parked = parked(bw))) abw = resume(s.str[RTK_STR_CONS_MOVES_BW], &nm_bw);
    else {
        RTK_SITE(RTK_SITE_CONS_BW); abw = rtk_align_path(c, bw->seq, bw->seq_len, ref, ref_len, RTK_MODE_NW, &nm_bw);
        if (rtk_failed(s) || nm_bw > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return false; }
        rtk_wcopy(s.str[RTK_STR_CONS_MOVES_BW], s.my.moves, nm_bw);
    }
    s.cnt[(fw_parked || bw_parked) ? RTK_RC_CONS_RESUMED : RTK_RC_CONS_SWEPT] += 1;
    const double n_fw = static_cast<double>(afw.dist) / static_cast<double>(fw->seq_len > ref_len ? fw->seq_len : ref_len);
    const double n_bw = static_cast<double>(abw.dist) / static_cast<double>(bw->seq_len > ref_len ? bw->seq_len : ref_len);
    if (max_norm > 0.0 && (n_fw > max_norm || n_bw > max_norm)) {
        if (n_fw > max_norm && n_bw > max_norm) return false;
        if (n_fw > max_norm) return take(bw);
        return take(fw);
    }
    RTK_PL(s, RTK_LAP_CONS_BW_PATH);
    CigCur cf, cb;
    cf.mv = reinterpret_cast<const uint8_t*>(s.str[RTK_STR_CONS_MOVES_FW].get()); cf.n = nm_fw; cf.idx = 0; cf.qpos = 0; cf.rpos = 0;
    cb.mv = reinterpret_cast<const uint8_t*>(s.str[RTK_STR_CONS_MOVES_BW].get()); cb.n = nm_bw; cb.idx = 0; cb.qpos = 0; cb.rpos = 0;
    uint32_t i = 0;
    while (i < ref_len && !rtk_failed(s)) {
        int64_t len_fw = rtk_rc_len_corrected(*fw, i), len_bw = rtk_rc_len_corrected(*bw, i);
        if ((len_fw + len_bw) <= 0) {
            len_fw = rtk_rc_len_uncorrected(*fw, i); len_bw = rtk_rc_len_uncorrected(*bw, i);
            if (len_fw > len_bw || len_fw <= 0) len_fw = -1; else len_bw = -1;
        }
        uint32_t rs, re, rout;
        if (len_fw >= len_bw) {
            rtk_move_into_cigar(i, static_cast<uint32_t>(static_cast<int64_t>(i) + len_fw), cf, &rs, &re, &rout);
            if (re > rs) { rtk_app(s, out_s, out_sl, fw->seq + rs, (rs < fw->seq_len) ? ((re - rs) < (fw->seq_len - rs) ? (re - rs) : (fw->seq_len - rs)) : 0);
                           rtk_app(s, out_q, out_ql, fw->qual + rs, (rs < fw->qual_len) ? ((re - rs) < (fw->qual_len - rs) ? (re - rs) : (fw->qual_len - rs)) : 0); }
        } else {
            rtk_move_into_cigar(i, static_cast<uint32_t>(static_cast<int64_t>(i) + len_bw), cb, &rs, &re, &rout);
            if (re > rs) { rtk_app(s, out_s, out_sl, bw->seq + rs, (rs < bw->seq_len) ? ((re - rs) < (bw->seq_len - rs) ? (re - rs) : (bw->seq_len - rs)) : 0);
                           rtk_app(s, out_q, out_ql, bw->qual + rs, (rs < bw->qual_len) ? ((re - rs) < (bw->qual_len - rs) ? (re - rs) : (bw->qual_len - rs)) : 0); }
        }
        if (rout == i) { rtk_fail_ovf(s, RTK_OVF_CONS_STALL); return false; } // no progress: would loop forever in the reference as well
        i = rout;
    }
    RTK_PL(s, RTK_LAP_CONS_MERGE);
    if (max_norm > 0.0 && !rtk_failed(s)) {
        // The merged string is very often one of the two inputs again. Its distance to the raw region is then the one computed above --
        // provided the plain configuration of this last call (edlibDefaultAlignConfig, :460: no IUPAC equalities) cannot tell the two
        // apart, i.e. both strings hold A/C/G/T only -- and that distance already passed the max_norm test above: nothing to compute.
        const bool is_fw = *out_sl == fw->seq_len && rtk_str_equal(out_s, fw->seq, fw->seq_len);
        const bool is_bw = !is_fw && *out_sl == bw->seq_len && rtk_str_equal(out_s, bw->seq, bw->seq_len);
        if ((is_fw || is_bw) && rtk_all_acgt(out_s, *out_sl) && rtk_all_acgt(ref, ref_len)) return true;
        RTK_SITE(RTK_SITE_CONS_FINAL); const MyersResult a = rtk_align(c, out_s, *out_sl, ref, ref_len, -1, RTK_MODE_NW, /*iupac=*/false); // edlibDefaultAlignConfig (:460)
        const double n = static_cast<double>(a.dist) / static_cast<double>(*out_sl > ref_len ? *out_sl : ref_len);
        if (n > max_norm) { *out_sl = 0; *out_ql = 0; return take(fw); }
    }
    return true;
}

#endif
