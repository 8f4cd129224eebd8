// Region stage, anchors, arenas and path records (reference: src/Path.hpp: extend :308-363, merge :366-414, toString :449-485, prunePrefix
// :487-571; the anchor lists of src/Correction.cpp:196-213; getQual / getMinMaxLength of src/Common.hpp:410-438). Paths live as immutable
// records in the per-wave bump arenas (three nesting levels, RtkArena); a WPath is the one mutable working copy of a level.
#ifndef RTK_REGION_PATHS_H
#define RTK_REGION_PATHS_H

#include "rtk_region_types.h"
#include "rtk_seeds.h"

#ifndef RTK_SIM
RTK_DEV UMap rtk_u(const UMap& m) { UMap r; r.unitig = rtk_u(m.unitig); r.dist = rtk_u(m.dist); r.len = rtk_u(m.len); r.strand = rtk_u(m.strand); return r; }
#endif

// ------------------------------------------------------------------------------------------------ helpers (src/Common.hpp:410-438)
RTK_DEV char rtk_get_qual(double score, uint64_t qv_min, uint64_t qv_max) {
    const char phred_base_std = static_cast<char>(33);
    const char phred_scale_std = static_cast<char>(qv_max);
    const double s = score < 1.0 ? score : 1.0;
    const double qv_score = s * static_cast<double>(static_cast<uint64_t>(phred_scale_std) - qv_min);
    return static_cast<char>(qv_score + static_cast<double>(phred_base_std) + static_cast<double>(qv_min));
}
RTK_DEV void rtk_min_max_len(uint64_t l, double f, uint64_t* mn, uint64_t* mx) {
    const double lf = static_cast<double>(l);
    const double a = lf - (lf * f), b = lf + (lf * f);
    *mn = static_cast<uint64_t>(a > 1.0 ? a : 1.0); *mx = static_cast<uint64_t>(b > 1.0 ? b : 1.0);
}

RTK_DEV char rtk_comp(char c) {
    switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
                 case 'M': return 'K'; case 'K': return 'M'; case 'R': return 'Y'; case 'Y': return 'R';
                 case 'V': return 'B'; case 'B': return 'V'; case 'H': return 'D'; case 'D': return 'H'; default: return c; }
}

// the flag is the header's own ovf_word (s.overflow points at it for the alignment code, which only knows its MyersScratch)
RTK_DEV void rtk_fail_ovf(RegionScratch& s, uint32_t code) { s.ovf_word = code; }
RTK_DEV bool rtk_failed(const RegionScratch& s) { return s.ovf_word != 0; }

// anchors of a read in forward or reverse-complement orientation (src/Correction.cpp:196-213)
RTK_DEV uint32_t rtk_an_pos(const Anchors& a, uint32_t i) { return a.rev ? (a.L - a.pos[a.n - 1 - i] - static_cast<uint32_t>(a.k)) : a.pos[i]; }
RTK_DEV UMap rtk_an_um(const Anchors& a, uint32_t i) {
    const uint32_t j = a.rev ? (a.n - 1 - i) : i;
    UMap u = rtk_unpack_hit(a.hit ? a.hit[j] : a.hits_by_pos[a.pos[j]]);
    if (a.rev) u.strand ^= 1u;
    return u;
}

// positions are ascending in the anchor index: searches replace the reference's linear walks over the lists. A search is a chain of
// dependent memory round trips, so it is 64-ary: every lane probes one pivot per step (two steps for 4096 anchors instead of twelve).
// first x in [lo, hi) with pos(x) >= key (strict: > key), else hi
RTK_DEV uint32_t rtk_an_search(const Anchors& a, uint32_t lo_, uint32_t hi_, uint64_t key_, bool strict_) {
    uint32_t lo = rtk_u(lo_), hi = rtk_u(hi_); const uint64_t key = rtk_u(key_); const bool strict = rtk_u(strict_);
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
#ifdef RTK_SIM
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; const uint64_t p = rtk_an_pos(a, mid); if (strict ? (p <= key) : (p < key)) lo = mid + 1; else hi = mid; }
    (void)lane; return lo;
#else
    while (lo < hi) {
        const uint32_t span = hi - lo;
        if (span <= RTK_WAVE) { // one probe per candidate
            const uint32_t x = lo + lane; bool t = false;
            if (x < hi) { const uint64_t p = rtk_an_pos(a, x); t = strict ? (p > key) : (p >= key); }
            const uint64_t b = rtk_ballot(t);
            return b ? lo + static_cast<uint32_t>(rtk_ffs(b) - 1) : hi;
        }
        // 64 pivots strictly inside [lo, hi): x_i = lo + (i + 1) * span / 65
        const uint32_t x = lo + static_cast<uint32_t>((static_cast<uint64_t>(lane + 1) * span) / (RTK_WAVE + 1));
        const uint64_t p = rtk_an_pos(a, x);
        const bool t = strict ? (p > key) : (p >= key);
        const uint64_t b = rtk_ballot(t); // monotone: 0..0 1..1
        const int j = b ? rtk_ffs(b) - 1 : RTK_WAVE; // first pivot that satisfies the test
        const uint32_t nlo = (j == 0) ? lo : rtk_u(rtk_shfl(x, j - 1)) + 1u; // the answer is after pivot j-1 ...
        const uint32_t nhi = (j == RTK_WAVE) ? hi : rtk_u(rtk_shfl(x, j));   // ... and not after pivot j
        lo = nlo; hi = nhi;
    }
    return lo;
#endif
}
RTK_DEV uint32_t rtk_an_first_ge(const Anchors& a, uint32_t lo, uint32_t hi, uint64_t key) { return rtk_an_search(a, lo, hi, key, false); }
RTK_DEV uint32_t rtk_an_first_gt(const Anchors& a, uint32_t lo, uint32_t hi, uint64_t key) { return rtk_an_search(a, lo, hi, key, true); }

// ------------------------------------------------------------------------------------------------ arenas and paths (src/Path.hpp)
struct PathHdr { U<uint32_t> n, l, qlen, pad; }; // followed by n UMap and qlen quality bytes

RTK_DEV uint64_t rtk_arena_alloc(RegionScratch& s, int lvl, uint64_t bytes) {
    bytes = (bytes + 15ull) & ~15ull;
    const uint64_t off = rtk_ld(&s.top[lvl]);
    if (off + bytes > rtk_ld(&s.arena_cap)) { rtk_fail_ovf(s, RTK_OVF_ARENA); return 0; }
    s.top[lvl] = off + bytes; return off;
}
RTK_DEV PathHdr* rtk_path_hdr(const RegionScratch& s, int lvl, uint64_t h) { return reinterpret_cast<PathHdr*>(rtk_ld(&s.arena[lvl]) + h); }
RTK_DEV UMap* rtk_path_ums(const RegionScratch& s, int lvl, uint64_t h) { return reinterpret_cast<UMap*>(rtk_ld(&s.arena[lvl]) + h + sizeof(PathHdr)); }
RTK_DEV char* rtk_path_qual(const RegionScratch& s, int lvl, uint64_t h) { const PathHdr* p = rtk_path_hdr(s, lvl, h); return reinterpret_cast<char*>(const_cast<PathHdr*>(p)) + sizeof(PathHdr) + sizeof(UMap) * rtk_ld(&p->n); }
// handles carry their level in the top 2 bits
RTK_DEV uint64_t rtk_mk_handle(int lvl, uint64_t off) { return (static_cast<uint64_t>(lvl) << 62) | off; }
RTK_DEV int rtk_h_lvl(uint64_t h) { return static_cast<int>(h >> 62); }
RTK_DEV uint64_t rtk_h_off(uint64_t h) { return h & 0x3FFFFFFFFFFFFFFFull; }

RTK_DEV void rtk_wp_clear(WPath& p) { p.n = 0; p.l = 0; p.qlen = 0; }

RTK_FN_LEAF uint64_t rtk_wp_commit(RegionScratch& s_, const WPath& p_, int lvl_) { // working path -> immutable record
    RegionScratch& s = *rtk_u(&s_); RTK_ASSUME_LDS(&s); const WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); const int lvl = rtk_u(lvl_);
    const unsigned long long tc0 = rtk_clock();
    const uint32_t pn = rtk_ld(&p.n), pl = rtk_ld(&p.l), pq = rtk_ld(&p.qlen);
    const uint64_t off = rtk_arena_alloc(s, lvl, sizeof(PathHdr) + sizeof(UMap) * pn + pq);
    if (rtk_failed(s)) return 0;
    char* rec = rtk_ld(&s.arena[lvl]) + off;
    PathHdr* h = reinterpret_cast<PathHdr*>(rec);
    h->n = pn; h->l = pl; h->qlen = pq; h->pad = 0;
    rtk_wcopy2(rec + sizeof(PathHdr), rtk_ld(&p.ums), sizeof(UMap) * pn, rec + sizeof(PathHdr) + sizeof(UMap) * pn, rtk_ld(&p.qual), pq);
    s.cnt[RTK_RC_CYC_PATHREC] += rtk_clock() - tc0;
    return rtk_mk_handle(lvl, off);
}

RTK_FN_LEAF void rtk_wp_load(RegionScratch& s_, WPath& p_, uint64_t h_) {
    RegionScratch& s = *rtk_u(&s_); RTK_ASSUME_LDS(&s); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); const uint64_t h = rtk_u(h_);
    const int lvl = rtk_h_lvl(h); const uint64_t off = rtk_h_off(h);
    const char* rec = rtk_ld(&s.arena[lvl]) + off;
    const PathHdr* hd = reinterpret_cast<const PathHdr*>(rec);
    const uint32_t hn = rtk_ld(&hd->n), hl = rtk_ld(&hd->l), hq = rtk_ld(&hd->qlen);
    if (hn > rtk_ld(&s.um_cap) || hq > rtk_ld(&s.str_cap)) { rtk_fail_ovf(s, RTK_OVF_PATH_LOAD); rtk_wp_clear(p); return; }
    const unsigned long long tc0 = rtk_clock();
    p.n = hn; p.l = hl; p.qlen = hq;
    rtk_wcopy2(rtk_ld(&p.ums), rec + sizeof(PathHdr), sizeof(UMap) * hn, rtk_ld(&p.qual), rec + sizeof(PathHdr) + sizeof(UMap) * hn, hq);
    s.cnt[RTK_RC_CYC_PATHREC] += rtk_clock() - tc0;
}

RTK_DEV uint32_t rtk_rec_n(const RegionScratch& s, uint64_t h) { return rtk_ld(&rtk_path_hdr(s, rtk_h_lvl(h), rtk_h_off(h))->n); }
RTK_DEV uint32_t rtk_rec_l(const RegionScratch& s, uint64_t h) { return rtk_ld(&rtk_path_hdr(s, rtk_h_lvl(h), rtk_h_off(h))->l); }
RTK_DEV UMap rtk_rec_back(const RegionScratch& s, uint64_t h) { const int lv = rtk_h_lvl(h); const uint64_t o = rtk_h_off(h); const char* rec = rtk_ld(&s.arena[lv]) + o; return rtk_u(reinterpret_cast<const UMap*>(rec + sizeof(PathHdr))[rtk_ld(&reinterpret_cast<const PathHdr*>(rec)->n) - 1]); }

RTK_DEV uint32_t rtk_nkm_u(const RCtx& c, uint32_t u) { // k-mers of unitig u, uniform
    const uint64_t* uo = c.g.uoff.get() + u;
    return static_cast<uint32_t>(rtk_ld(uo + 1) - rtk_ld(uo)) - static_cast<uint32_t>(rtk_u(c.k)) + 1u;
}
RTK_DEV void rtk_wp_norm_back(const RCtx& c, WPath& p) { // the former end becomes a whole unitig (Path.hpp:319-323)
    const uint32_t pn = rtk_ld(&p.n);
    if (pn >= 2) { UMap* e = rtk_ld(&p.ums) + (pn - 1); e->dist = 0; e->len = rtk_nkm_u(c, rtk_ld(&e->unitig)); }
}

RTK_FN_HOT void rtk_wp_extend(const RCtx& c, WPath& p_, const UMap& um_) { // Path.hpp:308-330
    RegionScratch& s = *rtk_u(c.sc); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); const UMap um = rtk_u(um_);
    if (rtk_um_is_empty(um)) return;
    const uint32_t pn = rtk_ld(&p.n);
    if (pn >= rtk_ld(&s.um_cap)) { rtk_fail_ovf(s, RTK_OVF_PATH_UNITIGS); return; }
    UMap* ums = rtk_ld(&p.ums);
    if (pn == 0) { ums[0] = um; p.n = 1; p.l = um.len + static_cast<uint32_t>(rtk_u(c.k)) - 1; }
    else { rtk_wp_norm_back(c, p); ums[pn] = um; p.n = pn + 1; p.l = rtk_ld(&p.l) + um.len; }
}

// extend with a quality slice q[0..qn) (Path.hpp:332-363): appended only when its length equals um.len + k - 1
RTK_FN void rtk_wp_extend_q(const RCtx& c_, WPath& p_, UMap um_, const char* q_, uint32_t qn_) {
    const RCtx& c = *rtk_u(&c_); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); const UMap um = rtk_u(um_); const char* q = rtk_u(q_); uint32_t qn = rtk_u(qn_);
    RegionScratch& s = rtk_hdr(c);
    if (rtk_um_is_empty(um)) return;
    if (p.n >= s.um_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_UNITIGS); return; }
    const uint32_t want = um.len + static_cast<uint32_t>(c.k) - 1;
    if (p.n == 0) {
        p.ums[0] = um; p.n = 1; p.l = want;
        if (qn == want) { if (qn > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_QUAL); return; } rtk_wcopy(p.qual, q, qn); p.qlen = qn; }
    } else {
        rtk_wp_norm_back(c, p); p.ums[p.n] = um; ++p.n; p.l += um.len;
        if (qn == want) {
            const uint32_t add = qn - (static_cast<uint32_t>(c.k) - 1);
            if (p.qlen + add > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_QUAL); return; }
            rtk_wcopy(p.qual + p.qlen, q + (c.k - 1), add); p.qlen += add;
        }
    }
}

// fills qual with `ch` for a fresh single-unitig path (string(len + k - 1, getQual(1.0)))
RTK_FN_LEAF void rtk_wp_start(const RCtx& c_, WPath& p_, UMap um_, char ch_) {
    const RCtx& c = *rtk_u(&c_); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); const UMap um = rtk_u(um_); char ch = rtk_u(ch_);
    RegionScratch& s = rtk_hdr(c);
    rtk_wp_clear(p);
    const uint32_t want = um.len + static_cast<uint32_t>(c.k) - 1;
    if (want > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_QUAL); return; }
    p.ums[0] = um; p.n = 1; p.l = want;
    rtk_wfill(p.qual, ch, want); p.qlen = want;
}

// p.merge(o) where o is a committed record (Path.hpp:366-414)
RTK_FN void rtk_wp_merge(const RCtx& c_, WPath& p_, uint64_t ho_) {
    const RCtx& c = *rtk_u(&c_); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); uint64_t ho = rtk_u(ho_);
    RegionScratch& s = rtk_hdr(c);
    const int lv = rtk_h_lvl(ho); const uint64_t oo = rtk_h_off(ho);
    const PathHdr* o = rtk_path_hdr(s, lv, oo);
    const UMap* oums = rtk_path_ums(s, lv, oo);
    const char* oq = rtk_path_qual(s, lv, oo);
    if (o->l == 0) return;
    if (p.l == 0) { rtk_wp_load(s, p, ho); return; }
    if ((p.qlen == 0) != (o->qlen == 0)) return;
    const UMap last = p.ums[p.n - 1];
    if (last.unitig != oums[0].unitig || last.strand != oums[0].strand) return;
    if (p.n + o->n > s.um_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_UNITIGS); return; }
    if (p.n == 1) {
        UMap& st = p.ums[0];
        if (!st.strand) st.dist = oums[0].dist;
        st.len += oums[0].len - 1;
        for (uint32_t i = 1; i < o->n; ++i) p.ums[p.n++] = oums[i];
    } else {
        UMap& en = p.ums[p.n - 1];
        if (!en.strand) en.dist = oums[0].dist;
        en.len += oums[0].len - 1;
        if (o->n >= 2) { rtk_wp_norm_back(c, p); for (uint32_t i = 1; i < o->n; ++i) p.ums[p.n++] = oums[i]; }
    }
    p.l += o->l - static_cast<uint32_t>(c.k);
    if (o->qlen != 0) {
        const uint32_t kk = static_cast<uint32_t>(c.k);
        const uint32_t add = o->qlen > kk ? o->qlen - kk : 0; // o.qual.substr(k)
        if (p.qlen + add > s.str_cap) { rtk_fail_ovf(s, RTK_OVF_PATH_QUAL); return; }
        rtk_wcopy(p.qual + p.qlen, oq + kk, add); p.qlen += add;
    }
}

RTK_FN void rtk_wp_prune_prefix(const RCtx& c_, WPath& p_, uint32_t len_) {
    const RCtx& c = *rtk_u(&c_); WPath& p = *rtk_u(&p_); RTK_ASSUME_LDS(&p); uint32_t len = rtk_u(len_); // Path.hpp:487-571
    if (p.n == 0 || p.l == 0 || len >= p.l) return;
    const uint32_t k = static_cast<uint32_t>(c.k);
    UMap& st = p.ums[0];
    if (p.n == 1) { if (!st.strand) st.dist += p.l - len; st.len -= p.l - len; }
    else if (st.len + k - 1 >= len) {
        p.l = st.len + k - 1; p.n = 1;
        if (!st.strand) st.dist += p.l - len;
        st.len -= p.l - len;
    } else if (p.n == 2 || len > (p.l - p.ums[p.n - 1].len)) {
        UMap& en = p.ums[p.n - 1];
        if (!en.strand) en.dist += p.l - len;
        en.len -= p.l - len;
    } else {
        uint32_t acc = st.len + k - 1, w = 1; bool cut = false;
        const UMap old_end = p.ums[p.n - 1];
        for (uint32_t i = 1; i + 1 < p.n; ++i) {
            UMap cur = p.ums[i]; cur.dist = 0; cur.len = rtk_nkm(c.g, cur.unitig);
            acc += cur.len;
            if (acc < len) { p.ums[w++] = cur; }
            else { if (!cur.strand) cur.dist += acc - len; cur.len -= acc - len; p.ums[w++] = cur; cut = true; break; }
        }
        if (!cut) p.ums[w++] = old_end;
        p.n = w;
    }
    p.l = len;
    if (p.qlen != 0 && p.qlen > p.l) p.qlen = p.l;
}

// mappedSequenceToString of one mapping into dst (lane-parallel 2-bit decode, reverse complement on the fly)
RTK_DEV void rtk_um_decode(const RCtx& c, const UMap& um, char* dst, uint32_t skip) {
    const uint32_t n = um.len + static_cast<uint32_t>(rtk_u(c.k)) - 1;
    const uint64_t b0 = rtk_ld(c.g.uoff.get() + um.unitig) + um.dist;
    const uint64_t* useq = c.g.useq.get();
    for (uint32_t i = skip + static_cast<uint32_t>(rtk_lane()); i < n; i += RTK_WAVE) {
        const uint64_t pos = um.strand ? (b0 + i) : (b0 + (n - 1 - i));
        const uint32_t b = static_cast<uint32_t>((useq[pos >> 5] >> (2 * (pos & 31))) & 3ull);
        const uint32_t code = um.strand ? b : (3u - b);
        dst[i - skip] = static_cast<char>((0x54474341u >> (8 * code)) & 0xFFu); // "ACGT"
    }
}

// Path::toString (Path.hpp:449-485) of `n` mappings into dst; returns length (0xFFFFFFFF on overflow)
RTK_FN uint32_t rtk_ums_to_string(const RCtx& c, const UMap* ums_, uint32_t n_, char* dst_) {
    RegionScratch& s = *rtk_u(c.sc); const UMap* ums = rtk_u(ums_); const uint32_t n = rtk_u(n_); char* dst = rtk_u(dst_);
    const unsigned long long tc0 = rtk_clock();
    uint32_t len = 0;
    const uint32_t k1 = static_cast<uint32_t>(rtk_u(c.k)) - 1, str_cap = rtk_ld(&s.str_cap);
    for (uint32_t i = 0; i < n; ++i) {
        const UMap um = rtk_u(ums[i]);
        const uint32_t skip = i ? k1 : 0;
        const uint32_t add = um.len + k1 - skip;
        if (len + add > str_cap) { rtk_fail_ovf(s, RTK_OVF_STRING); return 0xFFFFFFFFu; }
        rtk_um_decode(c, um, dst + len, skip);
        len += add;
    }
    rtk_sync();
    s.cnt[RTK_RC_PATHBASE] += len;
    s.cnt[RTK_RC_CYC_TOSTRING] += rtk_clock() - tc0;
    return len;
}
RTK_DEV uint32_t rtk_rec_to_string(const RCtx& c, uint64_t h, char* dst) {
    const RegionScratch& s = *rtk_u(c.sc);
    return rtk_ums_to_string(c, rtk_path_ums(s, rtk_h_lvl(h), rtk_h_off(h)), rtk_rec_n(s, h), dst);
}

#endif
