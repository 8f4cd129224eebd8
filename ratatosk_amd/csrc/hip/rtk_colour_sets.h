// Colour sets of unitigs as the anchor and the region stage ask for them: the unitig of a hit, sizes of intersections (wave-wide and one pair per lane), the lowest
// shared ids, the running union of a walk, and the [D1] sort key of chooseColors. (rtk_colours.h and the region headers call these as well.)
#ifndef RTK_COLOUR_SETS_H
#define RTK_COLOUR_SETS_H

#include "rtk_seed_types.h"
#include "rtk_sets.h"
#include "rtk_types.h"
#include "rtk_wave.h"

RTK_DEV uint32_t rtk_hit_unitig(uint64_t h) { return static_cast<uint32_t>(h >> 33); }
RTK_DEV bool rtk_is_branching(const GraphView& g, uint32_t u) { return (g.flags[u] & RTK_F_BRANCHING) != 0; }


// min(|colours(u) & set|, cap)  (getNumberSharedPairID(SharedPairID, PairID), src/Common.cpp:73-83)
RTK_FN uint32_t rtk_shared_with_set(const GraphView& g_, uint32_t u_, const uint32_t* set_, uint32_t n_, uint32_t cap_) {
    const GraphView& g = *rtk_u(&g_); uint32_t u = rtk_u(u_); const uint32_t* set = rtk_u(set_); uint32_t n = rtk_u(n_); uint32_t cap = rtk_u(cap_);
    uint32_t shared = 0;
    const int32_t gi = g.gid[u];
    if (gi >= 0) shared = rtk_set_inter_count(g.col + g.goff[gi], static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]), set, n, cap);
    if (shared < cap) shared += rtk_set_inter_count(g.col + g.loff[u], static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]), set, n, cap - shared);
    return shared;
}

// The `want` lowest ids of colours(u) & set, ascending, into out; returns how many (< want when the intersection is smaller). This IS
// "(global & set) | (local & set), truncated to its `want` lowest ids" (chooseColors, src/Correction.cpp:372-390) without building
// either intersection: `set` is walked from its smallest id, 64 ids per step, and the walk stops as soon as `want` are found
// (want <= 30, the sets hold hundreds to thousands of ids).
RTK_FN uint32_t rtk_first_shared(const GraphView& g_, uint32_t u_, const uint32_t* set_, uint32_t n_, uint32_t want_, uint32_t* out_) {
    const GraphView& g = *rtk_u(&g_); uint32_t u = rtk_u(u_); const uint32_t* set = rtk_u(set_); uint32_t n = rtk_u(n_); uint32_t want = rtk_u(want_); uint32_t* out = rtk_u(out_);
    if (n == 0 || want == 0) return 0;
    const int32_t gi = g.gid[u];
    const uint32_t* gl = gi >= 0 ? g.col + g.goff[gi] : nullptr; const uint32_t ngl = gi >= 0 ? static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]) : 0u;
    const uint32_t* lo = g.col + g.loff[u]; const uint32_t nlo = static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]);
    if (ngl + nlo == 0) return 0;
#ifndef RTK_SIM
    uint32_t* const lds = rtk_lds_set_buf();
    const bool staged = (ngl + nlo) <= RTK_LDS_SET_CAP;
    if (staged) { for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < ngl + nlo; i += RTK_WAVE) lds[i] = i < ngl ? gl[i] : lo[i - ngl]; RTK_WG_SYNC(); }
#endif
    uint32_t found = 0;
    for (uint32_t i0 = 0; i0 < n && found < want; i0 += RTK_WAVE) {
        const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
        uint32_t x = 0; bool in = false;
        if (i < n) {
            x = set[i];
#ifndef RTK_SIM
            if (staged) in = rtk_lds_contains(lds, ngl, x) || rtk_lds_contains(lds + ngl, nlo, x); else
#endif
            in = (ngl && rtk_set_contains(gl, ngl, x)) || rtk_set_contains(lo, nlo, x);
        }
        const uint64_t bal = rtk_ballot(in);
        const uint32_t my = found + static_cast<uint32_t>(rtk_popc(bal & ((1ull << rtk_lane()) - 1ull)));
        if (in && my < want) out[my] = x;
        found += static_cast<uint32_t>(rtk_popc(bal));
    }
    rtk_sync();
    return found < want ? found : want;
}

// min(|colours(u) & colours(v)|, cap)  (getNumberSharedPairID(SharedPairID, SharedPairID), src/Common.cpp:51-71);
// global and local parts of one unitig are disjoint, so the four partial intersections add up
RTK_FN uint32_t rtk_shared_unitigs(const GraphView& g_, uint32_t u_, uint32_t v_, uint32_t cap_) {
    const GraphView& g = *rtk_u(&g_); uint32_t u = rtk_u(u_); uint32_t v = rtk_u(v_); uint32_t cap = rtk_u(cap_);
    const int32_t gu = g.gid[u], gv = g.gid[v];
    const uint32_t* lv = g.col + g.loff[v]; const uint32_t nlv = static_cast<uint32_t>(g.loff[v + 1] - g.loff[v]);
    if (gu >= 0 && gu == gv) {
        uint32_t shared = static_cast<uint32_t>(g.goff[gu + 1] - g.goff[gu]);
        if (shared < cap) shared += rtk_set_inter_count(g.col + g.loff[u], static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]), lv, nlv, cap - shared);
        return shared;
    }
    uint32_t shared = 0;
    if (gv >= 0) shared = rtk_shared_with_set(g, u, g.col + g.goff[gv], static_cast<uint32_t>(g.goff[gv + 1] - g.goff[gv]), cap);
    if (shared < cap) shared += rtk_shared_with_set(g, u, lv, nlv, cap - shared);
    return shared;
}

// The same count, one pair of unitigs PER LANE (no wave collectives): the junction filter of getSeeds evaluates its candidates 64 at a time.
// Sorted id arrays; the shorter is searched in the longer, the walk stops at `cap` matches.
RTK_DEV uint32_t rtk_lane_inter_count(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb, uint32_t cap) {
    if (na > nb) { const uint32_t* t = a; a = b; b = t; const uint32_t tn = na; na = nb; nb = tn; }
    uint32_t cnt = 0, lo = 0;
    for (uint32_t i = 0; i < na && cnt < cap && lo < nb; ++i) {
        const uint32_t x = a[i];
        uint32_t l = lo, h = nb;
        while (l < h) { const uint32_t m = (l + h) >> 1; if (b[m] < x) l = m + 1; else h = m; }
        lo = l;
        if (lo < nb && b[lo] == x) { ++cnt; ++lo; }
    }
    return cnt;
}
RTK_DEV uint32_t rtk_lane_shared_unitigs(const GraphView& g, uint32_t u, uint32_t v, uint32_t cap) { // min(|colours(u) & colours(v)|, cap), as rtk_shared_unitigs
    const int32_t gu = g.gid[u], gv = g.gid[v];
    const uint32_t* lu = g.col + g.loff[u]; const uint32_t nlu = static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]);
    const uint32_t* lv = g.col + g.loff[v]; const uint32_t nlv = static_cast<uint32_t>(g.loff[v + 1] - g.loff[v]);
    if (gu >= 0 && gu == gv) {
        const uint64_t ng = g.goff[gu + 1] - g.goff[gu];
        if (ng >= cap) return cap;
        return static_cast<uint32_t>(ng) + rtk_lane_inter_count(lu, nlu, lv, nlv, cap - static_cast<uint32_t>(ng));
    }
    const uint32_t* gul = gu >= 0 ? g.col + g.goff[gu] : nullptr; const uint32_t ngu = gu >= 0 ? static_cast<uint32_t>(g.goff[gu + 1] - g.goff[gu]) : 0u;
    const uint32_t* gvl = gv >= 0 ? g.col + g.goff[gv] : nullptr; const uint32_t ngv = gv >= 0 ? static_cast<uint32_t>(g.goff[gv + 1] - g.goff[gv]) : 0u;
    uint32_t shared = 0; // the four partial intersections add up (global and local part of one unitig are disjoint)
    if (ngu && ngv) shared += rtk_lane_inter_count(gul, ngu, gvl, ngv, cap);
    if (shared < cap && ngv && nlu) shared += rtk_lane_inter_count(lu, nlu, gvl, ngv, cap - shared);
    if (shared < cap && ngu && nlv) shared += rtk_lane_inter_count(gul, ngu, lv, nlv, cap - shared);
    if (shared < cap && nlu && nlv) shared += rtk_lane_inter_count(lu, nlu, lv, nlv, cap - shared);
    return shared;
}

// colours(u) = global | local, merged into the running union held in sc.set[cur]; returns new size (0xFFFFFFFF on overflow)
RTK_FN uint32_t rtk_union_unitig(const GraphView& g_, const SeedScratch& sc_, int& cur_, uint32_t n_cur_, uint32_t u_) {
    const GraphView& g = *rtk_u(&g_); const SeedScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); int& cur = *rtk_u(&cur_); uint32_t n_cur = rtk_u(n_cur_); uint32_t u = rtk_u(u_);
    const int32_t gi = g.gid[u];
    if (gi >= 0) {
        const uint32_t ng = static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]);
        if (n_cur + ng > sc.set_cap) { *sc.overflow = 1; return 0xFFFFFFFFu; }
        n_cur = rtk_set_union(sc.set[cur], n_cur, g.col + g.goff[gi], ng, sc.set[cur ^ 1], sc.set[2]);
        cur ^= 1;
    }
    const uint32_t nl = static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]);
    if (nl) {
        if (n_cur + nl > sc.set_cap) { *sc.overflow = 1; return 0xFFFFFFFFu; }
        n_cur = rtk_set_union(sc.set[cur], n_cur, g.col + g.loff[u], nl, sc.set[cur ^ 1], sc.set[2]);
        cur ^= 1;
    }
    return n_cur;
}

// [D1] sort key of a candidate anchor of chooseColors: (cardinality, unitig id), the id inverted for the descending reading; and the id back out of a key
RTK_DEV uint64_t rtk_d1_key(uint32_t card, uint32_t u, uint32_t desc) { return (static_cast<uint64_t>(card) << 32) | (desc ? (~u & 0xFFFFFFFFu) : u); }
RTK_DEV uint32_t rtk_d1_unitig(uint64_t key, uint32_t desc) { const uint32_t lo = static_cast<uint32_t>(key & 0xFFFFFFFFull); return desc ? ~lo : lo; }

#endif
