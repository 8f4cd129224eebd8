// Anchor stage, masking: the 'N'-masked copy of a read that the 1-edit search runs on (getSeeds, reference: src/Graph.cpp:102-191). One wavefront owns one segment
// of a long read.
#ifndef RTK_SEED_MASK_H
#define RTK_SEED_MASK_H

#include "rtk_colour_sets.h"
#include "rtk_seed_types.h"
#include "rtk_sets.h"
#include "rtk_wave.h"

// ---------------------------------------------------------------------------------------------- mask (src/Graph.cpp:102-191)
// presence bits of the 64 windows starting at global position g0 (bit j = window g0 + j), limited to the first n_valid of them
RTK_DEV uint64_t rtk_hit_bits(const uint64_t* map, uint64_t g0, uint64_t n_valid) {
    if (n_valid == 0) return 0ull;
    const uint64_t w0 = map[g0 >> 6], sh = g0 & 63ull;
    uint64_t bits = w0 >> sh;
    if (sh) bits |= map[(g0 >> 6) + 1] << (64ull - sh);
    return n_valid >= 64 ? bits : (bits & ((1ull << n_valid) - 1ull));
}

// Visits the exact hits at windows lo .. hi (inclusive, read coordinates) in ascending (dir > 0) or descending order and calls
// fn(unitig) at every change of unitig (src/Graph.cpp:127-183 walks the hits one by one and reacts to unitig changes only).
// 64 windows per step: presence bits from the bitmap, the hits of the set bits fetched by their lanes, changes found with a ballot.
template <class Fn>
RTK_DEV void rtk_scan_hit_runs(const uint64_t* hits, const uint64_t* hmap, uint64_t base, uint32_t nwin, int64_t lo, int64_t hi, int dir, Fn fn) {
    uint32_t prev_u = RTK_NONE32;
    if (hi >= static_cast<int64_t>(nwin)) hi = static_cast<int64_t>(nwin) - 1;
    if (lo < 0) lo = 0;
    for (int64_t done = 0; lo + done <= hi; done += RTK_WAVE) {
        const int64_t x = dir > 0 ? (lo + done + rtk_lane()) : (hi - done - rtk_lane());
        bool valid = x >= lo && x <= hi;
        if (valid) { const uint64_t g = base + static_cast<uint64_t>(x); valid = (hmap[g >> 6] >> (g & 63ull)) & 1ull; }
        uint32_t u = RTK_NONE32;
        if (valid) u = rtk_hit_unitig(hits[x]);
        const uint64_t m = rtk_ballot(valid);
        if (!m) continue;
        const uint64_t pm = m & ((1ull << rtk_lane()) - 1ull);
        const uint32_t up = rtk_shfl(u, pm ? (63 - __builtin_clzll(pm)) : 0);
        const uint32_t u_before = pm ? up : prev_u;
        uint64_t st = rtk_ballot(valid && (u_before == RTK_NONE32 || u != u_before));
        while (st) {
            const int l = rtk_ffs(st) - 1; st &= st - 1ull;
            if (!fn(rtk_u(rtk_shfl(u, l)))) return;
        }
        prev_u = rtk_u(rtk_shfl(u, 63 - __builtin_clzll(m)));
    }
}

// Windows [w_lo, w_hi) of read r (both multiples of the segment length, itself a multiple of 64 * RTK_WAVE; the kernel cuts long reads into such segments, one wave each: the launch lasted as
// long as the longest read of the ticket). The masked copy is all 'N' before the launch (seed_mask, rtk_seed_stage.inc), so that a segment may open a gap that reaches
// back into the segment before it. A gap [previous hit, p) belongs to the segment that holds its closing hit p; what the walk of src/Graph.cpp:127-183
// carries along -- the read's first hit and the last hit before the segment -- is read off the presence bits. The rule for the read's head is applied
// by the segment that holds the first hit, the rule for its tail by the last segment.
RTK_FN void rtk_mask_read(const GraphView& g, const OptsView& o, const BatchView& bv, const SeedScratch& sc, uint32_t r, uint32_t w_lo, uint32_t w_hi) {
    RTK_ASSUME_LDS(&sc);
    const uint64_t base = bv.roff[r];
    const uint32_t L = static_cast<uint32_t>(bv.roff[r + 1] - base);
    const uint32_t k = static_cast<uint32_t>(g.k);
    if (L <= k) return; // src/Graph.cpp:49
    const uint32_t nwin = L - k + 1;
    if (w_lo >= nwin) return;
    const bool last_seg = w_hi >= nwin;
    if (w_hi > nwin) w_hi = nwin;
    const uint64_t* hits = bv.hits + base;
    int64_t prev = -1, first = -1;
    const uint64_t* hmap = bv.hitmap;
    if (w_lo > 0) { // the first hit of the read and the last one before this segment
        for (uint32_t cc = 0; cc < w_lo && first < 0; cc += 64 * RTK_WAVE) {
            const uint32_t my_c0 = cc + 64u * static_cast<uint32_t>(rtk_lane());
            const uint64_t my_bits = (my_c0 < w_lo) ? rtk_hit_bits(hmap, base + my_c0, 64) : 0ull;
            const uint64_t any = rtk_ballot(my_bits != 0);
            if (any) { const int l = rtk_ffs(any) - 1; first = static_cast<int64_t>(cc) + 64 * l + __builtin_ctzll(rtk_u(rtk_shfl(my_bits, l))); }
        }
        for (uint32_t hi = w_lo; first >= 0 && hi > 0 && prev < 0; hi -= 64 * RTK_WAVE) { // blocks hi - 64, hi - 128, ...: lane 0 holds the nearest one
            const uint32_t my_c0 = hi - 64u * (static_cast<uint32_t>(rtk_lane()) + 1u);
            const uint64_t my_bits = rtk_hit_bits(hmap, base + my_c0, 64);
            const uint64_t any = rtk_ballot(my_bits != 0);
            if (any) { const int l = rtk_ffs(any) - 1; prev = static_cast<int64_t>(hi) - 64 * (l + 1) + 63 - __builtin_clzll(rtk_u(rtk_shfl(my_bits, l))); }
        }
    }
    const bool first_is_mine = first < 0;
    for (uint32_t cc = w_lo; cc < w_hi; cc += 64 * RTK_WAVE) { // every lane fetches the presence bits of one 64-window block, then the blocks are visited in order
        const uint32_t my_c0 = cc + 64u * static_cast<uint32_t>(rtk_lane());
        const uint64_t my_bits = (my_c0 < w_hi) ? rtk_hit_bits(hmap, base + my_c0, w_hi - my_c0) : 0ull;
      for (int bl = 0; bl < RTK_WAVE; ++bl) {
        const uint32_t c0 = cc + 64u * static_cast<uint32_t>(bl);
        if (c0 >= w_hi) break;
        uint64_t bal = rtk_u(rtk_shfl(my_bits, bl));
        if (bal == ~0ull && prev == static_cast<int64_t>(c0) - 1) { if (first < 0) first = c0; prev = c0 + 63; continue; } // inside a run: no gap
        // only the first hit of a run can close a gap: visit run starts, with `prev` = the last hit before each of them
        const uint64_t all_hits = bal; const int64_t prev_in = prev;
        uint64_t starts = bal & ~((bal << 1) | ((prev_in >= 0 && prev_in == static_cast<int64_t>(c0) - 1) ? 1ull : 0ull));
        if (all_hits) prev = static_cast<int64_t>(c0) + 63 - __builtin_clzll(all_hits);
        while (starts) {
            const int bit = rtk_ffs(starts) - 1;
            const uint32_t p = c0 + static_cast<uint32_t>(bit);
            starts &= starts - 1ull;
            const uint64_t below = all_hits & ((1ull << bit) - 1ull);
            const int64_t prev_hit = below ? (static_cast<int64_t>(c0) + 63 - __builtin_clzll(below)) : prev_in;
            if (prev_hit >= 0) {
                const uint32_t pv = static_cast<uint32_t>(prev_hit);
                const uint32_t diff = p - pv;
                bool unmask = false;
                if (diff >= o.insert_sz) unmask = true;
                else if (diff >= o.insert_sz / 2) {
                    const uint32_t ssl = o.insert_sz - diff;
                    const uint32_t min_pos_left = (pv < ssl) ? 0u : (pv - ssl);
                    const uint64_t max_pos_right = static_cast<uint64_t>(p) + ssl;
                    int cur = 0; uint32_t nL = 0, nR = 0; bool ovf = false;
                    // left of the gap: hits at pv, pv-1, ... above min_pos_left, stopping before the read's first hit (G13: index 0 is never visited)
                    const int64_t lb = (first > static_cast<int64_t>(min_pos_left)) ? first : static_cast<int64_t>(min_pos_left);
                    rtk_scan_hit_runs(hits, hmap, base, nwin, lb + 1, static_cast<int64_t>(pv), -1, [&](uint32_t u) {
                        if (!rtk_is_branching(g, u)) { nL = rtk_union_unitig(g, sc, cur, nL, u); if (nL == 0xFFFFFFFFu) { ovf = true; return false; } }
                        return true; });
                    if (!ovf) { // park the left union in set[3]
                        if (nL > sc.set_cap) ovf = true; else rtk_wcopy(sc.set[3], sc.set[cur], 4ull * nL);
                    }
                    cur = 0;
                    if (!ovf) rtk_scan_hit_runs(hits, hmap, base, nwin, static_cast<int64_t>(p), static_cast<int64_t>(max_pos_right) - 1, +1, [&](uint32_t u) {
                        if (!rtk_is_branching(g, u)) { nR = rtk_union_unitig(g, sc, cur, nR, u); if (nR == 0xFFFFFFFFu) { ovf = true; return false; } }
                        return true; });
                    if (!ovf) unmask = rtk_set_inter_count(sc.set[3], nL, sc.set[cur], nR, o.min_cov_vertices) < o.min_cov_vertices;
                }
                // two hits fewer than k windows apart (the rules above only let them through when the insert size is below 2 k): the reference's length diff - k
                // wraps around and std::string::replace cuts it off at the end of the read (src/Graph.cpp:115,124,182) -- everything behind the first hit's k-mer is opened
                if (unmask) rtk_wcopy(bv.masked + base + pv + k, bv.seq + base + pv + k, diff >= k ? diff - k : L - (pv + k));
            }
            if (first < 0) first = p;
        }
      }
    }
    if (first >= 0) {
        if (first_is_mine && static_cast<uint64_t>(first) >= o.insert_sz / 2) rtk_wcopy(bv.masked + base, bv.seq + base, static_cast<uint64_t>(first) + k - 1);
        if (last_seg && L - static_cast<uint64_t>(prev) >= o.insert_sz / 2) rtk_wcopy(bv.masked + base + prev + 1, bv.seq + base + prev + 1, L - static_cast<uint64_t>(prev) - 1);
    }
}

#endif
