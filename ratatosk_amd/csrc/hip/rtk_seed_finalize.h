// Anchor stage, finalize: solid/weak split (src/Graph.cpp:201-219), overlap filter (:221-239), keep_non_overlap (src/Alignment.cpp:1017-1199) and the adjacent-run
// consistency check (:329-372). One wavefront owns one long read.
#ifndef RTK_SEED_FINALIZE_H
#define RTK_SEED_FINALIZE_H

#include "rtk_colour_sets.h"
#include "rtk_acgt.h"
#include "rtk_seed_mask.h" // rtk_hit_bits
#include "rtk_seed_types.h"
#include "rtk_sets.h"
#include "rtk_types.h"
#include "rtk_wave.h"

// ---------------------------------------------------------------------------------------------- finalize (src/Graph.cpp:201-372)
RTK_DEV bool rtk_char_eq_base(char c, uint32_t b) { return rtk_cls(static_cast<unsigned char>(c)) == static_cast<int>(b); }

// classification of one weak hit (src/Alignment.cpp:1049-1072): returns key or 0 when the hit is dropped
RTK_FN uint64_t rtk_weak_key(const char* ref, uint32_t pos, uint64_t code, int k) {
    // the k read characters as 2-bit codes next to the graph k-mer `code`; a character that is not A/C/G/T equals nothing (inv)
    int n_ok; uint64_t inv;
    const uint64_t R = rtk_pack_acgt(reinterpret_cast<const unsigned char*>(ref) + pos, k, &n_ok, &inv);
    const uint64_t even = 0x5555555555555555ull;
    const uint64_t mk = (k < 32) ? ((1ull << (2 * k)) - 1ull) : ~0ull, mk1 = (1ull << (2 * (k - 1))) - 1ull;
    auto neq = [&](uint64_t x) -> uint64_t { return (x | (x >> 1)) & even; }; // one bit (the low one of its pair) per differing character
    // character i sits at bits [2(k-1-i), 2(k-1-i)+1]
    const uint64_t d0 = (neq(code ^ R) | inv) & mk;                 // read[i] != kmer[i]
    const int l = d0 ? (__builtin_clzll(d0) - (64 - 2 * k)) / 2 : k; // first differing position
    if (l >= k) return 0;
    const uint64_t below = (l + 1 < k) ? ((1ull << (2 * (k - 1 - l))) - 1ull) : 0ull; // characters after position l (k-character layout)
    int type_var = 0; uint32_t mis = 0;
    const uint32_t ql = static_cast<uint32_t>((code >> (2 * (k - 1 - l))) & 3ull);
    if ((d0 & below) == 0) { type_var = 1; mis = 1u << ql; }        // read[i] == kmer[i] for every i > l
    if (!type_var) { // read[l + i] == kmer[l + 1 + i]: the read without the k-mer's character l; compare kmer[1..k) with read[0..k-1) from position l on
        const uint64_t d = (neq((code & mk1) ^ (R >> 2)) | (inv >> 2)) & mk1; // (k-1)-character layout: index j <-> read[j] vs kmer[j+1], bits 2(k-2-j)
        const uint64_t from_l = (l < k - 1) ? ((1ull << (2 * (k - 1 - l))) - 1ull) : 0ull; // indices j >= l
        if ((d & from_l) == 0) { type_var = 2; mis = 1u << ql; }
    }
    if (!type_var) { // read[l + 1 + i] == kmer[l + i]: compare kmer[0..k-1) with read[1..k) from position l on
        const uint64_t d = (neq((code >> 2) ^ (R & mk1)) | (inv & mk1)) & mk1; // index j <-> kmer[j] vs read[j+1], bits 2(k-2-j)
        const uint64_t from_l = (l < k - 1) ? ((1ull << (2 * (k - 1 - l))) - 1ull) : 0ull;
        if ((d & from_l) == 0) type_var = 3;
    }
    if (type_var == 0 || l == 0 || l == k - 1) return 0;
    return (static_cast<uint64_t>(pos + static_cast<uint32_t>(l)) << 16) | (static_cast<uint64_t>(mis) << 8) | static_cast<uint64_t>(type_var);
}

// phase 3 (gather, in rtk_finalize_read) works on RTK_GQ chunks of 64 windows per step and writes the first hits of RTK_GH of them at a time
#ifdef RTK_SIM
#define RTK_GQ 2
#define RTK_GH 1
#else
#ifndef RTK_GQ_N
#define RTK_GQ_N 4
#endif
#ifndef RTK_GH_N
#define RTK_GH_N 4
#endif
#define RTK_GQ RTK_GQ_N
#define RTK_GH RTK_GH_N
static_assert(RTK_GQ % RTK_GH == 0, "a step is a whole number of halves");
#endif

// ---- phase 1, solid = exact hits minus runs that overlap the next run by less than k (src/Graph.cpp:221-239) -> n1 candidates in s_pos ----
// hit x (run end e, next hit nx after the gap) is dropped iff nx < x + k.
// In bits: with b = presence of the k-1 windows after x (bit 0 = x+1), x is dropped iff b has a one above its first zero,
// i.e. iff b & (b + 1) != 0. One ballot per 64 windows gives the presence bits; each lane looks at its own and the next block's.
RTK_DEV uint32_t rtk_fin_solid(const uint64_t* hmap, uint64_t base, uint32_t nwin, uint32_t k, uint32_t* s_pos) {
    uint32_t n1 = 0;
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    for (uint32_t cc = 0; cc < nwin; cc += 64 * RTK_WAVE) { // one 64-window block (and its successor) per lane, fetched together
        const uint32_t my_c0 = cc + 64u * lane;
        const uint64_t my_cur = (my_c0 < nwin) ? rtk_hit_bits(hmap, base + my_c0, nwin - my_c0) : 0ull;
        const uint64_t my_nxt = (my_c0 + 64 < nwin) ? rtk_hit_bits(hmap, base + my_c0 + 64, nwin - my_c0 - 64) : 0ull;
#ifndef RTK_SIM
        { // Every lane judges the 64 windows of ITS block with 128-bit shifts: window x is dropped iff a run of hits STARTS at x + 2 .. x + k - 1 (a one above a
          // zero in the presence bits behind x), i.e. iff the run starts T, OR-ed over a sliding window of k - 2 positions (doubling), have a bit at x + 2.
            const uint64_t Tl = my_cur & ~(my_cur << 1), Th = my_nxt & ~((my_nxt << 1) | (my_cur >> 63)); // (a start at bit 0 or 1 of the block is never asked for)
            uint64_t Rl = Tl, Rh = Th; uint32_t have = 1; const uint32_t w = k - 2;
            auto or_shifted = [&](uint32_t sft) { const uint64_t sl = (Rl >> sft) | (Rh << (64u - sft)), sh = Rh >> sft; Rl |= sl; Rh |= sh; }; // 0 < sft < 64
            while (2u * have <= w) { or_shifted(have); have *= 2u; }
            if (have < w) or_shifted(w - have);
            const uint64_t keep = my_cur & ~((Rl >> 2) | (Rh << 62));
            int total = 0; const uint32_t off = static_cast<uint32_t>(rtk_wave_excl_scan(rtk_popc(keep), &total));
            uint32_t o = n1 + off;
            for (uint64_t m = keep; m; m &= m - 1ull) s_pos[o++] = my_c0 + static_cast<uint32_t>(__builtin_ctzll(m));
            n1 += static_cast<uint32_t>(rtk_u(total));
        }
#else
        const uint64_t kmask = (1ull << (k - 1)) - 1ull;
        for (int bl = 0; bl < RTK_WAVE; ++bl) {
            const uint32_t c0 = cc + 64u * static_cast<uint32_t>(bl);
            if (c0 >= nwin) break;
            const uint64_t cur = rtk_u(rtk_shfl(my_cur, bl)), nxt = rtk_u(rtk_shfl(my_nxt, bl));
            if (cur == 0) continue;
            for (uint32_t j = 0; j < 64; ++j) { // the 1-lane simulator walks the 64 windows of the block
                if (!((cur >> j) & 1ull)) continue;
                const uint64_t after = (j == 63) ? nxt : ((cur >> (j + 1)) | (nxt << (63 - j))); // bits x+1 .. x+k-1 of the 128-bit presence string (k - 1 <= 62)
                const uint64_t b = after & kmask;
                if ((b & (b + 1ull)) == 0) s_pos[n1++] = c0 + j;
            }
        }
#endif
    }
    rtk_sync();
    return n1;
}

// ---- phase 2, junction: adjacent solid anchors on different unitigs must be graph neighbours sharing >= min_cov colours (:329-372) -> n2 solid anchors in s_pos ----
// A junction = two solid anchors at adjacent positions on different unitigs. The verdict on one only depends on its two unitigs, the
// emptiness flags it leaves behind carry on to later junctions. This kernel lasts as long as the longest read of the ticket (tens of
// thousands of solid anchors, hundreds of junctions, one every other 64-anchor chunk), so nothing here may cost a memory round trip per
// chunk or per junction: (1) the junctions are gathered into a list, four chunks of anchors in flight per step; (2) they are judged 64 at
// a time, one per lane (adjacency words and colour sets of 64 pairs read side by side); (3) only the invalid ones -- a handful -- are then
// visited in order to spread their flags (a valid junction changes nothing, whatever the flags around it say).
// emptied[i] = 1: candidate i is dropped; jl: the junction list (index of the right anchor, bit 63 = invalid), jcap entries
RTK_DEV uint32_t rtk_fin_junctions(const GraphView& g, uint32_t min_cov, const uint64_t* hits, uint32_t* s_pos, uint32_t n1, uint8_t* emptied, uint64_t* jl, uint32_t jcap) {
    for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < n1; i += RTK_WAVE) emptied[i] = 0; // 1 = emptied
    rtk_sync();
    uint32_t nj = 0;
    auto flush = [&]() {
        rtk_sync();
        for (uint32_t j0 = 0; j0 < nj; j0 += RTK_WAVE) { // (2)
            const uint32_t j = j0 + static_cast<uint32_t>(rtk_lane());
            if (j < nj) {
                const uint32_t ii = static_cast<uint32_t>(jl[j]);
                const UMap ul = rtk_unpack_hit(hits[s_pos[ii - 1]]), ur = rtk_unpack_hit(hits[s_pos[ii]]);
                // right unitig must be the successor of the left one in walk direction (tail/head k-1 overlap) ...
                bool inv = true;
                const uint32_t* a = g.adj + 8ull * ul.unitig + (ul.strand ? 0 : 4);
                for (int bb = 0; bb < 4; ++bb) if (a[bb] != RTK_NONE32 && (a[bb] >> 1) == ur.unitig && (a[bb] & 1u) == ur.strand) inv = false;
                // ... and share enough colours
                if (!inv) inv = rtk_lane_shared_unitigs(g, ul.unitig, ur.unitig, min_cov) < min_cov;
                if (inv) jl[j] |= 1ull << 63;
            }
        }
        rtk_sync();
        for (uint32_t j0 = 0; j0 < nj; j0 += RTK_WAVE) { // (3)
            const uint32_t j = j0 + static_cast<uint32_t>(rtk_lane());
            const uint64_t e = j < nj ? jl[j] : 0ull;
            uint64_t bad = rtk_ballot((e >> 63) != 0);
            while (bad) {
                const int l = rtk_ffs(bad) - 1; bad &= bad - 1ull;
                const uint32_t ii = static_cast<uint32_t>(rtk_u(rtk_shfl(e, l)));
                if (emptied[ii - 1] || emptied[ii]) continue;
                const UMap ul = rtk_unpack_hit(hits[s_pos[ii - 1]]), ur = rtk_unpack_hit(hits[s_pos[ii]]);
                uint32_t i_l = ii - 1, i_r = ii + 1;
                i_l -= (i_l != 0) ? 1u : 0u;
                while (i_l > 0 && s_pos[i_l] == s_pos[i_l + 1] - 1 && rtk_hit_unitig(hits[s_pos[i_l]]) == ul.unitig) { emptied[i_l] = 1; --i_l; }
                while (i_r < n1 && s_pos[i_r] == s_pos[i_r - 1] + 1 && rtk_hit_unitig(hits[s_pos[i_r]]) == ur.unitig) { emptied[i_r] = 1; ++i_r; }
                emptied[ii - 1] = 1; emptied[ii] = 1;
                rtk_sync();
            }
        }
        nj = 0;
    };
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    for (uint32_t c0 = 1; c0 < n1; c0 += 4 * RTK_WAVE) { // (1)
        if (nj + 4u * RTK_WAVE > jcap) flush();
        uint32_t p[4], q[4]; uint64_t hp[4], hq[4]; bool cand[4];
        for (int x = 0; x < 4; ++x) { const uint32_t i = c0 + static_cast<uint32_t>(x) * RTK_WAVE + lane; p[x] = q[x] = 0; if (i < n1) { p[x] = s_pos[i]; q[x] = s_pos[i - 1]; } }
        for (int x = 0; x < 4; ++x) { const uint32_t i = c0 + static_cast<uint32_t>(x) * RTK_WAVE + lane; cand[x] = i < n1 && p[x] - q[x] == 1; hp[x] = hq[x] = 0; if (cand[x]) { hp[x] = hits[p[x]]; hq[x] = hits[q[x]]; } }
        for (int x = 0; x < 4; ++x) {
            const bool c = cand[x] && rtk_hit_unitig(hp[x]) != rtk_hit_unitig(hq[x]);
            const uint64_t bal = rtk_ballot(c);
            if (c) jl[nj + static_cast<uint32_t>(rtk_popc(bal & ((1ull << lane) - 1ull)))] = c0 + static_cast<uint32_t>(x) * RTK_WAVE + lane;
            nj += static_cast<uint32_t>(rtk_popc(bal));
        }
    }
    flush();
    rtk_sync();
    uint32_t n2 = 0;
    for (uint32_t c0 = 0; c0 < n1; c0 += RTK_WAVE) { // in-place compaction (write index never passes read index)
        const uint32_t i = c0 + static_cast<uint32_t>(rtk_lane());
        const bool keep = i < n1 && !emptied[i];
        const uint32_t v = keep ? s_pos[i] : 0;
        const uint64_t bal = rtk_ballot(keep);
        rtk_sync();
        if (keep) s_pos[n2 + static_cast<uint32_t>(rtk_popc(bal & ((1ull << rtk_lane()) - 1ull)))] = v;
        n2 += static_cast<uint32_t>(rtk_popc(bal));
    }
    rtk_sync();
    return n2;
}

// ---- phases 4 - 7: keep_non_overlap (src/Alignment.cpp:1017-1199) ----
// NB: an inexact hit is never "solid": its mapped k-mer differs from the read window by construction.
// phase 4, classify + sort: the hits that rtk_weak_key classifies, sorted by key -> nvalid of them in skey (key) / sidx (index of the hit); vflag cleared.
// Ka, Ia, Kb, Ib: the 32-bit key / index buffers of the radix sort.
RTK_DEV uint32_t rtk_fin_classify_sort(const char* ref, uint32_t L, uint32_t k, uint32_t nv, const uint32_t* vpos, const uint64_t* vcode, uint8_t* vflag, uint64_t* skey, uint64_t* sidx,
                                       uint32_t* Ka, uint32_t* Ia, uint32_t* Kb, uint32_t* Ib) {
    uint32_t nvalid = 0;
#ifndef RTK_SIM
    if (nv > RTK_LDS_SORT_CAP && L < (1u << 26)) {
        // thousands of hits (the read that the launch waits for): the classified ones are compacted in hit order as (32-bit key, hit index) -- variant position,
        // base mask and kind of the 64-bit key side by side -- and sorted by a stable radix sort (three passes for a 100 kb read; the bitonic network of
        // rtk_sort_pairs on 8 192 pairs takes a third of that read's time); Ka .. Ib are the buffers
        const uint64_t lt = (1ull << rtk_lane()) - 1ull;
        for (uint32_t c0 = 0; c0 < nv; c0 += RTK_WAVE) {
            const uint32_t i = c0 + static_cast<uint32_t>(rtk_lane());
            uint64_t key = 0;
            if (i < nv) { key = rtk_weak_key(ref, vpos[i], vcode[i], static_cast<int>(k)); vflag[i] = 0; }
            const bool ok = key != 0;
            const uint64_t bal = rtk_ballot(ok);
            if (ok) { const uint32_t j = nvalid + static_cast<uint32_t>(rtk_popc(bal & lt)); Ka[j] = static_cast<uint32_t>(((key >> 16) << 6) | (((key >> 8) & 15ull) << 2) | (key & 3ull)); Ia[j] = i; }
            nvalid += static_cast<uint32_t>(rtk_popc(bal));
        }
        rtk_sync();
        rtk_radix_sort_pairs_u32(Ka, Ia, Kb, Ib, nvalid, (L << 6) | 63u);
        for (uint32_t j = static_cast<uint32_t>(rtk_lane()); j < nvalid; j += RTK_WAVE) {
            const uint32_t K = Ka[j];
            skey[j] = (static_cast<uint64_t>(K >> 6) << 16) | (static_cast<uint64_t>((K >> 2) & 15u) << 8) | static_cast<uint64_t>(K & 3u); sidx[j] = Ia[j];
        }
        rtk_sync();
    } else
#endif
    {
        for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < nv; i += RTK_WAVE) {
            const uint64_t key = rtk_weak_key(ref, vpos[i], vcode[i], static_cast<int>(k));
            skey[i] = key ? key : ~0ull; sidx[i] = i; vflag[i] = 0;
        }
        rtk_sync();
        rtk_sort_pairs(skey, sidx, nv);
        { // number of classified hits = first index with an all-ones key
            uint32_t lo = 0, hi = nv; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (skey[mid] == ~0ull) hi = mid; else lo = mid + 1; } nvalid = lo;
        }
    }
    return nvalid;
}

// phase 5, groups of equal key -> ng groups: first sorted index (gstart), size (gcnt), position span (gps, gpe), gkeep = 1, and one word each in ginfo -- the variant's
// position and, for a group of one hit, the unitig and strand of that hit -- so that the neighbour test of phase 6 reads a group with independent loads instead of three dependent ones
RTK_DEV uint32_t rtk_fin_groups(uint32_t nvalid, uint32_t k, const uint64_t* skey, const uint64_t* sidx, const uint32_t* vpos, const uint64_t* vhit,
                                uint32_t* gstart, uint32_t* gcnt, uint32_t* gps, uint32_t* gpe, uint8_t* gkeep, uint64_t* ginfo) {
    uint32_t ng = 0;
    for (uint32_t i0 = 0; i0 < nvalid; i0 += RTK_WAVE) { // group starts, compacted in order
        const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
        const bool st = i < nvalid && (i == 0 || skey[i] != skey[i - 1]);
        const uint64_t sb = rtk_ballot(st);
        if (st) gstart[ng + static_cast<uint32_t>(rtk_popc(sb & ((1ull << rtk_lane()) - 1ull)))] = i;
        ng += static_cast<uint32_t>(rtk_popc(sb));
    }
    rtk_sync();
    for (uint32_t gi = static_cast<uint32_t>(rtk_lane()); gi < ng; gi += RTK_WAVE) { // one group per lane: extent and position span
        const uint32_t a = gstart[gi], e = (gi + 1 < ng) ? gstart[gi + 1] : nvalid;
        uint32_t ps = 0xFFFFFFFFu, pe = 0;
        for (uint32_t j = a; j < e; ++j) { const uint32_t pp = vpos[sidx[j]]; ps = pp < ps ? pp : ps; pe = (pp + k) > pe ? (pp + k) : pe; }
        gcnt[gi] = e - a; gps[gi] = ps; gpe[gi] = pe; gkeep[gi] = 1;
        const uint64_t h0 = vhit[sidx[a]];
        ginfo[gi] = (((static_cast<uint64_t>(rtk_hit_unitig(h0)) << 1) | (h0 & 1ull)) << 32) | (skey[a] >> 16 & 0xFFFFFFFFull);
    }
    rtk_sync();
    return ng;
}

// phase 6, conflicts: a variant is dropped iff another variant overlaps it within k without sharing a unitig (order independent); vflag = 1 for the hits of the groups that stay
RTK_DEV void rtk_fin_conflicts(uint32_t ng, uint32_t k, uint32_t L, const uint64_t* ginfo, const uint32_t* gstart, const uint32_t* gcnt, const uint32_t* gps, const uint32_t* gpe, uint8_t* gkeep,
                               const uint64_t* sidx, const uint64_t* vhit, uint8_t* vflag) {
    for (uint32_t gi = static_cast<uint32_t>(rtk_lane()); gi < ng; gi += RTK_WAVE) {
        const uint64_t G1 = ginfo[gi]; const uint32_t p1 = static_cast<uint32_t>(G1 & 0xFFFFFFFFull);
        const uint32_t ps1 = gps[gi], pe1 = gpe[gi], c1 = gcnt[gi];
        const uint32_t lower = (p1 < k - 1) ? 0u : (p1 - k + 1); const uint32_t upper = ((p1 + k) >= L) ? L : (p1 + k);
        bool conflict = false;
        for (int dir = 0; dir < 2 && !conflict; ++dir) {
            int64_t gj = dir ? static_cast<int64_t>(gi) + 1 : static_cast<int64_t>(gi) - 1;
            while (gj >= 0 && gj < static_cast<int64_t>(ng) && !conflict) {
                const uint64_t G2 = ginfo[gj]; const uint32_t ps2 = gps[gj], pe2 = gpe[gj], c2 = gcnt[gj]; // (one round trip)
                const uint32_t p2 = static_cast<uint32_t>(G2 & 0xFFFFFFFFull);
                if (p2 < lower || p2 > upper) break;
                const bool ov1 = (p1 >= ps2) && (p1 < pe2);
                const bool ov2 = (p2 >= ps1) && (p2 < pe1);
                if (ov1 || ov2) {
                    bool same = false;
                    if (c1 == 1 && c2 == 1) same = (G1 >> 32) == (G2 >> 32);
                    else for (uint32_t a = 0; a < c1 && !same; ++a) {
                        const uint64_t ha = vhit[sidx[gstart[gi] + a]];
                        for (uint32_t b2 = 0; b2 < c2 && !same; ++b2) {
                            const uint64_t hb = vhit[sidx[gstart[gj] + b2]];
                            same = (rtk_hit_unitig(ha) == rtk_hit_unitig(hb)) && ((ha & 1ull) == (hb & 1ull));
                        }
                    }
                    if (!same) conflict = true;
                }
                gj += dir ? 1 : -1;
            }
        }
        if (conflict) gkeep[gi] = 0;
    }
    rtk_sync();
    for (uint32_t gi = static_cast<uint32_t>(rtk_lane()); gi < ng; gi += RTK_WAVE) if (gkeep[gi]) for (uint32_t a = 0; a < gcnt[gi]; ++a) vflag[sidx[gstart[gi] + a]] = 1;
    rtk_sync();
}

// phase 7, write: count, reserve space in the weak pool, write in original order -> n_keep anchors from *first on (0: none, or the pool is full and *overflow is set)
RTK_DEV uint32_t rtk_fin_write(const BatchView& bv, uint32_t nv, const uint8_t* vflag, const uint32_t* vpos, const uint64_t* vhit, uint32_t* overflow, unsigned long long* first) {
    uint32_t n_keep = 0;
    for (uint32_t c0 = 0; c0 < nv; c0 += RTK_WAVE) { const uint32_t i = c0 + static_cast<uint32_t>(rtk_lane()); n_keep += static_cast<uint32_t>(rtk_popc(rtk_ballot(i < nv && vflag[i]))); }
    if (n_keep) {
        unsigned long long wb = 0;
        if (rtk_lane() == 0) wb = rtk_atomic_add(bv.wk_top, static_cast<unsigned long long>(n_keep));
        wb = rtk_shfl(wb, 0);
        if (wb + n_keep > bv.wk_cap) { *overflow = 1; n_keep = 0; }
        else {
            uint32_t w = 0;
            for (uint32_t c0 = 0; c0 < nv; c0 += RTK_WAVE) {
                const uint32_t i = c0 + static_cast<uint32_t>(rtk_lane());
                const bool kp = i < nv && vflag[i];
                const uint64_t bal = rtk_ballot(kp);
                if (kp) { const uint64_t dst = wb + w + static_cast<uint32_t>(rtk_popc(bal & ((1ull << rtk_lane()) - 1ull))); bv.wk_pos[dst] = vpos[i]; bv.wk_hit[dst] = vhit[i]; }
                w += static_cast<uint32_t>(rtk_popc(bal));
            }
            *first = wb;
        }
    }
    return n_keep;
}

// One read: the seven phases in order, RTK_PHASE() closing each (slot i of RTK_CNT_FINALIZE; a read without weak hits closes four). Which SeedScratch buffer serves which phase
// under which name: the table at SeedScratch (rtk_seed_types.h). Phase 3 stands here and not in a function of its own: inlined from one, whatever its parameters, it costs
// k_finalize four more callee-saved registers, 232 instead of 216 bytes of scratch per lane (profiles/seed_stage_names.txt).
RTK_FN void rtk_finalize_read(const GraphView& g, const OptsView& o, const BatchView& bv, const SeedScratch& sc, uint32_t r) {
    RTK_ASSUME_LDS(&sc);
    const uint64_t base = bv.roff[r];
    const uint32_t L = static_cast<uint32_t>(bv.roff[r + 1] - base);
    const uint32_t k = static_cast<uint32_t>(g.k);
    if (rtk_lane() == 0) { bv.n_solid[r] = 0; bv.w_cnt[r] = 0; bv.w_off[r] = 0; }
    if (L <= k) { rtk_sync(); return; }
    const uint32_t nwin = L - k + 1;
    unsigned long long tph[8]; int iph = 0; const unsigned long long tstart = rtk_clock(); unsigned long long tlast = tstart;
#define RTK_PHASE() { const unsigned long long tn_ = rtk_clock(); tph[iph++] = tn_ - tlast; tlast = tn_; }
    const uint64_t* hits = bv.hits + base;
    uint32_t* s_pos = bv.s_pos + base;
    const uint32_t n1 = rtk_fin_solid(bv.hitmap, base, nwin, k, s_pos);
    RTK_PHASE();
    const uint32_t n2 = rtk_fin_junctions(g, o.min_cov_vertices, hits, s_pos, n1, sc.sflag, sc.vkey, 2u * sc.v_cap + 512u);
    if (rtk_lane() == 0) bv.n_solid[r] = n2;
    RTK_PHASE();
    // ---- phase 3, gather: weak = raw inexact hits sorted by (pos, mapped k-mer), deduplicated (src/Graph.cpp:201-216) -> nv hits in vpos / vcode / vhit ----
    // 64 windows per step. Windows holding several raw hits are first sorted by k-mer and stripped of duplicates in place (one
    // window at a time, the whole wave on it); then every lane appends the hits of its own window at its prefix-sum offset.
    uint32_t nv = 0; bool ovf = false;
    // This loop runs on the ONE wave that owns the read, 1 500 chunks for a 100 kb read, and the launch lasts as long as its slowest read: nothing in it
    // may wait for memory once per chunk. (1) The descriptors of RTK_GQ chunks are fetched together, those of the next step BEFORE this step's chunks are
    // worked on; a chunk without raw hits -- most of them -- costs nothing more. (2) The hits of the next window with several raw hits are fetched before
    // the current one is ranked and written back. (3) A lane appends the hits of its window four at a time (four 16-byte loads in flight, then the stores).
    // The pointers are read from the launch's views once: behind every store the compiler would fetch them again.
    {
      const uint64_t* const wdesc = bv.wdesc.get() + base; uint64_t* const ipool = bv.ipool.get();
      uint32_t* const vpos = sc.vpos.get(); uint64_t* const vcode = sc.vcode.get(); uint64_t* const vhit = sc.vhit.get(); const uint32_t v_cap = sc.v_cap;
      const uint32_t lane_u = static_cast<uint32_t>(rtk_lane());
      uint64_t dn[RTK_GQ];
      for (int q = 0; q < RTK_GQ; ++q) { const uint32_t xx = static_cast<uint32_t>(q) * RTK_WAVE + lane_u; dn[q] = (xx < nwin) ? wdesc[xx] : 0ull; }
      for (uint32_t c4 = 0; c4 < nwin && !ovf; c4 += RTK_GQ * RTK_WAVE) {
        uint64_t d4[RTK_GQ];
        for (int q = 0; q < RTK_GQ; ++q) d4[q] = dn[q];
        { const uint32_t cn = c4 + RTK_GQ * RTK_WAVE; // (1)
          if (cn < nwin) for (int q = 0; q < RTK_GQ; ++q) { const uint32_t xx = cn + static_cast<uint32_t>(q) * RTK_WAVE + lane_u; dn[q] = (xx < nwin) ? wdesc[xx] : 0ull; } }
        // (a) the windows with several raw hits of all chunks of the step: duplicates out, in place
        uint32_t ucnt[RTK_GQ];
#pragma unroll
        for (int x4 = 0; x4 < RTK_GQ; ++x4) ucnt[x4] = (d4[x4] & 0xFFFFFFull) ? 1u : 0u;
#pragma unroll
        for (int x4 = 0; x4 < RTK_GQ; ++x4) {
          if (ovf) break;
          const uint64_t d = d4[x4];
          const uint64_t off = d >> 24; const uint32_t cnt = static_cast<uint32_t>(d & 0xFFFFFFull);
          uint64_t multi = rtk_ballot(cnt >= 2);
          if (!multi) continue;
          // (2) the group of the next window with several hits, one element per lane when it fits (w_cnt <= 64)
          uint64_t nkey = ~0ull, nval = ~0ull;
          auto fetch_group = [&](uint64_t m) { nkey = ~0ull; nval = ~0ull; if (!m) return; const int s2 = rtk_ffs(m) - 1; const uint64_t o2 = rtk_u(rtk_shfl(off, s2)); const uint32_t n2_ = rtk_u(rtk_shfl(cnt, s2));
                                               if (n2_ <= RTK_WAVE && lane_u < n2_) { nkey = ipool[2 * (o2 + lane_u)]; nval = ipool[2 * (o2 + lane_u) + 1]; } };
          fetch_group(multi);
          while (multi) {
            const int sl = rtk_ffs(multi) - 1;
            multi &= multi - 1ull;
            const uint64_t w_off = rtk_u(rtk_shfl(off, sl)); const uint32_t w_cnt = rtk_u(rtk_shfl(cnt, sl));
            const uint64_t key = nkey, val = nval;
            fetch_group(multi);
            if (w_cnt <= RTK_WAVE) { // the usual case: the group fits one element per lane -> rank by all-pairs comparison in registers, no scratch, no barrier
                const uint32_t li = lane_u;
                bool dup = false;
                for (uint32_t j = 0; j < w_cnt; ++j) { // is an equal k-mer ordered before mine? ((k-mer, hit, index) ascending, like the sort + first-of-run rule)
                    const uint64_t kj = rtk_shfl(key, static_cast<int>(j)), vj = rtk_shfl(val, static_cast<int>(j));
                    dup = dup || (kj == key && (vj < val || (vj == val && j < li)));
                }
                const bool uq = li < w_cnt && !dup;
                uint64_t ub = rtk_ballot(uq);
                const uint32_t nu = static_cast<uint32_t>(rtk_popc(ub));
                uint32_t pos = 0;
                while (ub) { const int j = rtk_ffs(ub) - 1; ub &= ub - 1ull; pos += (rtk_shfl(key, j) < key) ? 1u : 0u; }
                if (uq) { ipool[2 * (w_off + pos)] = key; ipool[2 * (w_off + pos) + 1] = val; }
                if (static_cast<int>(li) == sl) ucnt[x4] = nu;
                continue;
            }
            if (2ull * w_cnt > 2ull * sc.v_cap + 512ull) { ovf = true; break; } // vkey / vidx hold 2 * v_cap + 512 entries, the sort pads to a power of two
            for (uint32_t i = lane_u; i < w_cnt; i += RTK_WAVE) { sc.vkey[i] = ipool[2 * (w_off + i)]; sc.vidx[i] = ipool[2 * (w_off + i) + 1]; }
            rtk_sync();
            rtk_sort_pairs(sc.vkey, sc.vidx, w_cnt);
            uint32_t nu = 0; // first entry of every run of equal k-mers goes back to the front of the group
            for (uint32_t i0 = 0; i0 < w_cnt; i0 += RTK_WAVE) {
                const uint32_t i = i0 + lane_u;
                const bool uq = i < w_cnt && (i == 0 || sc.vkey[i] != sc.vkey[i - 1]);
                const uint64_t ub = rtk_ballot(uq);
                if (uq) { const uint64_t dst = w_off + nu + static_cast<uint32_t>(rtk_popc(ub & ((1ull << rtk_lane()) - 1ull))); ipool[2 * dst] = sc.vkey[i]; ipool[2 * dst + 1] = sc.vidx[i]; }
                nu += static_cast<uint32_t>(rtk_popc(ub));
            }
            rtk_sync();
            if (rtk_lane() == sl) ucnt[x4] = nu;
          }
        }
        if (ovf) break;
        rtk_sync(); // compacted groups are read back by their window's lane
        // (b) where every window's hits go: chunk after chunk, window after window
        uint32_t my_o[RTK_GQ]; uint32_t nv_step = nv; bool any = false;
#pragma unroll
        for (int x4 = 0; x4 < RTK_GQ; ++x4) { int tot = 0; const uint32_t mo = static_cast<uint32_t>(rtk_wave_excl_scan(static_cast<int>(ucnt[x4]), &tot)); my_o[x4] = nv_step + mo; nv_step += static_cast<uint32_t>(rtk_u(tot)); any = any || tot != 0; }
        if (!any) continue;
        if (nv_step > v_cap) { ovf = true; break; }
        // (c) the first hit of every window of the step: the loads of all chunks in flight, then the stores; (3) the further hits of a window four at a time
#pragma unroll
        for (int h0 = 0; h0 < RTK_GQ; h0 += RTK_GH) { // (half a step at a time: registers)
          uint64_t cc_[RTK_GH], hh_[RTK_GH];
#pragma unroll
          for (int x4 = 0; x4 < RTK_GH; ++x4) if (ucnt[h0 + x4]) { const uint64_t off = d4[h0 + x4] >> 24; cc_[x4] = ipool[2 * off]; hh_[x4] = ipool[2 * off + 1]; }
#pragma unroll
          for (int x4 = 0; x4 < RTK_GH; ++x4) if (ucnt[h0 + x4]) { const uint32_t o = my_o[h0 + x4]; vpos[o] = c4 + static_cast<uint32_t>(h0 + x4) * RTK_WAVE + lane_u; vcode[o] = cc_[x4]; vhit[o] = hh_[x4]; }
        }
#pragma unroll
        for (int x4 = 0; x4 < RTK_GQ; ++x4) {
          if (rtk_ballot(ucnt[x4] > 1) == 0) continue;
          const uint64_t off = d4[x4] >> 24; const uint32_t x = c4 + static_cast<uint32_t>(x4) * RTK_WAVE + lane_u;
          for (uint32_t i = 1; i < ucnt[x4]; i += 4) {
              uint64_t cc_[4], hh_[4];
              for (uint32_t j = 0; j < 4; ++j) if (i + j < ucnt[x4]) { cc_[j] = ipool[2 * (off + i + j)]; hh_[j] = ipool[2 * (off + i + j) + 1]; }
              for (uint32_t j = 0; j < 4; ++j) if (i + j < ucnt[x4]) { const uint32_t o = my_o[x4] + i + j; vpos[o] = x; vcode[o] = cc_[j]; vhit[o] = hh_[j]; }
          }
        }
        nv = nv_step;
      }
    }
    if (ovf) { *sc.overflow = 1; nv = 0; }
    rtk_sync();
    RTK_PHASE();
    if (nv) {
        const uint32_t nvalid = rtk_fin_classify_sort(bv.seq + base, L, k, nv, sc.vpos, sc.vcode, sc.vflag, sc.vkey, sc.vidx, sc.gstart.get(), sc.gcnt.get(), sc.gps.get(), sc.gpe.get());
        RTK_PHASE();
        uint64_t* const ginfo = sc.vcode.get(); // (free once the hits are classified)
        const uint32_t ng = rtk_fin_groups(nvalid, k, sc.vkey, sc.vidx, sc.vpos, sc.vhit, sc.gstart, sc.gcnt, sc.gps, sc.gpe, sc.gkeep, ginfo);
        RTK_PHASE();
        rtk_fin_conflicts(ng, k, L, ginfo, sc.gstart, sc.gcnt, sc.gps, sc.gpe, sc.gkeep, sc.vidx, sc.vhit, sc.vflag);
        RTK_PHASE();
        unsigned long long first = 0;
        const uint32_t n_keep = rtk_fin_write(bv, nv, sc.vflag, sc.vpos, sc.vhit, sc.overflow, &first);
        if (n_keep && rtk_lane() == 0) { bv.w_off[r] = first; bv.w_cnt[r] = n_keep; }
    }
    RTK_PHASE();
    if (rtk_lane() == 0) { // phase profile of the stage (wave cycles), read back under RTK_TRACE
        for (int i = 0; i < iph && i < 7; ++i) rtk_atomic_add(bv.counters + RTK_CNT_FINALIZE + i, tph[i]);
#ifndef RTK_SIM
        { const unsigned long long mine = rtk_clock() - tstart; const unsigned long long was = atomicMax(bv.counters.get() + RTK_CNT_FINALIZE_SLOWEST, mine);
          if (mine > was) for (int i = 0; i < iph && i < 7; ++i) bv.counters[RTK_CNT_FINALIZE_SLOWEST_PHASES + i] = tph[i]; } // (developer trace: the phases of the slowest read so far; races between two record holders are harmless)
#endif
    }
#undef RTK_PHASE
    rtk_sync();
}
#undef RTK_GQ
#undef RTK_GH

#endif
