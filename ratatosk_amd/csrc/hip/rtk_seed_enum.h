// Anchor stage, 1-edit k-mer search by enumeration (src/Graph.cpp:193, Bifrost searchSequence inexact [A2]): RTK_INEXACT_ENUM=1 cross-check, and the fallback when
// the half-k-mer index is not built. One wavefront owns one tile of 64 window positions.
#ifndef RTK_SEED_ENUM_H
#define RTK_SEED_ENUM_H

#include "rtk_seed_types.h"
#include "rtk_seed_window.h"
#include "rtk_types.h"
#include "rtk_wave.h"

// ---------------------------------------------------------------------------------------------- inexact probes (src/Graph.cpp:193 [A2])
// One tile = 64 consecutive base positions; every candidate window of the tile is expanded by the whole wave into its
// 93 substitution + 124 "insertion" + 29 "deletion" variants (one variant per lane per round), each probed in the k-mer table.
#define RTK_N_VARIANTS 246

// variant v (0..245) of the window whose first k-1 / k / k+1 characters are (w_k1, w_ck, w_ck1): 2-bit code of the graph k-mer to look for.
// The numbering is that of k = 31 (rtk_variant_kind keys on it); at a smaller k the variants whose offset the window does not have -- substitution and
// insertion offsets from k on, deletion offsets above k - 2 -- are not valid, so no shift count below goes negative.
RTK_DEV bool rtk_variant_code(int v, int k, uint64_t w_k1, uint32_t w_ck, uint32_t w_ck1, uint64_t* code_out) {
    uint64_t code = 0; bool valid = false;
    if (v < 93) { // substitution: needs k characters
        if (w_ck <= 3) {
            const int oo = v / 3, j = v % 3;
            if (oo >= k) { *code_out = 0; return false; }
            const uint64_t full = (w_k1 << 2) | w_ck;
            const int sh = 2 * (k - 1 - oo);
            const uint32_t orig = static_cast<uint32_t>((full >> sh) & 3ull);
            const uint32_t nb = static_cast<uint32_t>(j) + (static_cast<uint32_t>(j) >= orig ? 1u : 0u);
            code = (full & ~(3ull << sh)) | (static_cast<uint64_t>(nb) << sh); valid = true;
        }
    } else if (v < 217) { // graph k-mer has one extra base: k-1 read characters + an inserted one
        const int vv = v - 93, oo = vv / 4; const uint64_t nb = static_cast<uint64_t>(vv % 4);
        if (oo >= k) { *code_out = 0; return false; }
        const int rest = k - 1 - oo; // characters after the inserted base
        const uint64_t lo_mask = rest ? ((1ull << (2 * rest)) - 1ull) : 0ull;
        code = ((w_k1 >> (2 * rest)) << (2 * rest + 2)) | (nb << (2 * rest)) | (w_k1 & lo_mask); valid = true;
        // inserting b in front of a b spells the same k-mer as inserting it behind that b: only the last offset of such a run is probed
        // (the hits of a window are reduced to distinct k-mers anyway, src/Graph.cpp:201-216)
        if (rest >= 1 && ((w_k1 >> (2 * (rest - 1))) & 3ull) == nb) valid = false;
    } else if (v < RTK_N_VARIANTS) { // graph k-mer lacks one interior read base: k+1 read characters
        if (w_ck <= 3 && w_ck1 <= 3) {
            const int oo = v - 217 + 1; // deleted offset in [1, k-2]
            if (oo > k - 2) { *code_out = 0; return false; }
            const uint64_t full2 = (w_k1 << 4) | (static_cast<uint64_t>(w_ck) << 2) | static_cast<uint64_t>(w_ck1); // k+1 characters (exactly 64 bits for k = 31)
            const int keep_lo = k - oo; // characters after the deleted one
            const uint64_t lo_mask = (1ull << (2 * keep_lo)) - 1ull;
            const uint64_t hi = (2 * (keep_lo + 1) >= 64) ? 0ull : (full2 >> (2 * (keep_lo + 1)));
            code = (hi << (2 * keep_lo)) | (full2 & lo_mask); valid = true;
            // deleting either of two equal neighbours spells the same k-mer: only the last offset of a run is probed
            if (oo <= k - 3 && ((full2 >> (2 * (k - oo))) & 3ull) == ((full2 >> (2 * (k - oo - 1))) & 3ull)) valid = false;
        }
    }
    *code_out = code & ((k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull));
    return valid;
}

RTK_DEV uint32_t rtk_variant_kind(int v) { return v < 93 ? RTK_EDIT_SUB : (v < 217 ? RTK_EDIT_INS : RTK_EDIT_DEL); }
RTK_FN void rtk_inexact_tile(const GraphView& g, const BatchView& bv, uint64_t tile, unsigned long long* acc_probes, unsigned long long* acc_slots, unsigned long long* acc_hits, PoolChunk* chunk, uint32_t exclusive) {
    const int k = g.k;
#ifdef RTK_SIM
    const int n_sub = 64;
#else
    const int n_sub = 1;
#endif
    const uint64_t* const roff = bv.roff; const uint32_t n_reads = bv.n_reads;
    const unsigned char* const text = reinterpret_cast<const unsigned char*>(bv.masked.get());
    const uint32_t lo_tile = rtk_owner_read(roff, n_reads, tile * 64); // one scalar search per tile: largest r with roff[r] <= first base of the tile
    for (int sub = 0; sub < n_sub; ++sub) { // the 1-lane simulator visits the 64 positions of the tile one after the other
#ifdef RTK_SIM
        const uint64_t bb = tile * 64 + static_cast<uint64_t>(sub);
#else
        const uint64_t bb = tile * 64 + static_cast<uint64_t>(rtk_lane());
#endif
        // per-lane: is the window starting at bb a candidate? how many usable characters follow (k-1, k or k+1)?
        const RtkWinCode w = rtk_window_code(bv, roff, n_reads, lo_tile, text, k, bb);
        const uint64_t c_k1 = w.c_k1; const uint32_t ck = w.ck, ck1 = w.ck1;
        uint64_t bal = rtk_ballot(w.cand);
        // appends the `total` hits of window w_b (lane-local lists my_code / my_hit, my_n entries) to the raw-hit pool
        auto emit = [&](uint64_t w_b, int total, const uint64_t* my_code, const uint64_t* my_hit, int my_n, uint32_t probes, uint32_t slots) {
            if (total > 0) {
                const unsigned long long pbase = rtk_pool_take(bv, chunk, total);
                if (pbase + static_cast<unsigned long long>(total) <= bv.ipool_cap) {
                    int tot2; const int off = rtk_wave_excl_scan(my_n, &tot2);
                    for (int i = 0; i < my_n; ++i) { bv.ipool[2 * (pbase + off + i)] = my_code[i]; bv.ipool[2 * (pbase + off + i) + 1] = my_hit[i]; }
                    if (rtk_lane() == 0) bv.wdesc[w_b] = (static_cast<uint64_t>(pbase) << 24) | static_cast<uint64_t>(total);
                } else if (rtk_lane() == 0) rtk_atomic_add(bv.counters + RTK_CNT_OVERFLOW, 1ull);
            }
            *acc_slots += slots;
            *acc_probes += probes; // per-lane tallies, reduced once per wave at kernel end (a device-wide atomic per window saturates one L2 word)
            if (rtk_lane() == 0) *acc_hits += static_cast<unsigned long long>(total);
        };
#ifdef RTK_SIM
        while (bal) { // simulator: one lane walks all variants of its window
            bal &= bal - 1ull;
            uint64_t sim_code[RTK_N_VARIANTS], sim_hit[RTK_N_VARIANTS]; uint32_t sim_kind[RTK_N_VARIANTS]; int total = 0; uint32_t probes = 0, slots = 0, any = 0;
            for (int v = 0; v < RTK_N_VARIANTS; ++v) {
                uint64_t code; uint64_t hit = RTK_NO_HIT;
                if (rtk_variant_code(v, k, c_k1, ck, ck1, &code)) { uint32_t np; hit = rtk_find_kmer(g, code, &np); probes += 1; slots += np; }
                if (hit != RTK_NO_HIT) { sim_code[total] = code; sim_hit[total] = hit; sim_kind[total] = rtk_variant_kind(v); any |= sim_kind[total]; ++total; }
            }
            if (exclusive && total) { const uint32_t keep = rtk_a2_keep(any, exclusive); int w2 = 0; for (int i = 0; i < total; ++i) if (sim_kind[i] & keep) { sim_code[w2] = sim_code[i]; sim_hit[w2] = sim_hit[i]; ++w2; } total = w2; }
            emit(bb, total, sim_code, sim_hit, total, probes, slots);
        }
#else
        // Two-stage software pipeline over the candidate windows of the tile. Per window: four rounds of 64 variants; all four
        // pre-filter words are requested together, then the first table slot (key + value, one 16-byte read) of every variant that
        // passes. Those slot reads stay in flight while the NEXT window's variants are generated and its filter words requested.
        // (Two stages, not three: DESIGN_HISTORY.md, "Seed stage: what the comments used to tell".)
        // A window in flight is remembered by its three scalar words; the k-mers of the few variants that pass the filter are spelled
        // again when their slot arrives, so that only the slot contents wait in vector registers.
        struct Win { uint64_t w_b, w_k1; uint32_t w_ck, w_ck1; };
        const uint64_t* const ht = g.ht; const uint64_t ht_slots = g.ht_slots; const uint64_t* const bf = g.bf; const uint64_t bf_mask = g.bf_mask; const uint64_t* const bf1 = g.bf1; const uint64_t bf1_mask = g.bf1_mask;
        auto stage_probe = [&](Win& wn, uint32_t& pass, uint64_t* skey, uint64_t* sval) { // takes the next candidate off `bal`
            const int sl = rtk_ffs(bal) - 1;
            bal &= bal - 1ull;
            wn.w_k1 = rtk_u(rtk_shfl(c_k1, sl)); wn.w_ck = rtk_u(rtk_shfl(ck, sl)); wn.w_ck1 = rtk_u(rtk_shfl(ck1, sl));
            wn.w_b = tile * 64 + static_cast<uint64_t>(sl);
            uint64_t hh[4], word[4]; bool valid[4], valid1[4]; uint32_t probes = 0;
            for (int rr = 0; rr < 4; ++rr) {
                uint64_t code, can; uint32_t q;
                valid[rr] = rtk_variant_code(rtk_lane() + 64 * rr, k, wn.w_k1, wn.w_ck, wn.w_ck1, &code);
                rtk_kmer_prepare(code, k, &can, &hh[rr], &q);
                probes += valid[rr] ? 1u : 0u;
            }
            // first-level bit (L2 resident), then the filter word only for the variants whose bit is set
            uint64_t w1[4];
            for (int rr = 0; rr < 4; ++rr) w1[rr] = valid[rr] ? bf1[((hh[rr] >> 12) & bf1_mask) >> 6] : 0ull;
            for (int rr = 0; rr < 4; ++rr) valid1[rr] = valid[rr] && rtk_filter1_pass(w1[rr], hh[rr], bf1_mask);
            for (int rr = 0; rr < 4; ++rr) word[rr] = valid1[rr] ? bf[(hh[rr] >> 32) & bf_mask] : 0ull;
            *acc_probes += probes; // per-lane tallies, reduced once per wave at kernel end (a device-wide atomic per window saturates one L2 word)
            pass = 0;
            for (int rr = 0; rr < 4; ++rr) {
                const bool ps = valid1[rr] && rtk_filter_pass(word[rr], hh[rr]);
                skey[rr] = RTK_EMPTY_KEY; sval[rr] = 0;
                if (ps) { pass |= 1u << rr; const uint64_t* sp = ht + 2 * rtk_ht_slot(hh[rr], ht_slots); skey[rr] = sp[0]; sval[rr] = sp[1]; }
            }
        };
        auto stage_resolve = [&](const Win& wn, uint32_t pass, const uint64_t* skey, const uint64_t* sval) {
            uint64_t my_code[4]; uint64_t my_hit[4]; uint32_t my_kind[4]; int my_n = 0; uint32_t slots = 0; int total = 0; uint32_t any = 0;
            for (int rr = 0; rr < 4; ++rr) {
                uint64_t hit = RTK_NO_HIT; uint64_t code = 0;
                if ((pass >> rr) & 1u) {
                    uint64_t can, hh; uint32_t q;
                    rtk_variant_code(rtk_lane() + 64 * rr, k, wn.w_k1, wn.w_ck, wn.w_ck1, &code);
                    rtk_kmer_prepare(code, k, &can, &hh, &q);
                    slots += 1;
                    if (skey[rr] == can) hit = rtk_pack_hit(static_cast<uint32_t>(sval[rr] >> 32), static_cast<uint32_t>((sval[rr] & 0xFFFFFFFFull) >> 1), (static_cast<uint32_t>(sval[rr] & 1ull) == q) ? 1u : 0u);
                    else if (skey[rr] != RTK_EMPTY_KEY) { uint32_t np; hit = rtk_table_probe_from(g, can, rtk_ht_next(rtk_ht_slot(hh, ht_slots), ht_slots), q, &np); slots += np; } // collision: keep probing from the next slot
                }
                const uint64_t hb = rtk_ballot(hit != RTK_NO_HIT);
                if (hit != RTK_NO_HIT) { my_code[my_n] = code; my_hit[my_n] = hit; my_kind[my_n] = rtk_variant_kind(rtk_lane() + 64 * rr); any |= my_kind[my_n]; ++my_n; }
                total += rtk_popc(hb);
            }
            if (exclusive && total) { // [A2] exclusive: only the hits of the first kind of edit (substitution -> insertion -> deletion) that has one in this window
                for (int o = 32; o > 0; o >>= 1) any |= static_cast<uint32_t>(__shfl_xor(static_cast<int>(any), o, 64));
                const uint32_t keep = rtk_a2_keep(any, exclusive);
                int w2 = 0; for (int i = 0; i < my_n; ++i) if (my_kind[i] & keep) { my_code[w2] = my_code[i]; my_hit[w2] = my_hit[i]; ++w2; }
                my_n = w2; total = rtk_wave_sum(my_n);
            }
            emit(wn.w_b, total, my_code, my_hit, my_n, 0u, slots);
        };
        if (bal) {
            Win cur; uint32_t pass; uint64_t skey[4], sval[4];
            stage_probe(cur, pass, skey, sval);
            while (bal) {
                Win nxt; uint32_t npass; uint64_t nkey[4], nval[4];
                stage_probe(nxt, npass, nkey, nval);   // next window: filter words, then its slots, on their way ...
                stage_resolve(cur, pass, skey, sval);  // ... while this window's slots (requested a window ago) are compared
                cur = nxt; pass = npass;
                for (int rr = 0; rr < 4; ++rr) { skey[rr] = nkey[rr]; sval[rr] = nval[rr]; }
            }
            stage_resolve(cur, pass, skey, sval);
        }
#endif
    }
}

#endif
