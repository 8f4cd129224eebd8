// Around the region kernel: the programs of k_enum (the regions of a read, src/Correction.cpp:159-175 and the loop of :776-957 as
// descriptors), k_stitch and k_stitch_copy (the segments of a read put together, the `+=` of the same loop). One wave per read, except
// the copy (64 segments per wave).
#ifndef RTK_REGION_ENUM_H
#define RTK_REGION_ENUM_H

#include "rtk_region_types.h"

// ------------------------------------------------------------------------------------------------ region enumeration (one wave per read)
// dst[i] = tab[src[n - 1 - i]] (tab == nullptr: the characters as they are). One wave; four characters per lane and access (the reverse complement of a 64 Mb
// step was 0.7 of k_enum's 0.8 ms as byte loads, a twelve-way switch per character and byte stores: `tab` is the complement as a 256-byte table in LDS, one
// entry per bank), eight such words per lane in flight. The words are not aligned (a read starts anywhere): global accesses need not be.
RTK_DEV uint32_t rtk_ld_u32(const char* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
RTK_DEV void rtk_st_u32(char* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
RTK_FN void rtk_reverse_copy(char* __restrict__ dst_, const char* __restrict__ src_, uint32_t n_, const unsigned char* tab_) {
    char* __restrict__ const dst = rtk_gp(rtk_u(dst_)); const char* __restrict__ const src = rtk_gp(rtk_u(src_)); const uint32_t n = rtk_u(n_); const unsigned char* const tab = rtk_u(tab_);
    const uint32_t n4 = n & ~3u;
    constexpr uint32_t RW = 8;
    for (uint32_t i0 = 0; i0 < n4; i0 += 4u * RW * RTK_WAVE) {
        uint32_t w[RW];
#pragma unroll
        for (uint32_t u = 0; u < RW; ++u) { const uint32_t i = i0 + 4u * (u * RTK_WAVE + static_cast<uint32_t>(rtk_lane())); w[u] = i < n4 ? rtk_ld_u32(src + (n - 4u - i)) : 0u; }
#pragma unroll
        for (uint32_t u = 0; u < RW; ++u) {
            const uint32_t i = i0 + 4u * (u * RTK_WAVE + static_cast<uint32_t>(rtk_lane()));
            uint32_t b0 = w[u] >> 24, b1 = (w[u] >> 16) & 0xFFu, b2 = (w[u] >> 8) & 0xFFu, b3 = w[u] & 0xFFu; // the last character of the word comes first
            if (tab) { RTK_ASSUME_LDS(tab); b0 = tab[b0]; b1 = tab[b1]; b2 = tab[b2]; b3 = tab[b3]; }
            if (i < n4) rtk_st_u32(dst + i, b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
        }
    }
    for (uint32_t i = n4 + static_cast<uint32_t>(rtk_lane()); i < n; i += RTK_WAVE) { { const unsigned char c = static_cast<unsigned char>(src[n - 1u - i]); unsigned char o = c; if (tab) { RTK_ASSUME_LDS(tab); o = tab[c]; } dst[i] = static_cast<char>(o); } }
}

RTK_FN void rtk_enum_regions(const GraphView& g, const BatchView& bv, const RegionBatch& rb, uint32_t r, const unsigned char* comp_tab) {
    const uint32_t k = static_cast<uint32_t>(g.k);
    const uint64_t base = bv.roff[r];
    const uint32_t L = static_cast<uint32_t>(bv.roff[r + 1] - base);
    const uint32_t* sp = bv.s_pos + base; const uint32_t ns = bv.n_solid[r];
    // reverse complement of the read (used by the head and backward corrections, src/Correction.cpp:175); pass 2: the quality string reversed beside it
    {
        rtk_reverse_copy(rb.seq_rc.get() + base, bv.seq.get() + base, L, comp_tab);
        if (bv.qual.get() != nullptr && rb.qual_rev.get() != nullptr) rtk_reverse_copy(rb.qual_rev.get() + base, bv.qual.get() + base, L, nullptr);
    }
    uint32_t n_gaps = 0;
    const bool whole = (L <= k) || ns == 0 || (ns == L - k + 1);
    // (this program runs on ONE wave per read and the launch lasts as long as its longest read -- tens of thousands of solid anchors: the anchors are
    // read sixteen chunks of 64 at a time, and what the descriptors need from a neighbouring anchor comes out of the lanes' registers, not from memory)
    constexpr uint32_t EU = 16;
    // (what is left of a retired A/B build that counted the gaps several times: a loop of one trip. As a plain block the compiler allocates the
    // registers of this function differently, so it stays until a change that touches this kernel anyway)
    for (int once = 0; once < 1; ++once) { n_gaps = 0;
    if (!whole) for (uint32_t c0 = 0; c0 + 1 < ns; c0 += EU * RTK_WAVE) {
        uint32_t a[EU], b2[EU];
        for (uint32_t u = 0; u < EU; ++u) { const uint32_t i = c0 + u * RTK_WAVE + static_cast<uint32_t>(rtk_lane()); const bool in = i + 1 < ns; a[u] = in ? sp[i] : 0u; b2[u] = in ? sp[i + 1] : 1u; }
        for (uint32_t u = 0; u < EU; ++u) n_gaps += static_cast<uint32_t>(rtk_popc(rtk_ballot(a[u] != b2[u] - 1u)));
    }
    }
    const uint32_t total = whole ? 1u : ((sp[0] != 0 ? 1u : 0u) + n_gaps + 1u);
    unsigned long long first = 0;
    if (rtk_lane() == 0) first = rtk_atomic_add(rb.n_regions, static_cast<unsigned long long>(total));
    first = rtk_shfl(first, 0);
    rb.r_first[r] = first; rb.r_count[r] = total;
    if (first + total > rb.regions_cap) return; // host notices n_regions > cap and retries with a bigger list
    RegionDesc* out = rb.regions + first;
    uint32_t w = 0;
    auto put = [&](uint32_t kind, uint32_t i_solid, uint32_t prev_pos) {
        RegionDesc d; d.read = r; d.kind = kind; d.i_solid = i_solid; d.prev_pos = prev_pos; d.seg_off = 0; d.seq_len = 0; d.qual_len = 0; d.status = 0; d.pad = 0;
        out[w++] = d;
    };
    if (whole) { put((L > k && ns != 0 && ns == L - k + 1) ? RTK_RG_WHOLE_MAX : RTK_RG_WHOLE_MIN, 0, 0); rtk_sync(); return; }
    if (sp[0] != 0) put(RTK_RG_HEAD, 0, 0);
    uint32_t prev_pos = sp[0];
    // the gaps between runs of consecutive solid anchors, 64 anchors at a time: every lane that sees a gap writes its descriptor. The
    // segment before it stopped at the anchor behind the PREVIOUS gap (prev_pos = sp[previous gap + 1], sp[0] for the first one)
    for (uint32_t c0 = 0; c0 + 1 < ns; c0 += EU * RTK_WAVE) {
        uint32_t a[EU], b2[EU]; // a = sp[i], b2 = sp[i + 1] (out of range: a pair without a gap)
        for (uint32_t u = 0; u < EU; ++u) { const uint32_t i = c0 + u * RTK_WAVE + static_cast<uint32_t>(rtk_lane()); const bool in = i + 1 < ns; a[u] = in ? sp[i] : 0u; b2[u] = in ? sp[i + 1] : 1u; }
        for (uint32_t u = 0; u < EU; ++u) {
            const uint32_t i = c0 + u * RTK_WAVE + static_cast<uint32_t>(rtk_lane());
            const bool gap = a[u] != b2[u] - 1u;
            const uint64_t bal = rtk_ballot(gap);
            if (bal == 0ull) continue;
            const uint64_t below = bal & ((1ull << rtk_lane()) - 1ull); // gaps of this chunk in front of this lane's
            const uint32_t behind_prev = rtk_shfl(b2[u], below ? (63 - __builtin_clzll(below)) : 0); // the anchor behind the previous gap of the chunk: sp[that gap + 1]
            if (gap) {
                RegionDesc d; d.read = r; d.kind = RTK_RG_GAP; d.i_solid = i; d.prev_pos = below ? behind_prev : prev_pos; d.seg_off = 0; d.seq_len = 0; d.qual_len = 0; d.status = 0; d.pad = 0;
                out[w + static_cast<uint32_t>(rtk_popc(below))] = d;
            }
            w += static_cast<uint32_t>(rtk_popc(bal));
            prev_pos = rtk_u(rtk_shfl(b2[u], 63 - __builtin_clzll(bal)));
        }
    }
    put(sp[ns - 1] < L - k ? RTK_RG_TAIL : RTK_RG_TAIL_COPY, ns - 1, prev_pos);
    rtk_sync();
}

// ------------------------------------------------------------------------------------------------ stitch
// Two steps (round 4; one wave per read copied a 100 kb read's thousand segments one after the other while the machine idled):
// (1) one wave per read adds up the lengths of its segments, reserves the read's place in the output pool and leaves every segment's
// place inside the read (st_off: characters / quality bytes in front of it); (2) the segments of ALL reads are copied 64 per wave.
RTK_FN void rtk_stitch_offsets(const BatchView& bv, const RegionBatch& rb, uint32_t r) {
    const uint64_t f0 = rb.r_first[r];
    const RegionDesc* rg = rb.regions + f0; uint64_t* st = rb.st_off.get() + f0; const uint32_t n = rb.r_count[r];
    // lengths of the read's segments, 64 at a time (the loads of a chunk are independent: one round trip per chunk, not per segment)
    uint64_t ts = 0, tq = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += RTK_WAVE) {
        const uint32_t i = c0 + static_cast<uint32_t>(rtk_lane());
        int a = 0, b = 0; if (i < n) { a = static_cast<int>(rg[i].seq_len); b = static_cast<int>(rg[i].qual_len); }
        int ta, tb; const int pa = rtk_wave_excl_scan(a, &ta), pb = rtk_wave_excl_scan(b, &tb);
        if (i < n) st[i] = ((tq + static_cast<uint64_t>(pb)) << 32) | (ts + static_cast<uint64_t>(pa));
        ts += static_cast<uint64_t>(rtk_u(ta)); tq += static_cast<uint64_t>(rtk_u(tb));
    }
    unsigned long long off = 0;
    if (rtk_lane() == 0) off = rtk_atomic_add(rb.out_top, static_cast<unsigned long long>(ts + tq));
    off = rtk_shfl(off, 0);
    rb.out_off[r] = off; rb.out_seq_len[r] = static_cast<uint32_t>(ts); rb.out_qual_len[r] = static_cast<uint32_t>(tq);
    (void)bv;
}

// segments c0 .. c0 + 63 of the flat list: their descriptors and their reads' places one per lane, then the copies back to back
RTK_FN void rtk_stitch_copy(const RegionBatch& rb, uint64_t c0, uint64_t n_regions) {
    const uint64_t i = c0 + static_cast<uint64_t>(rtk_lane());
    uint32_t sl = 0, ql = 0; uint64_t so = 0, ws = 0, wq = 0;
    if (i < n_regions) {
        const RegionDesc* rd = rb.regions.get() + i;
        const uint32_t r = rd->read; const uint64_t st = rb.st_off[i];
        const uint64_t off = rb.out_off[r], ts = rb.out_seq_len[r], tq = rb.out_qual_len[r];
        if (off + ts + tq <= rb.out_cap) { sl = rd->seq_len; ql = rd->qual_len; so = rd->seg_off; ws = off + (st & 0xFFFFFFFFull); wq = off + ts + (st >> 32); } // (a read beyond the pool's end is not written: the host sees out_top > out_cap)
    }
    const uint32_t m = (n_regions - c0) < static_cast<uint64_t>(RTK_WAVE) ? static_cast<uint32_t>(n_regions - c0) : static_cast<uint32_t>(RTK_WAVE);
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t jsl = rtk_shfl(sl, static_cast<int>(j)), jql = rtk_shfl(ql, static_cast<int>(j)); const uint64_t jso = rtk_shfl(so, static_cast<int>(j)), jws = rtk_shfl(ws, static_cast<int>(j)), jwq = rtk_shfl(wq, static_cast<int>(j));
        rtk_wcopy2(rb.out_pool + jws, rb.seg_pool + jso, jsl, rb.out_pool + jwq, rb.seg_pool + jso + jsl, jql);
    }
}

#endif
