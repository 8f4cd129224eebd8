// chooseColors (reference: src/Correction.cpp:215-429), all of it: the side lists, the two bit-vector programs for the regions that make up
// nearly all of a batch, the general sorted-array program for the rest, and the dispatcher rtk_choose_colors (at the end of the file).
//
// The bit-vector programs, for the regions that make up nearly all of a batch: the colour
// sets of the anchors around one weak region hold a few hundred distinct pair ids together (measured on configs[1]: < 512 in 90 % of
// the calls; on the 1 Mb set of the bench's generator arguments a median of 235, at most 526, out of a median of 405 ids with repeats).
// Those ids are sorted once into a small universe kept in LDS; every set of the algorithm -- the six anchor classes, their
// unions / intersections / differences, curr_pid, all_pids -- is then ONE 64-bit word per lane (4096 bits), the whole class loop runs
// in registers (OR / AND / ANDN, popcount + wave sum, "the quota lowest ids" = a prefix count), and all_pids is expanded back into a
// sorted id list at the end. Same selections as the general sorted-array version further down, which stays the fallback for
// larger universes (returns RTK_NONE32 then). Bit order = id order, so "lowest ids first" is "lowest bits first".
#ifndef RTK_COLOURS_H
#define RTK_COLOURS_H

#include "rtk_region_paths.h"
#include "rtk_sets.h"
#include "rtk_sim_census.h"

#define RTK_CB_MAX_IDS (RTK_LDS_SET_CAP - 384u)   // ids gathered from all anchors (with repeats); universe (u32), 256 radix counters and 64 scatter words share the 8 KB LDS buffer
#define RTK_CB_MAX_SLOTS 24u   // side-list entries whose bit vectors are kept

// ------------------------------------------------------------------------------------------------ side lists
// anchors of the three sides are given as small (unitig, non-branching) lists, first insertion wins (unordered_map::insert).
RTK_DEV bool rtk_side_insert(SideList& l, uint32_t u, bool nonbranching) { // returns true when unseen
    const uint32_t n = rtk_u(l.n); const uint32_t* lu = rtk_u(l.u);
    for (uint32_t i0 = 0; i0 < n; i0 += RTK_WAVE) { // 64 entries per step
        const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
        if (rtk_ballot(i < n && lu[i] == u)) return false;
    }
    if (n < rtk_u(l.cap)) { l.u[n] = u; l.nb[n] = nonbranching ? 1 : 0; l.n = n + 1; rtk_sync(); }
    return true;
}

// set-buffer helpers on RegionScratch: buffers are addressed by index; sizes kept by the caller
RTK_DEV uint32_t rtk_rs_union(RegionScratch& s, int a, uint32_t na, const uint32_t* b, uint32_t nb, int out) {
    if (na + nb > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); return 0; }
    return rtk_set_union(s.set[a], na, b, nb, s.set[out], s.set[RTK_SET_UNION_TMP]);
}

// ------------------------------------------------------------------------------------------------ the bit-vector programs
#ifndef RTK_SIM
// Least-significant-digit radix sort of n 32-bit keys by one wave, 8 bits per pass: the bitonic network it replaces costs 45-66 stages of
// LDS compare-exchanges (1 400 LDS operations per lane for 512 keys), this costs two passes over the keys per digit. `a` holds the keys
// (LDS) and the result; `b` is the other buffer (LDS or global memory, n entries); `bins` = 256 counters in LDS. A pass is stable: the 64
// keys of a chunk find their equals by eight ballots (one per digit bit), rank themselves among them, and chunks are taken in order.
RTK_DEV void rtk_radix_sort_u32(uint32_t* a, uint32_t* b, uint32_t n, uint32_t* bins, uint32_t max_key) {
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    const uint64_t lt = (1ull << lane) - 1ull;
    int passes = 0; { uint32_t m = max_key; while (m) { ++passes; m >>= 8; } if (passes == 0) passes = 1; }
    if (passes & 1) ++passes; // an even number of passes: the result ends in `a`
    uint32_t* src = a; uint32_t* dst = b;
    for (int ps = 0; ps < passes; ++ps) {
        const int sh = 8 * ps;
        for (uint32_t i = lane; i < 256u; i += RTK_WAVE) bins[i] = 0u;
        RTK_WG_SYNC();
        // histogram of the digit
        for (uint32_t c0 = 0; c0 < n; c0 += RTK_WAVE) {
            const uint32_t i = c0 + lane; const bool ok = i < n;
            const uint32_t d = ok ? ((src[i] >> sh) & 0xFFu) : 0x100u;
            uint64_t eq = rtk_ballot(ok);
            for (int bt = 0; bt < 8; ++bt) { const uint64_t bb = rtk_ballot((d >> bt) & 1u); eq &= ((d >> bt) & 1u) ? bb : ~bb; }
            if (ok && (eq & lt) == 0ull) atomicAdd(&bins[d], static_cast<uint32_t>(rtk_popc(eq))); // the first lane of every group of equal digits
        }
        RTK_WG_SYNC();
        { // exclusive prefix over the 256 bins: four bins per lane
            uint32_t v[4]; uint32_t sum = 0;
            for (int x = 0; x < 4; ++x) { v[x] = bins[4u * lane + static_cast<uint32_t>(x)]; sum += v[x]; }
            int tot; uint32_t base = static_cast<uint32_t>(rtk_wave_excl_scan(static_cast<int>(sum), &tot));
            RTK_WG_SYNC();
            for (int x = 0; x < 4; ++x) { bins[4u * lane + static_cast<uint32_t>(x)] = base; base += v[x]; }
        }
        RTK_WG_SYNC();
        // stable scatter, chunk by chunk
        for (uint32_t c0 = 0; c0 < n; c0 += RTK_WAVE) {
            const uint32_t i = c0 + lane; const bool ok = i < n;
            const uint32_t key = ok ? src[i] : 0u;
            const uint32_t d = ok ? ((key >> sh) & 0xFFu) : 0x100u;
            uint64_t eq = rtk_ballot(ok);
            for (int bt = 0; bt < 8; ++bt) { const uint64_t bb = rtk_ballot((d >> bt) & 1u); eq &= ((d >> bt) & 1u) ? bb : ~bb; }
            const uint32_t before = static_cast<uint32_t>(rtk_popc(eq & lt));
            uint32_t base = 0;
            if (ok) base = bins[d];
            RTK_WG_SYNC();
            if (ok && before == 0u) bins[d] = base + static_cast<uint32_t>(rtk_popc(eq));
            if (ok) dst[base + before] = key;
            RTK_WG_SYNC();
        }
        uint32_t* t_ = src; src = dst; dst = t_;
    }
}

// The universe sort of the register program: n (32-bit key, tag) entries sorted by key, stable, by one wave. Two forms of the tag. ta == nullptr: the tag rides in
// the low `lo` bits of the word and the key sits above them (key < 2^(32 - lo)); the digits start at bit `lo`. Otherwise lo = 0, the word is the key and the tags
// are a byte array moved with the words (ta <-> tb as a <-> b). Differences from rtk_radix_sort_u32: as many passes as the largest key has bytes, odd or even --
// the result is where the last pass left it and the routine returns that buffer (a or b; the tags are in ta or tb accordingly); the histograms are plain LDS adds,
// one per key (a histogram needs no order: the match network is kept for the scatter alone), and where `bins` has 256 counters per pass they are all taken in
// one read of the keys. `a` is in LDS; b, ta, tb in LDS or device memory.
RTK_DEV uint32_t* rtk_radix_sort_tagged(uint32_t* a, uint32_t* b, uint8_t* ta, uint8_t* tb, uint32_t n, uint32_t* bins, uint32_t bins_words, uint32_t lo, uint32_t max_key) {
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t passes = 0; { uint32_t m = max_key; while (m) { ++passes; m >>= 8; } if (passes == 0) passes = 1; }
    const bool fused = passes * 256u <= bins_words;
    if (fused) {
        for (uint32_t i = lane; i < passes * 256u; i += RTK_WAVE) bins[i] = 0u;
        RTK_WG_SYNC();
        for (uint32_t i = lane; i < n; i += RTK_WAVE) { const uint32_t key = a[i] >> lo; for (uint32_t ps = 0; ps < passes; ++ps) atomicAdd(&bins[256u * ps + ((key >> (8u * ps)) & 0xFFu)], 1u); }
        RTK_WG_SYNC();
    }
    uint32_t* src = a; uint32_t* dst = b; uint8_t* ts = ta; uint8_t* td = tb;
    for (uint32_t ps = 0; ps < passes; ++ps) {
        const uint32_t sh = lo + 8u * ps;
        uint32_t* const pb = fused ? bins + 256u * ps : bins;
        if (!fused) {
            for (uint32_t i = lane; i < 256u; i += RTK_WAVE) pb[i] = 0u;
            RTK_WG_SYNC();
            for (uint32_t i = lane; i < n; i += RTK_WAVE) atomicAdd(&pb[(src[i] >> sh) & 0xFFu], 1u);
            RTK_WG_SYNC();
        }
        { // exclusive prefix over the 256 bins: four bins per lane
            uint32_t v[4]; uint32_t sum = 0;
            for (int x = 0; x < 4; ++x) { v[x] = pb[4u * lane + static_cast<uint32_t>(x)]; sum += v[x]; }
            int tot; uint32_t base = static_cast<uint32_t>(rtk_wave_excl_scan(static_cast<int>(sum), &tot));
            RTK_WG_SYNC();
            for (int x = 0; x < 4; ++x) { pb[4u * lane + static_cast<uint32_t>(x)] = base; base += v[x]; }
        }
        RTK_WG_SYNC();
        // stable scatter, chunk by chunk
        for (uint32_t c0 = 0; c0 < n; c0 += RTK_WAVE) {
            const uint32_t i = c0 + lane; const bool ok = i < n;
            const uint32_t key = ok ? src[i] : 0u;
            const uint32_t tag = (ok && ts) ? ts[i] : 0u;
            const uint32_t d = ok ? ((key >> sh) & 0xFFu) : 0x100u;
            uint64_t eq = rtk_ballot(ok);
            for (int bt = 0; bt < 8; ++bt) { const uint64_t bb = rtk_ballot((d >> bt) & 1u); eq &= ((d >> bt) & 1u) ? bb : ~bb; }
            const uint32_t before = static_cast<uint32_t>(rtk_popc(eq & lt));
            uint32_t base = 0;
            if (ok) base = pb[d];
            RTK_WG_SYNC();
            if (ok && before == 0u) pb[d] = base + static_cast<uint32_t>(rtk_popc(eq));
            if (ok) { dst[base + before] = key; if (ts) td[base + before] = static_cast<uint8_t>(tag); }
            RTK_WG_SYNC();
        }
        { uint32_t* t_ = src; src = dst; dst = t_; uint8_t* u_ = ts; ts = td; td = u_; }
    }
    return src;
}
#endif

#ifdef RTK_SIM
struct RtkBM { uint64_t w[64]; };
inline RtkBM rtk_bm_zero() { RtkBM r; for (int i = 0; i < 64; ++i) r.w[i] = 0; return r; }
inline RtkBM operator|(const RtkBM& a, const RtkBM& b) { RtkBM r; for (int i = 0; i < 64; ++i) r.w[i] = a.w[i] | b.w[i]; return r; }
inline RtkBM operator&(const RtkBM& a, const RtkBM& b) { RtkBM r; for (int i = 0; i < 64; ++i) r.w[i] = a.w[i] & b.w[i]; return r; }
inline RtkBM rtk_bm_andn(const RtkBM& a, const RtkBM& b) { RtkBM r; for (int i = 0; i < 64; ++i) r.w[i] = a.w[i] & ~b.w[i]; return r; }
inline uint32_t rtk_bm_count(const RtkBM& a) { uint32_t c = 0; for (int i = 0; i < 64; ++i) c += static_cast<uint32_t>(__builtin_popcountll(a.w[i])); return c; }
inline RtkBM rtk_bm_lowest(const RtkBM& a, uint32_t q) { RtkBM r = rtk_bm_zero(); for (int i = 0; i < 64 && q; ++i) { uint64_t x = a.w[i]; while (x && q) { const uint64_t b = x & (~x + 1ull); r.w[i] |= b; x ^= b; --q; } } return r; }
inline RtkBM rtk_bm_load(const uint64_t* p) { RtkBM r; for (int i = 0; i < 64; ++i) r.w[i] = p[i]; return r; }
inline void rtk_bm_store(uint64_t* p, const RtkBM& a) { for (int i = 0; i < 64; ++i) p[i] = a.w[i]; }
#else
typedef uint64_t RtkBM; // word `lane` of a 4096-bit vector
RTK_DEV RtkBM rtk_bm_zero() { return 0ull; }
RTK_DEV RtkBM rtk_bm_andn(RtkBM a, RtkBM b) { return a & ~b; }
RTK_DEV uint32_t rtk_bm_count(RtkBM a) { return static_cast<uint32_t>(rtk_u(rtk_wave_sum(rtk_popc(a)))); }
RTK_DEV RtkBM rtk_bm_lowest(RtkBM a, uint32_t q) { // the q lowest set bits of the 4096-bit vector
    int total; const int before = rtk_wave_excl_scan(rtk_popc(a), &total);
    int keep = static_cast<int>(q) - before; const int mine = rtk_popc(a);
    keep = keep < 0 ? 0 : (keep > mine ? mine : keep);
    uint64_t rest = a; for (int i = 0; i < keep; ++i) rest &= rest - 1ull; // a without its `keep` lowest bits
    return a & ~rest;
}
RTK_DEV RtkBM rtk_bm_load(const uint64_t* p) { return p[rtk_lane()]; }
RTK_DEV void rtk_bm_store(uint64_t* p, RtkBM a) { p[rtk_lane()] = a; }
#endif

// bit vector of the ids of a sorted set inside the universe uni[0..U)
RTK_DEV RtkBM rtk_bm_from_ids(const uint32_t* uni, uint32_t U, uint64_t* scatter, const uint32_t* ids, uint32_t n) {
#ifdef RTK_SIM
    (void)scatter;
    RtkBM r = rtk_bm_zero();
    for (uint32_t i = 0; i < n; ++i) { const uint32_t x = rtk_lower_bound(uni, U, ids[i]); r.w[x >> 6] |= 1ull << (x & 63u); }
    return r;
#else
    scatter[rtk_lane()] = 0ull;
    RTK_WG_SYNC();
    for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < n; i += RTK_WAVE) {
        const uint32_t id = ids[i];
        uint32_t lo = 0, hi = U; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (uni[mid] < id) lo = mid + 1; else hi = mid; }
        atomicOr(reinterpret_cast<unsigned long long*>(scatter) + (lo >> 6), 1ull << (lo & 63u));
    }
    RTK_WG_SYNC();
    return scatter[rtk_lane()];
#endif
}


#ifndef RTK_SIM
// The same selection for the common case -- at most 1664 ids (with repeats) on at most 24 side unitigs -- with every chain of dependent memory round trips
// taken out: slot s lives in lane s (unitig, offsets and sizes of its colour lists, cardinality, flags: three round trips for all slots together instead of
// five per slot and pass), the candidate anchors are ranked in registers, the ids go from the colour pool straight into LDS (one flat pass over all lists),
// each with the number of the list it came from (its tag: 2 x slot + global), and the per-list bit vectors stay in LDS behind the universe. Returns
// RTK_NONE32 when the case does not fit (caller goes on to rtk_choose_colors_bits).
#ifndef RTK_CS_MAX_IDS
#define RTK_CS_MAX_IDS 512u // (developer builds with a smaller LDS buffer lower it: profiles/scripts/build_wpe_variant.sh)
#endif
#define RTK_CS_TAG_BITS 6u                                  // a tag is below 2 x RTK_CB_MAX_SLOTS = 48
#define RTK_CS_PACKED_LIMIT (1u << (32u - RTK_CS_TAG_BITS)) // ids below it carry their tag in the low bits of their word; larger ones have it in a byte array
static_assert(2u * RTK_CB_MAX_SLOTS <= (1u << RTK_CS_TAG_BITS), "colour selection: a tag fits its bits");
static_assert(2u * RTK_CS_MAX_IDS + 768u + RTK_CS_MAX_IDS / 2u <= RTK_LDS_SET_CAP && RTK_CS_MAX_IDS <= 512u && RTK_CS_MAX_IDS % 4u == 0u, "colour selection, at most RTK_CS_MAX_IDS ids: two key buffers, 24 x 2 x 8 vector words (before them: three sets of sort counters) and two tag arrays in the LDS buffer");

// Universe and bit vectors of one call. In: T <= RTK_CB_MAX_IDS entries in L (the wave's LDS buffer), each an id and a tag < n_vec <= 48; mx = the largest id.
// packed (mx < RTK_CS_PACKED_LIMIT): L[i] = (id << RTK_CS_TAG_BITS) | tag. Otherwise L[i] = id and the tag is byte i of rtk_cu_tags(). Out: the U distinct ids
// in rising order in L[0, U), and n_vec bit vectors of VW = ceil(U / 64) 64-bit words each at `vec` (in L, behind the universe): bit r of vector t is set when
// list t holds the id of rank r. The entries are sorted by id (rtk_radix_sort_tagged); a first pass over the sorted entries counts U, which fixes the layout;
// a second one writes the universe and ORs every entry's bit into the vector of its tag -- an entry's rank is the number of run heads up to it, so nothing is
// searched. Returns false when universe and vectors do not fit the buffer (nothing of the caller's is changed then).
// T <= RTK_CS_MAX_IDS: keys in L[0, 512) and L[512, 1024), counters, then vectors, in L[1024, 1792), tag arrays in L[1792, 2048).
// Above: keys in L[0, 1664) and in gbuf (device memory, T words), counters in L[1664, 1920), tag arrays in gtags (device memory, 2 x 1664 bytes); the sorted
// entries are read from gbuf (copied there when the sort ended in L), so that the vectors can take the place of the keys.
RTK_DEV uint8_t* rtk_cu_tags(uint32_t* L, uint32_t T, uint8_t* gtags) { return T > RTK_CS_MAX_IDS ? gtags : reinterpret_cast<uint8_t*>(L + 2u * RTK_CS_MAX_IDS + 768u); }
// the sort of that layout: returns the sorted entries (in L, or in the second key buffer after an odd number of passes) and, in *tsrt, their tags when they travel apart
RTK_DEV uint32_t* rtk_cu_sort(uint32_t* L, uint32_t T, uint32_t mx, uint32_t* gbuf, uint8_t* gtags, const uint8_t** tsrt) {
    const bool big = T > RTK_CS_MAX_IDS, packed = mx < RTK_CS_PACKED_LIMIT;
    uint8_t* const ta = packed ? nullptr : rtk_cu_tags(L, T, gtags); uint8_t* const tb = packed ? nullptr : ta + (big ? RTK_CB_MAX_IDS : RTK_CS_MAX_IDS);
    uint32_t* const srt = rtk_radix_sort_tagged(L, big ? gbuf : L + RTK_CS_MAX_IDS, ta, tb, T, big ? L + RTK_CB_MAX_IDS : L + 2u * RTK_CS_MAX_IDS, big ? 256u : 768u, packed ? RTK_CS_TAG_BITS : 0u, mx);
    *tsrt = srt == L ? ta : tb;
    return srt;
}
RTK_DEV bool rtk_colour_universe(uint32_t* L, uint32_t T, uint32_t n_vec, uint32_t mx, uint32_t* gbuf, uint8_t* gtags, uint32_t* U_out, uint32_t* VW_out, uint64_t** vec_out) {
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    const uint64_t le = (2ull << lane) - 1ull; // this lane and the ones below
    const bool big = T > RTK_CS_MAX_IDS, packed = mx < RTK_CS_PACKED_LIMIT;
    const uint8_t* tsrt;
    const uint32_t* srt = rtk_cu_sort(L, T, mx, gbuf, gtags, &tsrt);
    if (big && srt == L) { for (uint32_t i = lane; i < T; i += RTK_WAVE) gbuf[i] = L[i]; RTK_WG_SYNC(); srt = gbuf; }
    // run heads of one chunk of 64 sorted entries (four chunks are loaded at a time: their round trips overlap when the entries are in device memory)
    uint32_t carry = 0; // id of the entry before the chunk
    auto heads = [&](uint32_t idx, uint32_t w, uint32_t* id) -> uint64_t {
        *id = packed ? (w >> RTK_CS_TAG_BITS) : w;
        const uint32_t prev = rtk_shfl_up1(*id, carry);
        carry = rtk_shfl(*id, 63);
        return rtk_ballot(idx < T && (idx == 0u || *id != prev));
    };
    uint32_t U = 0;
    for (uint32_t i0 = 0; i0 < T; i0 += 4u * RTK_WAVE) {
        uint32_t w[4];
        for (uint32_t k = 0; k < 4u; ++k) { const uint32_t idx = i0 + k * RTK_WAVE + lane; w[k] = idx < T ? srt[idx] : 0u; }
        for (uint32_t k = 0; k < 4u; ++k) { uint32_t id; U += static_cast<uint32_t>(rtk_popc(heads(i0 + k * RTK_WAVE + lane, w[k], &id))); }
    }
    const uint32_t VW = U ? (U + 63u) / 64u : 1u;
    *U_out = U; *VW_out = VW;
    const uint32_t at = big ? ((U + 1u) & ~1u) : 2u * RTK_CS_MAX_IDS;
    if (at + 2u * n_vec * VW > (big ? RTK_LDS_SET_CAP : 2u * RTK_CS_MAX_IDS + 768u)) return false;
    uint64_t* const vec = reinterpret_cast<uint64_t*>(L + at);
    for (uint32_t i = lane; i < n_vec * VW; i += RTK_WAVE) vec[i] = 0ull;
    RTK_WG_SYNC();
    uint32_t R = 0; carry = 0;
    for (uint32_t i0 = 0; i0 < T; i0 += 4u * RTK_WAVE) {
        uint32_t w[4], tg[4];
        for (uint32_t k = 0; k < 4u; ++k) { const uint32_t idx = i0 + k * RTK_WAVE + lane; w[k] = idx < T ? srt[idx] : 0u; tg[k] = packed ? (w[k] & ((1u << RTK_CS_TAG_BITS) - 1u)) : (idx < T ? tsrt[idx] : 0u); }
        RTK_WG_SYNC(); // (T <= RTK_CS_MAX_IDS and an even number of passes: the universe is written over entries read above, at or below their own place)
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t idx = i0 + k * RTK_WAVE + lane; uint32_t id;
            const uint64_t bal = heads(idx, w[k], &id);
            if (idx < T) {
                const uint32_t rank = R + static_cast<uint32_t>(rtk_popc(bal & le)) - 1u;
                if ((bal >> lane) & 1ull) L[rank] = id;
                atomicOr(reinterpret_cast<unsigned long long*>(vec) + tg[k] * VW + (rank >> 6), 1ull << (rank & 63u));
            }
            R += static_cast<uint32_t>(rtk_popc(bal));
        }
    }
    RTK_WG_SYNC();
    *vec_out = vec;
    return true;
}
// the 512-bit vectors of the small case live in lanes 0..7 (the other lanes hold zero): sums and prefix sums over eight lanes by DPP
// moves inside one row (quad permutes, half-row mirror, row shifts) instead of six cross-lane permutes through LDS
RTK_DEV int rtk_sum8(int v) { // every lane of 0..7 gets the sum over lanes 0..7 (callers read lane 0)
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false); // row_half_mirror: lane i <-> 7 - i
    return v;
}
RTK_DEV uint32_t rtk_bm8_count(RtkBM a) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(rtk_sum8(rtk_popc(a)))); }
RTK_DEV RtkBM rtk_bm8_lowest(RtkBM a, uint32_t q) { // the q lowest set bits
    const int mine = rtk_popc(a);
    int inc = mine; // inclusive prefix sum over the row (zeros shifted in)
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xF, 0xF, true); // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xF, 0xF, true); // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xF, 0xF, true); // row_shr:4
    int keep = static_cast<int>(q) - (inc - mine);
    keep = keep < 0 ? 0 : (keep > mine ? mine : keep);
    uint64_t rest = a; for (int i = 0; i < keep; ++i) rest &= rest - 1ull;
    return a & ~rest;
}
RTK_FN uint32_t rtk_choose_colors_small(const RCtx& c_, const SideList& side_s_, const SideList& side_e_, const SideList& side_w_) {
    const RCtx& c = *rtk_u(&c_); const SideList& side_s = *rtk_u(&side_s_); const SideList& side_e = *rtk_u(&side_e_); const SideList& side_w = *rtk_u(&side_w_); RTK_ASSUME_LDS(&side_s); RTK_ASSUME_LDS(&side_e); RTK_ASSUME_LDS(&side_w);
    RegionScratch& s = rtk_hdr(c);
    const GraphView& g = c.g;
    const uint32_t nw = rtk_u(side_w.n), ne = rtk_u(side_e.n), ns = rtk_u(side_s.n), n_slots = nw + ne + ns; // slot order: middle, right, left
    if (n_slots == 0 || n_slots > RTK_CB_MAX_SLOTS) return RTK_NONE32;
    const uint32_t lane = static_cast<uint32_t>(rtk_lane());
    const uint32_t* const pw = rtk_u(side_w.u); const uint32_t* const pe = rtk_u(side_e.u); const uint32_t* const ps = rtk_u(side_s.u);
    const uint8_t* const qw = rtk_u(side_w.nb); const uint8_t* const qe = rtk_u(side_e.nb); const uint8_t* const qs = rtk_u(side_s.nb);
    const uint32_t* const col = g.col; const uint64_t* const loff = g.loff; const uint64_t* const goff = g.goff; const int32_t* const gid = g.gid; const uint32_t* const cardp = g.card;
    (void)rtk_clock(); // (what is left of a retired lap profile: one read of the cycle counter. Without it the compiler emits other code for this function,
                       // so it stays until a change that touches this kernel anyway)
    // ---- A. one lane per slot ----
    uint32_t m_u = 0, m_nl = 0, m_ng = 0, m_card = 0, m_nb = 0; uint64_t m_lo = 0, m_go = 0; int32_t m_gi = -1;
    if (lane < n_slots) {
        const uint32_t* pu; const uint8_t* pn; uint32_t i = lane;
        if (i < nw) { pu = pw; pn = qw; } else if (i - nw < ne) { i -= nw; pu = pe; pn = qe; } else { i -= nw + ne; pu = ps; pn = qs; }
        m_u = pu[i]; m_nb = pn[i];
        m_gi = gid[m_u]; m_lo = loff[m_u]; m_nl = static_cast<uint32_t>(loff[m_u + 1] - m_lo); m_card = cardp[m_u];
        if (m_gi >= 0) { m_go = goff[m_gi]; m_ng = static_cast<uint32_t>(goff[m_gi + 1] - m_go); }
    }
    int total = 0; const uint32_t st = static_cast<uint32_t>(rtk_wave_excl_scan(static_cast<int>(m_nl + m_ng), &total)); // first id of the slot in the flat order
    const uint32_t T = static_cast<uint32_t>(rtk_u(total));
    // (above RTK_CS_MAX_IDS ids the sort's second buffer is set[RTK_SET_CS_SORT], and set[RTK_SET_CS_TAGS] holds the tags of ids too large to carry them)
    const bool big = T > RTK_CS_MAX_IDS;
    if (T > RTK_CB_MAX_IDS || (big && s.set_cap < RTK_CB_MAX_IDS)) return RTK_NONE32;
    // ---- B. candidate anchors: cardinality >= min_cov_vertices, first occurrence of their unitig, ordered by (cardinality, unitig) [D1] ----
    const uint32_t min_cov_v = c.o.min_cov_vertices;
    bool dup = false;
    for (uint32_t j = 0; j + 1 < n_slots; ++j) { const uint32_t uj = rtk_shfl(m_u, static_cast<int>(j)); dup = dup || ((j < lane) && (uj == m_u)); }
    const bool cand = lane < n_slots && m_card >= min_cov_v && !dup;
    const uint64_t cb = rtk_ballot(cand); const uint32_t nsp = static_cast<uint32_t>(rtk_popc(cb));
    const uint64_t key = rtk_d1_key(m_card, m_u, c.o.d1_desc); // distinct among the candidates
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n_slots; ++j) { const uint64_t kj = rtk_shfl(key, static_cast<int>(j)); rank += (((cb >> j) & 1ull) && kj < key) ? 1u : 0u; }
    uint32_t src = 0;
    for (uint32_t j = 0; j < n_slots; ++j) { const uint32_t rj = rtk_shfl(rank, static_cast<int>(j)); if (((cb >> j) & 1ull) && rj == lane) src = j; }
    // lane j < nsp holds the j-th candidate: its slot, cardinality and remaining quota (p_spid.second)
    const uint32_t cov = 30;
    const uint32_t k_slot = src; const uint32_t k_card = rtk_shfl(m_card, static_cast<int>(src));
    uint32_t k_quota = k_card < cov ? k_card : cov;
    // ---- C. every id of every side unitig, with its tag, straight into LDS ----
    uint32_t* const L = rtk_lds_set_buf();
    uint32_t* const uni = L;
    uint8_t* const gtags = reinterpret_cast<uint8_t*>(s.set[RTK_SET_CS_TAGS].get());
    uint32_t mx = 0;
    for (bool packed = true;; packed = false) { // (a second time, tags apart, when an id turns out too large to carry its tag)
        uint8_t* const tags = rtk_cu_tags(L, T, gtags);
        for (uint32_t t0 = 0; t0 < T; t0 += RTK_WAVE) {
            const uint32_t t = t0 + lane;
            uint32_t i = 0;
            for (uint32_t j = 1; j < n_slots; ++j) { const uint32_t sj = rtk_shfl(st, static_cast<int>(j)); if (sj <= t) i = j; } // the last slot that starts at or before t (empty slots share their start with the next one)
            const uint32_t s_i = rtk_shfl(st, static_cast<int>(i)), nl_i = rtk_shfl(m_nl, static_cast<int>(i));
            const uint64_t lo_i = rtk_shfl(m_lo, static_cast<int>(i)), go_i = rtk_shfl(m_go, static_cast<int>(i));
            if (t < T) {
                const uint32_t off = t - s_i; const uint32_t tag = 2u * i + (off >= nl_i ? 1u : 0u);
                const uint32_t x = col[off < nl_i ? lo_i + off : go_i + (off - nl_i)];
                mx = x > mx ? x : mx;
                if (packed) L[t] = (x << RTK_CS_TAG_BITS) | tag; else { L[t] = x; tags[t] = static_cast<uint8_t>(tag); }
            }
        }
        for (int o = 32; o > 0; o >>= 1) { const uint32_t v2 = static_cast<uint32_t>(__shfl_xor(static_cast<int>(mx), o, 64)); mx = v2 > mx ? v2 : mx; }
        mx = rtk_u(mx);
        if (!packed || mx < RTK_CS_PACKED_LIMIT) break;
    }
    RTK_WG_SYNC();
    // ---- D. universe (sorted, duplicates dropped) and the bit vectors of every slot (local part, global part), both in LDS ----
    uint32_t U = 0, VW = 1; uint64_t* cbm = nullptr;
    if (!rtk_colour_universe(L, T, 2u * n_slots, mx, s.set[RTK_SET_CS_SORT], gtags, &U, &VW, &cbm)) { s.cnt[RTK_RC_COLOURS_DECLINED_FIT] += 1; return RTK_NONE32; }
    s.cnt[RTK_RC_COLOUR] += T;
    // (up to 8 words a vector lives in lanes 0..7 and the 8-lane forms count it)
    const bool w8 = VW <= 8u;
    auto ld = [&](uint32_t idx) -> RtkBM { return lane < VW ? cbm[idx * VW + lane] : 0ull; };
    auto cnt_ = [&](RtkBM a) -> uint32_t { return w8 ? rtk_bm8_count(a) : rtk_bm_count(a); };
    auto low_ = [&](RtkBM a, uint32_t q) -> RtkBM { return w8 ? rtk_bm8_lowest(a, q) : rtk_bm_lowest(a, q); };
    // ---- E. the six anchor classes: side (middle, right, left) x branching / non-branching; G2: the global set alone when there is one ----
    RtkBM a[6];
    for (int sh = 0; sh < 6; ++sh) {
        RtkBM acc = 0ull;
        const uint32_t first = (sh % 3 == 0) ? 0u : (sh % 3 == 1 ? nw : nw + ne), cnt = (sh % 3 == 0) ? nw : (sh % 3 == 1 ? ne : ns);
        const uint32_t want_nb = sh >= 3 ? 1u : 0u;
        for (uint32_t slot = first; slot < first + cnt; ++slot) {
            if (rtk_u(rtk_shfl(m_nb, static_cast<int>(slot))) != want_nb) continue;
            const bool has_global = rtk_u(rtk_shfl(m_gi, static_cast<int>(slot))) >= 0;
            acc |= ld(2u * slot + (has_global ? 1u : 0u));
        }
        a[sh] = acc;
    }
    const RtkBM pos0 = a[0] | a[3], pos1 = a[1] | a[4], pos2 = a[2] | a[5];
    const RtkBM a01 = pos0 & pos1, a12 = pos1 & pos2, a02 = pos0 & pos2;
    const RtkBM nobranch_all = a[3] | a[4] | a[5];
    const RtkBM i3 = a01 & a12, i2 = a01 | a12 | a02;
    RtkBM nobranch = nobranch_all, branching = 0ull, prev2 = 0ull, all = 0ull;
    uint32_t nb_unselected = nsp;
    // ---- F. class loop (:331-429) ----
    for (int i = 5; i >= 0; --i) {
        if (nb_unselected == 0) break;
        RtkBM a2;
        if (i == 5) a2 = nobranch & i3;
        else if (i == 4) { nobranch = rtk_bm_andn(nobranch, prev2); a2 = nobranch & i2; }
        else if (i == 3) { nobranch = rtk_bm_andn(nobranch, prev2); a2 = nobranch; }
        else if (i == 2) { branching = rtk_bm_andn(a[0] | a[1] | a[2], nobranch_all); a2 = branching & i3; }
        else if (i == 1) { branching = rtk_bm_andn(branching, prev2); a2 = branching & i2; }
        else { branching = rtk_bm_andn(branching, prev2); a2 = branching; }
        prev2 = a2;
        if (cnt_(a2) == 0) continue;
        nb_unselected = 0;
        RtkBM curr = a2;
        for (uint32_t j = 0; j < nsp; ++j) {
            int quota = static_cast<int>(rtk_u(rtk_shfl(k_quota, static_cast<int>(j))));
            if (quota > 0) {
                const uint32_t slot = rtk_u(rtk_shfl(k_slot, static_cast<int>(j)));
                const RtkBM cu = ld(2u * slot) | ld(2u * slot + 1u); // all colours of the anchor
                if (i == 0 || cnt_(cu & curr) >= 1) {
                    const uint32_t cd = rtk_u(rtk_shfl(k_card, static_cast<int>(j))); const uint32_t min_cov = cd < cov ? cd : cov;
                    const uint32_t sh = cnt_(cu & all);
                    quota = static_cast<int>(min_cov - (sh < min_cov ? sh : min_cov));
                    if (quota > 0) {
                        const uint32_t all_card = cnt_(all);
                        const RtkBM pid = low_(cu & curr, static_cast<uint32_t>(quota));
                        all = all | pid; curr = rtk_bm_andn(curr, pid);
                        const int gained = static_cast<int>(cnt_(all) - all_card);
                        quota -= gained < quota ? gained : quota;
                    }
                }
                if (lane == j) k_quota = static_cast<uint32_t>(quota);
            }
            nb_unselected += quota > 0 ? 1u : 0u;
        }
    }
    // ---- all_pids back to a sorted id list in set[RTK_SET_ALL_PIDS] ----
    const uint32_t n_all = rtk_bm_count(all);
    if (n_all > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); return 0; }
    uint32_t* out = s.set[RTK_SET_ALL_PIDS];
    { int tot2; uint32_t at = static_cast<uint32_t>(rtk_wave_excl_scan(rtk_popc(all), &tot2)); uint64_t x = all;
      while (x) { const int b = __builtin_ctzll(x); out[at++] = uni[64u * lane + static_cast<uint32_t>(b)]; x &= x - 1ull; } }
    rtk_sync();
    s.cnt[big ? RTK_RC_COLOURS_WIDE : RTK_RC_COLOURS_SMALL] += 1;
    return n_all;
}
#endif

// Returns |all_pids| (ids in s.set[RTK_SET_ALL_PIDS]), or RTK_NONE32 when the anchors' sets do not fit the small universe (caller falls back).
RTK_FN uint32_t rtk_choose_colors_bits(const RCtx& c_, const SideList& side_s_, const SideList& side_e_, const SideList& side_w_) {
    const RCtx& c = *rtk_u(&c_); const SideList& side_s = *rtk_u(&side_s_); const SideList& side_e = *rtk_u(&side_e_); const SideList& side_w = *rtk_u(&side_w_); RTK_ASSUME_LDS(&side_s); RTK_ASSUME_LDS(&side_e); RTK_ASSUME_LDS(&side_w);
    RegionScratch& s = rtk_hdr(c);
    const GraphView& g = c.g;
    const SideList* sides[3] = {&side_w, &side_e, &side_s};
    const uint32_t n_slots = side_w.n + side_e.n + side_s.n;
    if (n_slots == 0 || n_slots > RTK_CB_MAX_SLOTS || s.set_cap < 2 * RTK_CB_MAX_IDS + 64u * 4u * RTK_CB_MAX_SLOTS || s.list_cap < 2 * RTK_CB_MAX_SLOTS) return RTK_NONE32;
    // how many ids in all (global + local of every side unitig)
    uint32_t T = 0;
    for (int sd = 0; sd < 3; ++sd) for (uint32_t i = 0; i < sides[sd]->n; ++i) {
        const uint32_t u = sides[sd]->u[i]; const int32_t gi = g.gid[u];
        T += static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]) + (gi >= 0 ? static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]) : 0u);
        if (T > RTK_CB_MAX_IDS) return RTK_NONE32;
    }
    // candidate anchors: cardinality >= min_cov_vertices, ordered by (cardinality, unitig id) [D1]; the value carried through the sort is
    // the anchor's slot (its position in the concatenated side lists: middle, right, left)
    uint64_t* keys = s.list[RTK_L_COL_KEYS]; uint64_t* vals = s.list[RTK_L_COL_VALS]; uint64_t* slot_of = s.list[RTK_L_COL_SLOT_OF];
    uint32_t nsp = 0;
    { uint32_t slot = 0;
      for (int sd = 0; sd < 3; ++sd) for (uint32_t i = 0; i < sides[sd]->n; ++i, ++slot) {
        const uint32_t u = sides[sd]->u[i];
        if (g.card[u] < c.o.min_cov_vertices) continue;
        bool dup = false; for (uint32_t j0 = 0; j0 < nsp && !dup; j0 += RTK_WAVE) { const uint32_t j = j0 + static_cast<uint32_t>(rtk_lane()); dup = rtk_ballot(j < nsp && rtk_d1_unitig(keys[j], c.o.d1_desc) == u) != 0ull; }
        if (dup) continue;
        keys[nsp] = rtk_d1_key(g.card[u], u, c.o.d1_desc); vals[nsp] = slot; ++nsp; rtk_sync();
      } }
    rtk_sort_pairs(keys, vals, nsp); // (uses the LDS buffer: before the universe moves in)
    const uint32_t cov = 30;
    for (uint32_t j = static_cast<uint32_t>(rtk_lane()); j < nsp; j += RTK_WAVE) { slot_of[j] = vals[j]; const uint32_t cd = static_cast<uint32_t>(keys[j] >> 32); vals[j] = cd < cov ? cd : cov; } // remaining quota (p_spid.second)
    rtk_sync();
    // ---- universe: every id of every side unitig, sorted, duplicates dropped ----
    uint32_t* gathered = s.set[RTK_SET_CB_IDS];
    { uint32_t at = 0;
      for (int sd = 0; sd < 3; ++sd) for (uint32_t i = 0; i < sides[sd]->n; ++i) {
        const uint32_t u = sides[sd]->u[i]; const int32_t gi = g.gid[u];
        const uint32_t nl = static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]); const uint32_t* pl = g.col + g.loff[u];
        for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < nl; x += RTK_WAVE) gathered[at + x] = pl[x];
        at += nl;
        if (gi >= 0) { const uint32_t ng = static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]); const uint32_t* pg = g.col + g.goff[gi];
                       for (uint32_t x = static_cast<uint32_t>(rtk_lane()); x < ng; x += RTK_WAVE) gathered[at + x] = pg[x]; at += ng; }
      } }
    rtk_sync();
    s.cnt[RTK_RC_COLOUR] += T;
    uint32_t U = 0;
#ifdef RTK_SIM
    uint32_t* const uni = s.set[RTK_SET_CB_IDS] + RTK_CB_MAX_IDS; uint64_t* const scatter = nullptr;
    { for (uint32_t i = 0; i < T; ++i) uni[i] = gathered[i];
      std::sort(uni, uni + T);
      for (uint32_t i = 0; i < T; ++i) if (i == 0 || uni[i] != uni[i - 1]) uni[U++] = uni[i]; }
#else
    uint32_t* const uni = rtk_lds_set_buf(); uint64_t* const scatter = reinterpret_cast<uint64_t*>(uni + RTK_CB_MAX_IDS + 256u); // [0, 1664) ids, [1664, 1920) radix counters, [1920, 2048) scatter words
    { // radix sort of the ids in LDS (second buffer: the gathered copy in scratch memory)
      uint32_t mx = 0;
      for (uint32_t i = static_cast<uint32_t>(rtk_lane()); i < T; i += RTK_WAVE) { const uint32_t x = gathered[i]; uni[i] = x; mx = x > mx ? x : mx; }
      for (int o = 32; o > 0; o >>= 1) { const uint32_t v2 = static_cast<uint32_t>(__shfl_xor(static_cast<int>(mx), o, 64)); mx = v2 > mx ? v2 : mx; }
      RTK_WG_SYNC();
      rtk_radix_sort_u32(uni, gathered, T, uni + RTK_CB_MAX_IDS, rtk_u(mx));
      for (uint32_t i0 = 0; i0 < T; i0 += RTK_WAVE) { // forward compaction of the first elements of the runs
          const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane());
          uint32_t x = 0; bool keep = false;
          if (i < T) { x = uni[i]; keep = (i == 0) || (uni[i - 1] != x); }
          RTK_WG_SYNC();
          const uint64_t bal = rtk_ballot(keep);
          if (keep) uni[U + static_cast<uint32_t>(rtk_popc(bal & ((1ull << rtk_lane()) - 1ull)))] = x;
          U += static_cast<uint32_t>(rtk_popc(bal));
          RTK_WG_SYNC();
      } }
#endif
    // ---- bit vectors of every side unitig: global part, local part (kept in scratch: 2 x 512 B per slot) ----
    uint64_t* const store = reinterpret_cast<uint64_t*>(s.set[RTK_SET_CB_STORE].get());
    { uint32_t slot = 0;
      for (int sd = 0; sd < 3; ++sd) for (uint32_t i = 0; i < sides[sd]->n; ++i, ++slot) {
        const uint32_t u = sides[sd]->u[i]; const int32_t gi = g.gid[u];
        const RtkBM bl = rtk_bm_from_ids(uni, U, scatter, g.col + g.loff[u], static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]));
        rtk_bm_store(store + (2ull * slot) * 64ull, bl);
        const RtkBM bg = gi >= 0 ? rtk_bm_from_ids(uni, U, scatter, g.col + g.goff[gi], static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi])) : rtk_bm_zero();
        rtk_bm_store(store + (2ull * slot + 1ull) * 64ull, bg);
      } }
    rtk_sync();
    // ---- the six anchor classes: side (middle, right, left) x branching / non-branching; G2: the global set alone when there is one ----
    RtkBM a[6];
    for (int sh = 0; sh < 6; ++sh) {
        RtkBM acc = rtk_bm_zero();
        uint32_t slot = (sh % 3 == 0) ? 0u : (sh % 3 == 1 ? side_w.n : side_w.n + side_e.n);
        const SideList& sl = *sides[sh % 3]; const uint8_t want_nb = sh >= 3 ? 1 : 0;
        for (uint32_t i = 0; i < sl.n; ++i, ++slot) {
            if (sl.nb[i] != want_nb) continue;
            const bool has_global = g.gid[sl.u[i]] >= 0;
            acc = acc | rtk_bm_load(store + (2ull * slot + (has_global ? 1ull : 0ull)) * 64ull);
        }
        a[sh] = acc;
    }
    const RtkBM pos0 = a[0] | a[3], pos1 = a[1] | a[4], pos2 = a[2] | a[5];
    const RtkBM a01 = pos0 & pos1, a12 = pos1 & pos2, a02 = pos0 & pos2;
    const RtkBM nobranch_all = a[3] | a[4] | a[5];
    const RtkBM i3 = a01 & a12, i2 = a01 | a12 | a02;
    RtkBM nobranch = nobranch_all, branching = rtk_bm_zero(), prev2 = rtk_bm_zero(), all = rtk_bm_zero();
    uint32_t nb_unselected = nsp;
    for (int i = 5; i >= 0; --i) {
        if (nb_unselected == 0) break;
        RtkBM a2;
        if (i == 5) a2 = nobranch & i3;
        else if (i == 4) { nobranch = rtk_bm_andn(nobranch, prev2); a2 = nobranch & i2; }
        else if (i == 3) { nobranch = rtk_bm_andn(nobranch, prev2); a2 = nobranch; }
        else if (i == 2) { branching = rtk_bm_andn(a[0] | a[1] | a[2], nobranch_all); a2 = branching & i3; }
        else if (i == 1) { branching = rtk_bm_andn(branching, prev2); a2 = branching & i2; }
        else { branching = rtk_bm_andn(branching, prev2); a2 = branching; }
        prev2 = a2;
        if (rtk_bm_count(a2) == 0) continue;
        nb_unselected = 0;
        RtkBM curr = a2;
        for (uint32_t j = 0; j < nsp; ++j) {
            const uint32_t u = rtk_d1_unitig(rtk_ld(keys + j), c.o.d1_desc);
            int quota = static_cast<int>(rtk_ld(vals + j));
            if (quota > 0) {
                const uint64_t slot = rtk_ld(slot_of + j);
                const RtkBM cu = rtk_bm_load(store + (2ull * slot) * 64ull) | rtk_bm_load(store + (2ull * slot + 1ull) * 64ull); // all colours of u
                if (i == 0 || rtk_bm_count(cu & curr) >= 1) {
                    const uint32_t cd = rtk_ld(g.card.get() + u); const uint32_t min_cov = cd < cov ? cd : cov;
                    const uint32_t sh = rtk_bm_count(cu & all);
                    quota = static_cast<int>(min_cov - (sh < min_cov ? sh : min_cov));
                    if (quota > 0) {
                        const uint32_t all_card = rtk_bm_count(all);
                        const RtkBM pid = rtk_bm_lowest(cu & curr, static_cast<uint32_t>(quota));
                        all = all | pid; curr = rtk_bm_andn(curr, pid);
                        const int gained = static_cast<int>(rtk_bm_count(all) - all_card);
                        quota -= gained < quota ? gained : quota;
                    }
                }
            }
            vals[j] = static_cast<uint64_t>(quota);
            nb_unselected += quota > 0 ? 1u : 0u;
        }
        rtk_sync();
    }
    // ---- all_pids back to a sorted id list in set[RTK_SET_ALL_PIDS] ----
    const uint32_t n_all = rtk_bm_count(all);
    if (n_all > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); return 0; }
    uint32_t* out = s.set[RTK_SET_ALL_PIDS];
#ifdef RTK_SIM
    { uint32_t at = 0; for (uint32_t w = 0; w < 64; ++w) { uint64_t x = all.w[w]; while (x) { const int b = __builtin_ctzll(x); out[at++] = uni[64u * w + static_cast<uint32_t>(b)]; x &= x - 1ull; } } }
#else
    { int total; uint32_t at = static_cast<uint32_t>(rtk_wave_excl_scan(rtk_popc(all), &total)); uint64_t x = all;
      while (x) { const int b = __builtin_ctzll(x); out[at++] = uni[64u * static_cast<uint32_t>(rtk_lane()) + static_cast<uint32_t>(b)]; x &= x - 1ull; } }
#endif
    rtk_sync();
    return n_all;
}

// ------------------------------------------------------------------------------------------------ dispatcher and general program
// Computes all_pids into set[RTK_SET_ALL_PIDS]; returns its size. Every other member of `set` is its temporary (RtkSet).
RTK_FN uint32_t rtk_choose_colors_general(const RCtx& c_, const SideList& side_s_, const SideList& side_e_, const SideList& side_w_);
// chooseColors: the two register / bit-vector programs of rtk_colours.h first (nearly every region), the general program below otherwise.
// Compiled into its caller: the dispatcher itself as a function would save 17 register rows on every region for a path it almost never takes.
// Every call that ends without an overflow is counted by the program that answered it (RTK_RC_COLOURS_*; the small program counts its own two sizes, and the
// calls it hands on because universe and bit vectors do not fit its LDS buffer: RTK_RC_COLOURS_DECLINED_FIT).
// OptsView::colours_mode (tests): RTK_CM_ROUTE_BITS skips the small program, RTK_CM_ROUTE_GENERAL both bit-vector programs. RTK_CM_AUDIT: where a bit-vector
// program answered, its list is kept in the region-level arena (free here: the path search resets it after this call; the general program writes every other member of `set`,
// arena level RTK_ARENA_COL_SETS, list[RTK_L_COL_VALS], list[RTK_L_COL_KEYS] and the LDS buffer), the general program selects again into set[RTK_SET_ALL_PIDS], and a difference in the number of ids or in any id is
// counted. The region goes on with the general program's list. RTK_CM_FAULT (test hook): the kept list loses its largest id first.
RTK_DEV uint32_t rtk_choose_colors(const RCtx& c, const SideList& side_s, const SideList& side_e, const SideList& side_w) {
    RegionScratch& s = rtk_hdr(c);
    const unsigned long long tf = rtk_clock();
    const uint32_t cm = rtk_u(c.o.colours_mode);
    uint32_t r = RTK_NONE32;
#ifndef RTK_SIM
    if ((cm & RTK_CM_ROUTE) == 0u) {
        r = rtk_u(rtk_choose_colors_small(c, side_s, side_e, side_w));
        if (r != RTK_NONE32) { const unsigned long long d_ = rtk_clock() - tf; s.fine[RTK_FINE_COL_UNIONS] += d_; s.fine[RTK_FINE_COL_S_CYCLES] += d_; s.fine[RTK_FINE_COL_S_CALLS] += 1; }
    }
#endif
    if (r == RTK_NONE32 && (cm & RTK_CM_ROUTE) != RTK_CM_ROUTE_GENERAL) {
        r = rtk_u(rtk_choose_colors_bits(c, side_s, side_e, side_w));
        if (r != RTK_NONE32) { const unsigned long long d_ = rtk_clock() - tf; s.fine[RTK_FINE_COL_UNIONS] += d_; s.fine[RTK_FINE_COL_B_CYCLES] += d_; s.fine[RTK_FINE_COL_B_CALLS] += 1; if (!rtk_failed(s)) s.cnt[RTK_RC_COLOURS_BITS] += 1; }
    }
    uint32_t n_first = RTK_NONE32; // audit: ids of the first answer that were kept
    if (r != RTK_NONE32) {
        if (rtk_failed(s)) return 0;
        if ((cm & RTK_CM_AUDIT) == 0u || 4ull * r > s.arena_cap) return r; // (no room to keep the list: not compared)
        n_first = r - (((cm & RTK_CM_FAULT) != 0u && r != 0u) ? 1u : 0u);
        rtk_wcopy(s.arena[RTK_ARENA_COL_AUDIT].get(), s.set[RTK_SET_ALL_PIDS].get(), 4ull * n_first);
    }
    const uint32_t rg = rtk_u(rtk_choose_colors_general(c, side_s, side_e, side_w));
    if (rtk_failed(s)) return 0; // (the region is redone: nothing to compare)
    if (n_first == RTK_NONE32) { s.cnt[RTK_RC_COLOURS_GENERAL] += 1; return rg; }
    const uint32_t* const first = reinterpret_cast<const uint32_t*>(s.arena[RTK_ARENA_COL_AUDIT].get()); const uint32_t* const second = s.set[RTK_SET_ALL_PIDS].get();
    bool differs = rg != n_first;
    for (uint32_t i0 = 0; i0 < rg && !differs; i0 += RTK_WAVE) { const uint32_t i = i0 + static_cast<uint32_t>(rtk_lane()); differs = rtk_ballot(i < rg && first[i] != second[i]) != 0ull; }
    if (differs) s.cnt[RTK_RC_COLOURS_AUDIT_MISMATCH] += 1;
    return rg;
}
RTK_FN uint32_t rtk_choose_colors_general(const RCtx& c_, const SideList& side_s_, const SideList& side_e_, const SideList& side_w_) {
    const RCtx& c = *rtk_u(&c_); const SideList& side_s = *rtk_u(&side_s_); const SideList& side_e = *rtk_u(&side_e_); const SideList& side_w = *rtk_u(&side_w_); RTK_ASSUME_LDS(&side_s); RTK_ASSUME_LDS(&side_e); RTK_ASSUME_LDS(&side_w);
    RegionScratch& s = rtk_hdr(c);
    const GraphView& g = c.g;
    unsigned long long tf = rtk_clock();
    // a_pid[shift], shift = side index (0 middle, 1 right, 2 left) + 3 * nonbranching: built one after the other into the arena (level RTK_ARENA_COL_SETS, the DFS level, is free here)
    s.top[RTK_ARENA_COL_SETS] = 0;
    tf = rtk_clock();
#define RTK_FINE_LAP(i) { const unsigned long long tn_ = rtk_clock(); s.fine[i] += tn_ - tf; tf = tn_; }
    const SideList* sides[3] = {&side_w, &side_e, &side_s};
    const uint32_t* a_ptr[6]; uint32_t a_n[6];
    for (int sh = 0; sh < 6 && !rtk_failed(s); ++sh) {
        const SideList& sl = *sides[sh % 3]; const uint8_t want_nb = sh >= 3 ? 1 : 0;
        int cur = RTK_SET_UNION_A; uint32_t n = 0, n_src = 0; const uint32_t* one = nullptr;
        for (uint32_t i = 0; i < sl.n && !rtk_failed(s); ++i) {
            if (sl.nb[i] != want_nb) continue;
            const uint32_t u = sl.u[i];
            const int32_t gi = g.gid[u]; // G2: only the global set when there is one
            const uint32_t* src = gi >= 0 ? g.col + g.goff[gi] : g.col + g.loff[u];
            const uint32_t ns = gi >= 0 ? static_cast<uint32_t>(g.goff[gi + 1] - g.goff[gi]) : static_cast<uint32_t>(g.loff[u + 1] - g.loff[u]);
            s.cnt[RTK_RC_COLOUR] += ns;
            if (ns == 0) continue;
            // a class fed by ONE anchor set (the usual case: a region is flanked by a unitig or two) is that set: used where it lies in
            // the graph's colour pool, neither merged nor copied
            if (n_src == 0) { one = src; n = ns; n_src = 1; continue; }
            if (n_src == 1) { if (n > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); break; } rtk_wcopy(s.set[cur], one, 4ull * n); rtk_sync(); }
            n = rtk_rs_union(s, cur, n, src, ns, cur ^ 3); cur ^= 3; ++n_src; // ping-pong between set[RTK_SET_UNION_A] and set[RTK_SET_UNION_B]
#ifdef RTK_SIM
            rtk_sim_site_stat[29][4] += 1;
#endif
        }
        a_n[sh] = n;
        if (n_src <= 1) a_ptr[sh] = n_src ? one : reinterpret_cast<const uint32_t*>(s.arena[RTK_ARENA_COL_SETS].get());
        else {
            const uint64_t off = rtk_arena_alloc(s, RTK_ARENA_COL_SETS, 4ull * n + 4);
            if (!rtk_failed(s)) rtk_wcopy(s.arena[RTK_ARENA_COL_SETS] + off, s.set[cur], 4ull * n);
            a_ptr[sh] = reinterpret_cast<const uint32_t*>(s.arena[RTK_ARENA_COL_SETS] + off);
        }
    }
    if (rtk_failed(s)) return 0;
#ifdef RTK_SIM
    { std::atomic<unsigned long long>* t = rtk_sim_site_stat[29]; t[0] += 1; t[1] += side_s.n; t[2] += side_e.n; t[3] += side_w.n; for (int i = 0; i < 6; ++i) rtk_sim_site_stat[30][i] += a_n[i];
      unsigned long long tot = 0; for (int i = 0; i < 6; ++i) tot += a_n[i]; int b = 0; while (b < 7 && (256ull << b) <= tot) ++b; rtk_sim_site_stat[31][b] += 1; }
#endif
    RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 0)
    auto A = [&](int i) -> const uint32_t* { return a_ptr[i]; };
    // candidate anchors: cardinality >= min_cov_vertices, ordered by (cardinality, unitig id) [D1]
    uint64_t* keys = s.list[RTK_L_COL_KEYS]; uint64_t* vals = s.list[RTK_L_COL_VALS];
    uint32_t nsp = 0;
    for (int sd = 0; sd < 3; ++sd) for (uint32_t i = 0; i < sides[sd]->n; ++i) {
        const uint32_t u = sides[sd]->u[i];
        if (g.card[u] < c.o.min_cov_vertices) continue;
        bool dup = false; for (uint32_t j0 = 0; j0 < nsp && !dup; j0 += RTK_WAVE) { const uint32_t j = j0 + static_cast<uint32_t>(rtk_lane()); dup = rtk_ballot(j < nsp && rtk_d1_unitig(keys[j], c.o.d1_desc) == u) != 0ull; }
        if (dup) continue;
        if (2 * (nsp + 1) > s.list_cap) { rtk_fail_ovf(s, RTK_OVF_LIST); return 0; }
        keys[nsp] = rtk_d1_key(g.card[u], u, c.o.d1_desc); vals[nsp] = 0; ++nsp; rtk_sync();
    }
    rtk_sort_pairs(keys, vals, nsp);
    RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 1)
    const uint32_t cov = 30;
    for (uint32_t j = 0; j < nsp; ++j) { const uint32_t cd = static_cast<uint32_t>(keys[j] >> 32); vals[j] = cd < cov ? cd : cov; } // remaining quota (p_spid.second)
    // Set expressions of src/Correction.cpp:233-275,300-352 on immutable operands: a result is either one of its operands (union with
    // / difference by the empty set -- the usual case: most regions have no weak anchor, so the whole "middle" side is empty) or a
    // fresh slice of the DFS-level arena; nothing is copied to be kept, and a class only computes what it reads.
    struct SetRef { const uint32_t* p; uint32_t n; };
    const SetRef EMPTY = { reinterpret_cast<const uint32_t*>(s.arena[RTK_ARENA_COL_SETS].get()), 0u };
    auto alloc = [&](uint32_t n) -> uint32_t* { const uint64_t off = rtk_arena_alloc(s, RTK_ARENA_COL_SETS, 4ull * n + 4); return rtk_failed(s) ? nullptr : reinterpret_cast<uint32_t*>(s.arena[RTK_ARENA_COL_SETS] + off); };
    auto Un = [&](SetRef a, SetRef b) -> SetRef {
        if (!a.n) return b; if (!b.n) return a;
        if (a.n + b.n > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); return EMPTY; } // set[RTK_SET_UNION_TMP] holds b \ a
        uint32_t* o = alloc(a.n + b.n); if (!o) return EMPTY;
        SetRef r; r.p = o; r.n = rtk_set_union(a.p, a.n, b.p, b.n, o, s.set[RTK_SET_UNION_TMP]); return r; };
    auto In = [&](SetRef a, SetRef b) -> SetRef {
        if (!a.n || !b.n) return EMPTY;
        if (a.n > b.n) { const SetRef t = a; a = b; b = t; } // walk the smaller set, search the larger one
        uint32_t* o = alloc(a.n); if (!o) return EMPTY;
        SetRef r; r.p = o; r.n = rtk_set_inter(a.p, a.n, b.p, b.n, o); return r; };
    auto Di = [&](SetRef a, SetRef b) -> SetRef {
        if (!a.n) return EMPTY; if (!b.n) return a;
        uint32_t* o = alloc(a.n); if (!o) return EMPTY;
        SetRef r; r.p = o; r.n = rtk_set_diff(a.p, a.n, b.p, b.n, o); return r; };
    SetRef a[6]; for (int i = 0; i < 6; ++i) { a[i].p = a_ptr[i]; a[i].n = a_n[i]; }
    const SetRef pos0 = Un(a[0], a[3]), pos1 = Un(a[1], a[4]), pos2 = Un(a[2], a[5]);
    const SetRef a01 = In(pos0, pos1), a12 = In(pos1, pos2), a02 = In(pos0, pos2);
    const SetRef nobranch_all = Un(Un(a[3], a[4]), a[5]);
    if (rtk_failed(s)) return 0;
    RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 2)
    uint32_t n_all = 0; int allb = RTK_SET_ALL_PIDS; // all_pids lives in set[RTK_SET_ALL_PIDS] (while it is being built: in set[allb])
    uint32_t nb_unselected = nsp;
    SetRef nobranch = nobranch_all, branching = EMPTY, i3 = EMPTY, i2 = EMPTY, prev2 = EMPTY; // prev2: a_pid2 of the previous class
    bool have_i3 = false, have_i2 = false;
    for (int i = 5; i >= 0 && !rtk_failed(s); --i) {
        if (nb_unselected == 0) break;
        if ((i == 5 || i == 2) && !have_i3) { i3 = In(a01, a12); have_i3 = true; }
        if ((i == 4 || i == 1) && !have_i2) { i2 = Un(Un(a01, a12), a02); have_i2 = true; }
        SetRef a2 = EMPTY; // a_pid2[i]
        if (i == 5) a2 = In(nobranch, i3);
        else if (i == 4) { nobranch = Di(nobranch, prev2); a2 = In(nobranch, i2); }
        else if (i == 3) { nobranch = Di(nobranch, prev2); a2 = nobranch; }
        else if (i == 2) { branching = Di(Un(Un(a[0], a[1]), a[2]), nobranch_all); a2 = In(branching, i3); }
        else if (i == 1) { branching = Di(branching, prev2); a2 = In(branching, i2); }
        else { branching = Di(branching, prev2); a2 = branching; }
        const uint32_t n2 = a2.n;
        if (rtk_failed(s)) break;
        prev2 = a2; // a_pid2[i] is needed by the next class
        RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 3)
        if (n2 != 0) {
            nb_unselected = 0;
            const uint32_t* cur_p = a2.p; uint32_t ncur = n2; int curb = RTK_SET_CUR_B; // curr_pid: a_pid2[i] itself until the first selection, then set[RTK_SET_CUR_A] / set[RTK_SET_CUR_B] (ping-pong)
            for (uint32_t j = 0; j < nsp && !rtk_failed(s); ++j) {
                const uint32_t u = rtk_d1_unitig(keys[j], c.o.d1_desc);
                int quota = static_cast<int>(vals[j]);
                bool touch = false;
                if (quota > 0) { touch = (i == 0 || rtk_shared_with_set(g, u, cur_p, ncur, 1) >= 1); RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 4) }
#ifdef RTK_SIM
                rtk_sim_site_stat[29][5] += 1; if (touch) rtk_sim_site_stat[29][6] += 1;
#endif
                if (touch) {
                    const uint32_t min_cov = g.card[u] < cov ? g.card[u] : cov;
                    const uint32_t sh = rtk_shared_with_set(g, u, s.set[allb], n_all, min_cov);
                    RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 5)
                    quota = static_cast<int>(min_cov - (sh < min_cov ? sh : min_cov));
                    if (quota > 0) {
                        const uint32_t all_card = n_all;
                        // pid = (global & curr) | (local & curr), truncated to its `quota` lowest ids
                        const uint32_t npid = rtk_first_shared(g, u, cur_p, ncur, static_cast<uint32_t>(quota), s.set[RTK_SET_PICKED]);
                        if (n_all + npid > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); break; }
                        const uint32_t nn = rtk_set_union(s.set[allb], n_all, s.set[RTK_SET_PICKED], npid, s.set[allb ^ 3], s.set[RTK_SET_UNION_TMP]);
                        allb ^= 3; n_all = nn; // all_pids alternates between set[RTK_SET_ALL_PIDS] and set[RTK_SET_ALL_PIDS_ALT]; it is moved to the former once, at the end
                        const int nb2 = curb == RTK_SET_CUR_B ? RTK_SET_CUR_A : RTK_SET_CUR_B;
                        if (ncur > s.set_cap) { rtk_fail_ovf(s, RTK_OVF_SET); break; }
                        ncur = rtk_set_diff(cur_p, ncur, s.set[RTK_SET_PICKED], npid, s.set[nb2]); curb = nb2; cur_p = s.set[nb2];
#ifdef RTK_SIM
                        rtk_sim_site_stat[29][7] += 1; rtk_sim_site_stat[30][6] += ncur; rtk_sim_site_stat[30][7] += n_all;
#endif
                        const int gained = static_cast<int>(n_all - all_card);
                        quota -= gained < quota ? gained : quota;
                        RTK_FINE_LAP(RTK_FINE_COL_GENERAL + 6)
                    }
                }
                vals[j] = static_cast<uint64_t>(quota);
                nb_unselected += quota > 0 ? 1u : 0u;
            }
        }
    }
    if (allb != RTK_SET_ALL_PIDS && !rtk_failed(s)) rtk_wcopy(s.set[RTK_SET_ALL_PIDS], s.set[RTK_SET_ALL_PIDS_ALT], 4ull * n_all);
    return rtk_failed(s) ? 0 : n_all;
}

#endif
