// Anchor stage, 1-edit k-mer search by half-k-mer seeds (the default; src/Graph.cpp:193 [A2], same hit sets as rtk_seed_enum.h). One wavefront owns one tile of 64
// window positions.
#ifndef RTK_SEED_SEEDED_H
#define RTK_SEED_SEEDED_H

#include "rtk_acgt.h"
#include "rtk_seed_types.h"
#include "rtk_seed_window.h"
#include "rtk_types.h"
#include "rtk_wave.h"

// ---------------------------------------------------------------------------------------------- 1-edit search by half-k-mer seeds ([A2], same hit sets as above)
// A graph k-mer G one edit away from a read window keeps its first h or its last h characters (h = (k-1)/2, the middle character
// belongs to neither half): the edit cannot touch both. So instead of spelling the ~246 variants of a window and probing each, a lane
// looks up the read h-mers that would be G's first half (1 key) or G's last half (3 keys: substitution, graph-has-extra-base, graph-
// lacks-a-base shift the second half by 0 / -1 / +1) in the index of all unitig h-mers (GraphView::hx), in both orientations, and
// checks the k-mers those h-mers belong to with three XOR / count-leading-zero tests. One lane per window.

RTK_DEV uint64_t rtk_rev2(uint64_t x, int n) { // reverses the order of the n 2-bit groups held in the low 2n bits
    uint64_t y = rtk_brev64(x);
    y = ((y & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((y & 0x5555555555555555ull) << 1);
    return (n >= 32) ? y : (y >> (64 - 2 * n));
}
RTK_DEV uint64_t rtk_pool_kmer(const GraphView& g, uint64_t gp, int k) { // 2-bit code (first base in the high bits) of the k bases of the unitig pool at gp
    const uint64_t w0 = g.useq[gp >> 5], w1 = g.useq[(gp >> 5) + 1];
    const int sh = static_cast<int>(2 * (gp & 31ull));
    uint64_t lsb = sh ? ((w0 >> sh) | (w1 << (64 - sh))) : w0;
    if (k < 32) lsb &= (1ull << (2 * k)) - 1ull;
    return rtk_rev2(lsb, k);
}
RTK_DEV int rtk_clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }
RTK_DEV int rtk_ctz64(uint64_t x) { return x ? __builtin_ctzll(x) : 64; }

// which 1-edit variants of the window whose first k-1 characters are w_k1 (and ck, ck1 the next two, 4 = unusable) is G? (oracle: searchInexact)
// bit 0 substitution, bit 1 graph k-mer has an extra base ("insertion"), bit 2 graph k-mer lacks a read base ("deletion"); 0 = none.
// want = the kinds that matter to the caller: the tests stop at the first of them that holds when only "any" is asked for.
RTK_DEV uint32_t rtk_one_edit(uint64_t G, int k, uint64_t w_k1, uint32_t ck, uint32_t ck1, bool all_kinds) {
    const uint64_t mk = (k < 32) ? ((1ull << (2 * k)) - 1ull) : ~0ull, mk1 = (1ull << (2 * (k - 1))) - 1ull;
    uint32_t kinds = 0;
    if (ck <= 3) { // substitution: exactly one differing character
        const uint64_t x = (G ^ ((w_k1 << 2) | static_cast<uint64_t>(ck))) & mk;
        if (rtk_popc((x | (x >> 1)) & 0x5555555555555555ull) == 1) { kinds |= RTK_EDIT_SUB; if (!all_kinds) return kinds; }
    }
    { // G = the k-1 read characters with one base inserted anywhere: common prefix + common suffix cover the k-1 characters
        const uint64_t xp = ((G >> 2) ^ w_k1) & mk1, xs = (G ^ w_k1) & mk1;
        const int lcp = xp ? (rtk_clz64(xp) - (64 - 2 * (k - 1))) / 2 : k - 1, lcs = xs ? rtk_ctz64(xs) / 2 : k - 1;
        if (lcp + lcs >= k - 1) { kinds |= RTK_EDIT_INS; if (!all_kinds) return kinds; }
    }
    if (ck <= 3 && ck1 <= 3) { // G = the k+1 read characters without one interior character (offset 1..k-2)
        const uint64_t S = (w_k1 << 4) | (static_cast<uint64_t>(ck) << 2) | static_cast<uint64_t>(ck1);
        const uint64_t xp = (G ^ (S >> 2)) & mk, xs = (G ^ S) & mk;
        const int lcp = xp ? (rtk_clz64(xp) - (64 - 2 * k)) / 2 : k, lcs = xs ? rtk_ctz64(xs) / 2 : k;
        const int lo = (k - lcs) > 1 ? (k - lcs) : 1, hi = lcp < (k - 2) ? lcp : (k - 2);
        if (lo <= hi) kinds |= RTK_EDIT_DEL;
    }
    return kinds;
}

// visits (code, hit) of every graph k-mer that is a 1-edit variant of the window and contains one of its seed h-mers; a k-mer reached
// through two seeds is visited twice (the hits of a window are reduced to distinct k-mers downstream, src/Graph.cpp:201-216)
// One look-up of a canonical h-mer c in the index: the probe chain over hx[], then the count word of its list. -> found; *first = the list's count word in hxl[].
RTK_DEV bool rtk_hx_find(const uint64_t* hx, uint64_t hx_mask, const uint64_t* hxl, uint64_t c, uint64_t* first, uint32_t* cnt, uint32_t* n_slots) {
    uint64_t i = rtk_hash64(c) & hx_mask;
    while (true) { const uint64_t sv = hx[i]; *n_slots += 1; if (sv == RTK_EMPTY_KEY) return false; if ((sv >> 34) == c) { *first = sv & 0x3FFFFFFFFull; *cnt = static_cast<uint32_t>(hxl[*first]); return true; } i = (i + 1) & hx_mask; }
}
// Where a window gets the list of its seed q (canonical h-mer c) from: lookup(q, c, &first, &cnt) -> found.
//   RtkHxProbe   the window asks the index itself (RTK_INEXACT_SHARED=0)
//   RtkHxShared  the tile has looked every read position up once, the window reads the answer of position p + offset_q from the tile's table
struct RtkHxProbe {
    const uint64_t* hx; uint64_t hx_mask; const uint64_t* hxl; uint32_t* n_lookups; uint32_t* n_slots;
    RTK_DEV bool operator()(int, uint64_t c, uint64_t* first, uint32_t* cnt) const { *n_lookups += 1; return rtk_hx_find(hx, hx_mask, hxl, c, first, cnt, n_slots); }
};
#define RTK_HXT_N 96          // entries of a tile's table: the 64 + (k + 1 - h) <= 82 read positions its windows can ask for (k <= 32)
#define RTK_HXT_NOT_ASKED RTK_EMPTY_KEY // `first` of a position no candidate window of the tile asks for (cnt 0 with any other `first`: asked, not in the index)
struct RtkHxShared {
    const uint64_t* tab_first; const uint32_t* tab_cnt; int at, d1; // at = the window's position in the tile, d1 = k - 1 - h
    RTK_DEV bool operator()(int q, uint64_t, uint64_t* first, uint32_t* cnt) const { const int j = at + (q ? d1 - 1 + q : 0); *first = tab_first[j]; *cnt = tab_cnt[j]; return *cnt != 0u; }
};

template <class LK, class V>
RTK_DEV void rtk_seeded_window(const uint64_t* hxl, int k, uint64_t w_k1, uint32_t ck, uint32_t ck1, uint32_t* n_slots, bool all_kinds, LK lookup, V visit) { // visit(code, hit, kinds)
    const int h = (k - 1) / 2;
    const uint64_t hm = (1ull << (2 * h)) - 1ull;
    // the window's characters as one code of k + 1 (ck / ck1 = 0 where the read has none: those keys are not asked for). The four seed h-mers are shifts of it:
    //   q = 0  m[p .. p+h)              first half of G
    //   q = 1  m[p+k-1-h .. p+k-1)      last half when the graph k-mer has an extra base
    //   q = 2  m[p+k-h .. p+k)          last half, substitution              (needs ck)
    //   q = 3  m[p+k+1-h .. p+k+1)      last half, a read base missing in G  (needs ck and ck1)
    // The keys are computed where they are used: arrays of them indexed by the loop variable spill to the lane's stack.
    const uint64_t S_all = (w_k1 << 4) | (static_cast<uint64_t>(ck <= 3 ? ck : 0u) << 2) | static_cast<uint64_t>(ck1 <= 3 ? ck1 : 0u);
    const int nkeys = (ck <= 3) ? ((ck1 <= 3) ? 4 : 3) : 2;
    // One key after the other, each with its own chain of loads: the look-ups of six waves per SIMD overlap as they are, and arrays of slots in flight together spill
    // (DESIGN.md 3.3). The index is keyed by the CANONICAL h-mer (the smaller of an h-mer and its reverse complement): one look-up per read h-mer finds the places where
    // it stands in a unitig as it is AND those where its reverse complement does (bit 63 of a place: the unitig holds the reverse complement of the key). `lookup` is
    // RtkHxShared on the default route, where the tile has looked every read position up once (profiles/inexact_shared_lookups.txt), and RtkHxProbe under RTK_INEXACT_SHARED=0.
    for (int q = 0; q < nkeys; ++q) {
        const bool first_half_q = q == 0;
        const uint64_t kq = (S_all >> (q == 0 ? 2 * (k - 1 - h) + 4 : 2 * (3 - q))) & hm, rq = rtk_revcomp(kq, h);
        const uint64_t c = kq < rq ? kq : rq;
        uint64_t first = 0; uint32_t cnt = 0;
        if (!lookup(q, c, &first, &cnt)) continue;
        ++first;
        const bool palin = kq == rq; // (even h only: the h-mer reads the same on both strands, every place is a place of both orientations)
        for (uint32_t e = 0; e < cnt; ++e) {
            // a place is two words: the h + 1 bases behind / in front of the h-mer, then reversed << 63 | unitig << 32 | following-bases-exist << 31 | offset (bit 31 = `a_ok` of the two builders: the h + 1 bases that FOLLOW the h-mer in the forward unitig sequence exist): the candidate k-mer is the
            // h-mer with one of its flanks, the entry alone verifies it (the unitig's bounds and its sequence would be two more dependent cache lines each)
            const uint64_t fl = hxl[first + 2ull * e], ent = hxl[first + 2ull * e + 1ull];
            *n_slots += 2; // a candidate costs its 16-byte list entry
            const uint64_t x = (ent >> 63) ? (c == kq ? rq : kq) : c; // the h-mer as the unitig spells it
            const uint32_t u = static_cast<uint32_t>(ent >> 32) & 0x7FFFFFFFu, pos = static_cast<uint32_t>(ent & 0x7FFFFFFFull);
            for (int ori = (x == kq ? 0 : 1), last = (palin ? 1 : ori); ori <= last; ++ori) { // ori 1: the unitig spells the reverse complement of the read's h-mer
                // the unitig h-mer is the first half of the forward k-mer F starting there, or the last half of the one starting h+1 earlier;
                // read-oriented G = F when the read h-mer itself was found, its reverse complement when the reverse-complemented key was
                const bool at_start = (first_half_q != (ori != 0));
                int64_t t; uint64_t F;
                if (at_start) { if (!((ent >> 31) & 1ull)) continue; t = pos; F = (x << (2 * (h + 1))) | (fl >> 32); }
                else { if (pos < static_cast<uint32_t>(h + 1)) continue; t = static_cast<int64_t>(pos) - (h + 1); F = ((fl & 0xFFFFFFFFull) << (2 * h)) | x; }
                const uint64_t G = ori ? rtk_revcomp(F, k) : F;
                const uint32_t kinds = rtk_one_edit(G, k, w_k1, ck, ck1, all_kinds);
                if (kinds) visit(G, rtk_pack_hit(u, static_cast<uint32_t>(t), ori ? 0u : 1u), kinds);
            }
        }
    }
}

#ifndef RTK_SEED_REGS
#define RTK_SEED_REGS 4 // distinct hits of a window kept in registers; windows with more take the counted slow path
#endif
// OptsView::inexact_route: the old routes of rtk_inexact_tile_seeded, kept in the same binary (rtk_knobs.h)
#define RTK_IR_PER_WINDOW 1u // RTK_INEXACT_SHARED=0: every window asks the index itself
#define RTK_IR_TEXT_PACK 2u  // RTK_INEXACT_PLANES=0: every lane packs its characters from text (rtk_pack_acgt)
#ifndef RTK_SIM
// v of lane src (src from the caller's own lane number: __shfl derives its index from a lane id of its own, one more value the compiler holds across the tiles)
RTK_DEV uint64_t rtk_bpermute64(uint64_t v, int src) {
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, static_cast<int>(static_cast<uint32_t>(v))), hi = __builtin_amdgcn_ds_bpermute(src << 2, static_cast<int>(static_cast<uint32_t>(v >> 32)));
    return (static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo);
}
#endif
// exclusive prefix sum across the lanes of a value below 2^nbits: one ballot per bit, a lane's share of it is the count of set bits below the lane (rtk_wave_excl_scan
// takes six shuffles and the six lane indices they read from, which the compiler keeps in registers across the tiles of a wave)
RTK_DEV int rtk_wave_excl_scan_bits(int v, int nbits, int* total) {
#ifdef RTK_SIM
    (void)nbits; *total = v; return 0;
#else
    int off = 0, tot = 0;
    for (int b = 0; b < nbits; ++b) {
        const uint64_t m = rtk_ballot(((v >> b) & 1) != 0);
        off += static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u))) << b;
        tot += rtk_popc(m) << b;
    }
    *total = tot; return off;
#endif
}

// One tile in three steps. (1) Every lane's window: candidate or not, its codes. (2) RTK_INEXACT_SHARED: the h-mer that starts at read position x is the seed of up to
// four windows (x, x - (k-1-h), x - (k-h), x - (k+1-h)); the positions that a candidate window of the tile asks for are looked up ONCE, one per lane (the lanes below
// k + 1 - h take a second one from the overhang behind the tile), and the answers (list start, count) stand in a table in LDS. (3) The windows, one per lane, with their
// seeds in the order q = 0 .. 3 as before; they read the table where they used to probe. The simulator takes the same three steps with its one lane.
RTK_DEV void rtk_inexact_tile_seeded(const GraphView& g, const BatchView& bv, uint64_t tile, unsigned long long* acc_probes, unsigned long long* acc_slots, unsigned long long* acc_hits, PoolChunk* chunk, uint32_t exclusive, uint32_t route) {
    const int k = g.k, h = (k - 1) / 2, d1 = k - 1 - h, d3 = k + 1 - h;
    const bool shared = !(route & RTK_IR_PER_WINDOW) && 64 + d3 <= RTK_HXT_N;
    const uint64_t* const roff = bv.roff; const uint32_t n_reads = bv.n_reads;
    const unsigned char* const text = reinterpret_cast<const unsigned char*>(bv.masked.get());
    const uint64_t* const hx = g.hx; const uint64_t hx_mask = g.hx_mask; const uint64_t* const hxl = g.hxl;
    const uint32_t lo_tile = rtk_owner_read(roff, n_reads, tile * 64); // one scalar search per tile: largest r with roff[r] <= first base of the tile
    const auto window_code = rtk_window_coder(bv, roff, n_reads, lo_tile, text, k); // (1) the window at bb (rtk_seed_window.h)
#ifdef RTK_SIM
    const int n_sub = 64; // the 1-lane simulator visits the 64 positions of the tile one after the other, in each of the three steps
    RtkWinCode win[64]; uint64_t tab_first[RTK_HXT_N]; uint32_t tab_cnt[RTK_HXT_N]; uint64_t st_[2 * RTK_SEED_REGS];
#define RTK_ST(i, w) st_[2 * (i) + (w)]
    uint64_t C = 0, C3 = 0, C4 = 0; // the tile's candidate windows / those with k / with k + 1 usable characters
    for (int sub = 0; sub < n_sub; ++sub) {
        const RtkWinCode w = win[sub] = window_code(tile * 64 + static_cast<uint64_t>(sub), false, 0, 0);
        if (w.cand) { C |= 1ull << sub; if (w.ck <= 3u) C3 |= 1ull << sub; if (w.ck1 <= 3u) C4 |= 1ull << sub; }
    }
#else
    const int n_sub = 1;
    __shared__ uint64_t tab_first[RTK_HXT_N]; __shared__ uint32_t tab_cnt[RTK_HXT_N];
    // pass 1 of a window stages up to four distinct hits in LDS (64 lanes x 4 hits x 16 bytes = 4 KB per wave, word (2 i + w) of lane l at [(2 i + w) * 64 + l]),
    // their kinds of edit packed into one register: arrays indexed by my_n spill to the lane's stack, 20 registers indexed by constants do not fit the kernel's 80
    // (six waves per SIMD). A hit is rare (3 % of the windows), its staging may be slow.
    __shared__ uint64_t rtk_inexact_stage[2 * RTK_SEED_REGS * RTK_WAVE];
    uint64_t* const st_ = rtk_inexact_stage + rtk_lane();
#define RTK_ST(i, w) st_[(2 * (i) + (w)) * RTK_WAVE]
    const uint64_t bb = tile * 64 + static_cast<uint64_t>(rtk_lane());
    // RTK_INEXACT_PLANES, k <= 31: the tile's 64 + 64 characters of the masked copy as bit planes (one character of each half per lane, three ballots per half: low bit, high bit, is-a-base), as k_lookup_exact has them. A lane's
    // k + 1 characters are k + 1 bits of each plane from its own position on, reversed (the first character sits in the high bits of a code) and interleaved; the
    // leading A/C/G/T are the trailing ones of the shifted is-a-base plane. (rtk_pack_acgt: four unaligned words and two 64-bit multiplies each, per lane.)
    const bool planes = !(route & RTK_IR_TEXT_PACK) && k <= 31;
    uint64_t S = 0; int n_ok = 0;
    if (planes) {
        const uint64_t a1 = bb + 64;
        const unsigned char ca = bb < bv.n_bases ? text[bb] : 'N', cb = a1 < bv.n_bases ? text[a1] : 'N';
        const bool va = ca == 'A' || ca == 'C' || ca == 'G' || ca == 'T', vb = cb == 'A' || cb == 'C' || cb == 'G' || cb == 'T';
        const uint32_t b1a = (ca >> 1) & 1u, b2a = (ca >> 2) & 1u, b1b = (cb >> 1) & 1u, b2b = (cb >> 2) & 1u; // bits 1-2 of 'A' 0x41, 'C' 0x43, 'G' 0x47, 'T' 0x54: code = b2 : b1 ^ b2
        const uint64_t L0a = rtk_ballot((b1a ^ b2a) != 0), L1a = rtk_ballot(b2a != 0), Va = rtk_ballot(va), L0b = rtk_ballot((b1b ^ b2b) != 0), L1b = rtk_ballot(b2b != 0), Vb = rtk_ballot(vb);
        const int sh = rtk_lane(), kk = k + 1;
        const uint64_t p0 = sh ? ((L0a >> sh) | (L0b << (64 - sh))) : L0a, p1 = sh ? ((L1a >> sh) | (L1b << (64 - sh))) : L1a, pv = sh ? ((Va >> sh) | (Vb << (64 - sh))) : Va;
        S = (rtk_spread32(rtk_brev64(p1) >> (64 - kk)) << 1) | rtk_spread32(rtk_brev64(p0) >> (64 - kk));
        n_ok = rtk_ctz64(~pv); if (n_ok > kk) n_ok = kk;
    }
    const RtkWinCode me = window_code(bb, planes, S, n_ok);
    const uint64_t C = rtk_ballot(me.cand), C3 = rtk_ballot(me.cand && me.ck <= 3u), C4 = rtk_ballot(me.cand && me.ck1 <= 3u);
#endif
    uint32_t lookups = 0, slots = 0; // this lane's tallies of the tile
    // (2) the read positions (relative to the tile: 0 .. 63 + d3) that a candidate window asks for: seed 0 at its own position, 1 at + d1, 2 at + d1 + 1 (needs ck), 3 at
    // + d3 (needs ck1). A position nobody asks for is not looked up, so the look-ups made are a subset of those the windows would make on their own. The h characters
    // of an asked position are A/C/G/T and belong to the asking window's read; which window may use them was decided in (1).
    if (shared && C) {
        const uint64_t need_lo = C | (C << d1) | (C3 << (d1 + 1)) | (C4 << d3), need_hi = (C >> (64 - d1)) | (C3 >> (63 - d1)) | (C4 >> (64 - d3));
#ifdef RTK_SIM
        for (int j = 0; j < 64 + d3; ++j) {
            tab_first[j] = RTK_HXT_NOT_ASKED; tab_cnt[j] = 0;
            if (!(((j < 64) ? (need_lo >> j) : (need_hi >> (j - 64))) & 1ull)) continue;
            int t; const uint64_t kq = rtk_pack_acgt(text + tile * 64 + static_cast<uint64_t>(j), h, &t), rq = rtk_revcomp(kq, h);
            lookups += 1; tab_first[j] = 0;
            uint64_t f = 0; uint32_t n = 0;
            if (rtk_hx_find(hx, hx_mask, hxl, kq < rq ? kq : rq, &f, &n, &slots)) { tab_first[j] = f; tab_cnt[j] = n; }
        }
#else
        const int lane = rtk_lane();
        const uint64_t hm = (1ull << (2 * h)) - 1ull;
        const bool needA = __builtin_amdgcn_inverse_ballot_w64(need_lo), needB = __builtin_amdgcn_inverse_ballot_w64(need_hi); // position `lane`, and for the low lanes position 64 + lane (need_hi has no bit from d3 on)
        uint64_t keyA, keyB;
        if (planes) { keyA = (S >> (2 * d3)) & hm; keyB = rtk_bpermute64(S & hm, 64 - d3 + lane); } // (the last h of the k + 1 characters of window 64 - d3 + lane start at 64 + lane; the lanes from d3 on ask for a lane past 63 and use nothing of what they get)
        else { int t; keyA = needA ? rtk_pack_acgt(text + bb, h, &t) : 0ull; keyB = needB ? rtk_pack_acgt(text + bb + 64, h, &t) : 0ull; }
        const uint64_t rA = rtk_revcomp(keyA, h), rB = rtk_revcomp(keyB, h), cA = keyA < rA ? keyA : rA, cB = keyB < rB ? keyB : rB;
        uint64_t iA = rtk_hash64(cA) & hx_mask, iB = rtk_hash64(cB) & hx_mask;
        uint64_t svA = needA ? hx[iA] : RTK_EMPTY_KEY, svB = needB ? hx[iB] : RTK_EMPTY_KEY; // both home slots are requested before either is waited for
        uint64_t fA = RTK_HXT_NOT_ASKED, fB = RTK_HXT_NOT_ASKED; uint32_t nA = 0, nB = 0; bool foundA = false, foundB = false;
        if (needA) { lookups += 1; fA = 0; while (true) { slots += 1; if (svA == RTK_EMPTY_KEY) break; if ((svA >> 34) == cA) { fA = svA & 0x3FFFFFFFFull; foundA = true; break; } iA = (iA + 1) & hx_mask; svA = hx[iA]; } }
        if (needB) { lookups += 1; fB = 0; while (true) { slots += 1; if (svB == RTK_EMPTY_KEY) break; if ((svB >> 34) == cB) { fB = svB & 0x3FFFFFFFFull; foundB = true; break; } iB = (iB + 1) & hx_mask; svB = hx[iB]; } }
        if (foundA) nA = static_cast<uint32_t>(hxl[fA]); // the count word is fetched here, by the look-up lane: a window starts at its list entries
        if (foundB) nB = static_cast<uint32_t>(hxl[fB]);
        rtk_sync(); // (the windows of the tile before have read the table)
        tab_first[lane] = fA; tab_cnt[lane] = nA;
        if (lane < d3) { tab_first[64 + lane] = fB; tab_cnt[64 + lane] = nB; }
        rtk_sync();
#endif
    }
    // (3) the windows. lookup_of(at, &lookups, &slots): where the window at tile position `at` gets the lists of its seeds from
    auto windows = [&](auto lookup_of) {
    for (int sub = 0; sub < n_sub; ++sub) {
#ifdef RTK_SIM
        const RtkWinCode w = win[sub]; const uint64_t wb = tile * 64 + static_cast<uint64_t>(sub); const int at = sub;
#else
        const RtkWinCode w = me; const uint64_t wb = bb; const int at = rtk_lane();
#endif
        const bool cand = w.cand; const uint64_t c_k1 = w.c_k1; const uint32_t ck = w.ck, ck1 = w.ck1;
        uint32_t kindpack = 0; int my_n = 0; bool more = false; // kinds of hit i: bits [4 i, 4 i + 3)
        // [A2] exclusive: the kinds of edit are searched one after the other and the first kind with a hit is the window's only one (rtk_a2_keep). ONE
        // visit of the window: every hit is kept with the kinds of edit that reach it, the kinds seen anywhere in the window decide which hits stay
        uint32_t keep = 7u, any = 0;
        if (cand) rtk_seeded_window(hxl, k, c_k1, ck, ck1, &slots, exclusive != 0u, lookup_of(at, &lookups, &slots), [&](uint64_t code, uint64_t hit, uint32_t kinds) {
            any |= kinds;
            for (int i = 0; i < my_n; ++i) if (RTK_ST(i, 1) == hit) { kindpack |= kinds << (4 * i); return; }
            if (my_n < RTK_SEED_REGS) { RTK_ST(my_n, 0) = code; RTK_ST(my_n, 1) = hit; kindpack |= kinds << (4 * my_n); ++my_n; } else more = true;
        });
        uint32_t live = (1u << my_n) - 1u; // the staged hits of a kept kind, in discovery order
        if (exclusive && cand) {
            keep = rtk_a2_keep(any, exclusive);
            if (!more) {
                for (int i = 0; i < RTK_SEED_REGS; ++i) if (!((kindpack >> (4 * i)) & keep)) live &= ~(1u << i);
                my_n = rtk_popc(static_cast<uint64_t>(live));
            }
        }
        *acc_probes += lookups; *acc_slots += slots; lookups = 0; slots = 0; // (the tallies of step (2) go with the lane's window)
        if (more) { // a window inside a repeat: count every visit, take a private slice of the pool, write them all. (`more` is raised by hits of ANY kind of edit -- the kinds
            // kept are only known once the whole window has been visited -- but the slice is sized from the KEPT hits alone: the pool does not grow with the exclusive reading of [A2])
            // (these two visits are not tallied; with the shared table they probe nothing either)
            uint32_t n_all = 0, l2 = 0, s2 = 0;
            rtk_seeded_window(hxl, k, c_k1, ck, ck1, &s2, exclusive, lookup_of(at, &l2, &s2), [&](uint64_t, uint64_t, uint32_t kinds) { if (kinds & keep) ++n_all; });
            const unsigned long long pb = rtk_atomic_add(bv.ipool_top, static_cast<unsigned long long>(n_all));
            if (pb + n_all <= bv.ipool_cap && n_all < (1u << 24)) {
                uint32_t w_ = 0;
                rtk_seeded_window(hxl, k, c_k1, ck, ck1, &s2, exclusive, lookup_of(at, &l2, &s2), [&](uint64_t code, uint64_t hit, uint32_t kinds) { if (!(kinds & keep)) return; bv.ipool[2 * (pb + w_)] = code; bv.ipool[2 * (pb + w_) + 1] = hit; ++w_; });
                bv.wdesc[wb] = (static_cast<uint64_t>(pb) << 24) | static_cast<uint64_t>(n_all);
                rtk_atomic_add(bv.counters + RTK_CNT_HITS_INEXACT, static_cast<unsigned long long>(n_all));
            } else rtk_atomic_add(bv.counters + RTK_CNT_OVERFLOW, 1ull);
            my_n = 0; live = 0;
        }
        static_assert(RTK_SEED_REGS < 8, "my_n is scanned as a 3-bit value");
        int total; const int off = rtk_wave_excl_scan_bits(my_n, 3, &total);
        if (total > 0) {
            const unsigned long long pbase = rtk_pool_take(bv, chunk, total);
            if (pbase + static_cast<unsigned long long>(total) <= bv.ipool_cap) {
                int w_ = 0;
                for (int i = 0; i < RTK_SEED_REGS; ++i) if ((live >> i) & 1u) { bv.ipool[2 * (pbase + off + w_)] = RTK_ST(i, 0); bv.ipool[2 * (pbase + off + w_) + 1] = RTK_ST(i, 1); ++w_; }
                if (my_n) bv.wdesc[wb] = (static_cast<uint64_t>(pbase + off) << 24) | static_cast<uint64_t>(my_n);
            } else if (rtk_lane() == 0) rtk_atomic_add(bv.counters + RTK_CNT_OVERFLOW, 1ull);
            *acc_hits += static_cast<unsigned long long>(total); // (wave-uniform: lane 0 reports it)
        }
    }
    };
    if (shared) windows([&](int at, uint32_t*, uint32_t*) { RtkHxShared s; s.tab_first = tab_first; s.tab_cnt = tab_cnt; s.at = at; s.d1 = d1; return s; });
    else windows([&](int, uint32_t* nl, uint32_t* ns) { RtkHxProbe p; p.hx = hx; p.hx_mask = hx_mask; p.hxl = hxl; p.n_lookups = nl; p.n_slots = ns; return p; });
#undef RTK_ST
}

#endif
