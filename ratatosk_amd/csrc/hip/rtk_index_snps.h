// rtk_index_snp_candidates: the graph k-mers one substitution away from every window of the searched unitigs (k_snp_*).
#ifndef RTK_INDEX_SNPS_H
#define RTK_INDEX_SNPS_H
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "rtk_index_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ SNP candidates (rtk_index_snp_candidates)
// The candidate search of the SNP annotations (detectSNPs, src/Graph.cpp:484-720; the host rule and its two sorted views: csrc/tools/index/annotate.hpp,
// NeighbourIndex) on the device. A graph k-mer ONE SUBSTITUTION away from a window shares its first k/2 bases or its last k - k/2 bases with it:
//   k_snp_keys   one lane per window of every unitig: its canonical k-mer and the unitig's id
//   view one     those pairs radix-sorted by the 2k-bit key (rocPRIM): the first half leads
//   view two     the same keys rotated so that the last k - k/2 bases lead (k_snp_rot), sorted again. Both views carry the unitig id as payload.
//   k_snp_table  in front of each view, the first entry of every value of the top min(24, 2k) key bits; on view one also the check that no key occurs twice
//   k_snp_scan   one lane per window of a SEARCHED unitig: x and rc(x) from the text, four range scans (same first half in view one, same last half in view two, for x
//                and for rc(x) with offset and base flipped back), the entries whose XOR with the query has exactly one non-zero base and that lie on another
//                unitig are candidates. Run twice: the candidates of every window counted, an exclusive scan of the counts (rocPRIM), then written to their place
//                (only the windows that have any search again). No cap: a window has at most 3k, and room is made for what was counted.
//   order        with RTK_SNP_FIRST_PER_SITE the candidates sorted by (u, p + j, alt, p) and the first of every (u, p + j, alt) kept (rocPRIM sort + select); then, always,
//                the candidates sorted by their two words (u << 32 | p, j << 40 | alt << 32 | w) as one 128-bit key: the order of the host rule's visits.
// Bounds: a window index below the number of windows counted on the host from seq_off; a window of unitig u starts at most k bases before seq_off[u + 1]; table indices
// are key >> shift <= 2^bits - 1 (+ 1 for the end of a range: the tables hold 2^bits + 1 entries); a candidate is written below the total that the count pass gave.
//
// When the views of all N windows do not fit the device (or RTK_INDEX_SNP_PASSES says so) the search runs in P passes over PARTITIONS of the key space. A partition is a
// range [lo, hi) of the prefix value key >> shift that the tables use; view one is cut by the prefix of the canonical key, view two by the prefix of the rotated key, each
// by its own P + 1 boundaries. The boundaries are balanced on the host from two histograms of the prefixes over all windows (k_snp_hist; they lie in the tables' memory,
// which is not in use yet): boundary i is the first prefix with i N / P keys below it, so a partition holds at most N / P keys plus those of one prefix, or none.
//   k_snp_keys_part  one lane per window of every unitig, every pass: the canonical key is appended to view one when its prefix lies in the pass's range, its rotation to
//                    view two when that one's does (one atomic per wave and view; the order does not matter: the keys are distinct and sorted next)
//   k_snp_table      over the prefixes lo .. hi of the partition only: T[v - lo]
//   k_snp_scan<PART> as above, against the partial views: a prefix is clamped to lo .. hi before the table is read. A query range below the partition then is
//                    T[0] .. T[0], one above it T[hi - lo] .. T[hi - lo] (= n .. n): empty; one that straddles a boundary is cut to the entries the view has.
// Count, exclusive scan and write run per pass; the candidates of a pass go to the host, and all of them are ordered once after the last pass has released its views
// (a candidate is an entry of one view and so of one partition: the union over the passes is the set of the single pass). The checks hold per pass: equal keys have
// equal prefixes and meet in one partition. One pass (P = 1) is the path without any of this: k_snp_keys, k_snp_rot, whole tables, k_snp_scan<false>.
// Bounds of a pass: the histograms are indexed by key >> shift < 2^bits; a key is appended below the cursor's cap = the partition's count from the histogram (the host
// compares both cursors with the counts before it sorts); the table of a partition has hi - lo + 1 <= 2^bits + 1 entries and is indexed by a value clamped to lo .. hi,
// less lo; its values are <= n, the pass's count of that view, so every entry read lies below n.
// the entry of a list of unitigs that holds window g: woff[s] = the windows before entry s (n_s + 1 values, woff[0] = 0 <= g < woff[n_s]); the last s with woff[s] <= g
__device__ __forceinline__ uint64_t snp_locate(const uint64_t* __restrict__ woff, uint64_t n_s, uint64_t g) {
    uint64_t lo = 0, hi = n_s;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (woff[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
template <class KM> __device__ __forceinline__ KM snp_window(const char* __restrict__ pool, uint64_t at, int k, bool* bad) {
    KM x = 0;
    for (int q = 0; q < k; ++q) { const uint32_t c = idx_code(static_cast<unsigned char>(pool[at + q])); if (c > 3u) *bad = true; x = (x << 2) | static_cast<KM>(c & 3u); }
    return x;
}
__device__ __forceinline__ int snp_ctz(uint64_t m) { return __ffsll(static_cast<unsigned long long>(m)) - 1; }
__device__ __forceinline__ int snp_ctz(km2_t m) { const uint64_t lo = static_cast<uint64_t>(m); return lo ? __ffsll(static_cast<unsigned long long>(lo)) - 1 : 63 + __ffsll(static_cast<unsigned long long>(static_cast<uint64_t>(m >> 64))); }

template <class KM>
__global__ void k_snp_keys(const char* __restrict__ pool, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ woff, uint64_t n_u, uint64_t n_win, int k,
                           KM* __restrict__ keys, uint32_t* __restrict__ ids, uint32_t* __restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < n_win; g += stride) {
        const uint64_t u = snp_locate(woff, n_u, g); bool bad = false;
        const KM x = snp_window<KM>(pool, seq_off[u] + (g - woff[u]), k, &bad), rc = idx_revcomp(x, k);
        keys[g] = x <= rc ? x : rc; ids[g] = static_cast<uint32_t>(u);
        if (bad) atomicOr(flag, 1u); // a character that is no base
    }
}
template <class KM> __global__ void k_snp_rot(const KM* __restrict__ a, const uint32_t* __restrict__ ia, uint64_t n, int k, KM* __restrict__ b, uint32_t* __restrict__ ib) {
    const int hi_n = k / 2, lo_n = k - hi_n; const KM lomask = (static_cast<KM>(1) << (2 * lo_n)) - static_cast<KM>(1);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) { const KM x = a[i]; b[i] = ((x & lomask) << (2 * hi_n)) | (x >> (2 * lo_n)); ib[i] = ia[i]; }
}
// the prefix values [a_lo, a_hi) of view one and [b_lo, b_hi) of view two that a pass holds (one pass: 0 and 2^bits)
struct SnpRange { uint64_t a_lo, a_hi, b_lo, b_hi; };
// the key of view two: the last k - k/2 bases lead
template <class KM> __device__ __forceinline__ KM snp_rotated(KM x, int k) { const int hi_n = k / 2, lo_n = k - hi_n; return ((x & ((static_cast<KM>(1) << (2 * lo_n)) - static_cast<KM>(1))) << (2 * hi_n)) | (x >> (2 * lo_n)); }
// One lane per window of every unitig: the prefixes of its canonical key and of the rotated key counted (ha, hb: 2^bits counters each; a key is below 2^(2k), its
// prefix key >> shift below 2^bits).
template <class KM>
__global__ void k_snp_hist(const char* __restrict__ pool, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ woff, uint64_t n_u, uint64_t n_win, int k, int shift,
                           unsigned long long* __restrict__ ha, unsigned long long* __restrict__ hb, uint32_t* __restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < n_win; g += stride) {
        const uint64_t u = snp_locate(woff, n_u, g); bool bad = false;
        const KM x = snp_window<KM>(pool, seq_off[u] + (g - woff[u]), k, &bad), rc = idx_revcomp(x, k), can = x <= rc ? x : rc;
        atomicAdd(ha + static_cast<uint64_t>(can >> shift), 1ull); atomicAdd(hb + static_cast<uint64_t>(snp_rotated(can, k) >> shift), 1ull);
        if (bad) atomicOr(flag, 1u); // a character that is no base
    }
}
// n lanes of a wave append one item each (all lanes of the wave call it): the place of this lane's item, from one atomic per wave
__device__ __forceinline__ uint64_t snp_append(bool mine, unsigned long long* __restrict__ cursor) {
    const uint64_t bal = __ballot(mine ? 1 : 0);
    if (!bal) return 0;
    const int lane = threadIdx.x & 63, first = __ffsll(static_cast<unsigned long long>(bal)) - 1;
    unsigned long long base = 0;
    if (lane == first) base = atomicAdd(cursor, static_cast<unsigned long long>(__popcll(bal)));
    base = __shfl(base, first, 64);
    return base + static_cast<uint64_t>(__popcll(bal & ((1ull << lane) - 1ull)));
}
// One lane per window of every unitig: the (key, id) pairs of one pass. The canonical key goes to view one when its prefix lies in [R.a_lo, R.a_hi), the rotated key to
// view two when its prefix lies in [R.b_lo, R.b_hi): appended at cursor[0] / cursor[1], below cap_a / cap_b (the partitions' counts from k_snp_hist).
template <class KM>
__global__ void k_snp_keys_part(const char* __restrict__ pool, const uint64_t* __restrict__ seq_off, const uint64_t* __restrict__ woff, uint64_t n_u, uint64_t n_win, int k, int shift, SnpRange R,
                                KM* __restrict__ ka, uint32_t* __restrict__ ia, uint64_t cap_a, KM* __restrict__ kb, uint32_t* __restrict__ ib, uint64_t cap_b,
                                unsigned long long* __restrict__ cursor, uint32_t* __restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; g0 < n_win; g0 += stride) { // (the same trips for every lane of a wave: the ballots)
        const uint64_t g = g0 + threadIdx.x; const bool live = g < n_win;
        KM can = 0, rot = 0; uint32_t u32 = 0; bool bad = false;
        if (live) {
            const uint64_t u = snp_locate(woff, n_u, g);
            const KM x = snp_window<KM>(pool, seq_off[u] + (g - woff[u]), k, &bad), rc = idx_revcomp(x, k);
            can = x <= rc ? x : rc; rot = snp_rotated(can, k); u32 = static_cast<uint32_t>(u);
        }
        const uint64_t pa = static_cast<uint64_t>(can >> shift), pb = static_cast<uint64_t>(rot >> shift);
        const bool in_a = live && pa >= R.a_lo && pa < R.a_hi, in_b = live && pb >= R.b_lo && pb < R.b_hi;
        const uint64_t at_a = snp_append(in_a, cursor), at_b = snp_append(in_b, cursor + 1);
        if (in_a && at_a < cap_a) { ka[at_a] = can; ia[at_a] = u32; }
        if (in_b && at_b < cap_b) { kb[at_b] = rot; ib[at_b] = u32; }
        if (bad) atomicOr(flag, 1u); // a character that is no base
    }
}
// T[v - base] = the first entry whose top bits (key >> shift) are >= v, for v in base .. top (the keys' top bits lie in base .. top - 1: T[top - base] = n; all keys:
// base = 0, top = n_pref = 2^bits). Lane i fills the values between the top bits of entries i - 1 and i, so every T[v - base] is written once. flag != nullptr: bit 1
// set when two neighbouring keys are equal.
template <class KM> __global__ void k_snp_table(const KM* __restrict__ keys, uint64_t n, int shift, uint64_t base, uint64_t top, uint64_t* __restrict__ T, uint32_t* __restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride) {
        const uint64_t a = i == 0 ? base : static_cast<uint64_t>(keys[i - 1] >> shift) + 1, b = i == n ? top : static_cast<uint64_t>(keys[i] >> shift);
        for (uint64_t v = a < base ? base : a; v <= b && v <= top; ++v) T[v - base] = i;
        if (flag && i != 0 && i < n && keys[i] == keys[i - 1]) atomicOr(flag, 2u);
    }
}

template <class KM> struct SnpViews { const KM* a; const uint32_t* ia; const uint64_t* ta; const KM* b; const uint32_t* ib; const uint64_t* tb; int k, shift; SnpRange r; };
// T[v] of a whole table, or of a partition's: v clamped to lo .. hi, the table starts at lo
template <bool PART> __device__ __forceinline__ uint64_t snp_first(const uint64_t* __restrict__ T, uint64_t v, uint64_t lo, uint64_t hi) {
    if (!PART) return T[v];
    return T[(v < lo ? lo : (v > hi ? hi : v)) - lo];
}
// The graph k-mers one substitution away from x (NeighbourIndex::scan): as (offset, base) of the ORIENTED neighbour of the window (flipped: x is the window's reverse
// complement). Those on the window's own unitig u are dropped. out == nullptr: counted only; else candidate number c goes to out[2 (at + c)], below `end`. Returns the count.
// PART: the views hold the partitions V.r only (their tables too); a range is cut to what the views hold.
template <class KM, bool PART>
__device__ __forceinline__ uint32_t snp_scan(const SnpViews<KM>& V, KM x, bool flipped, uint32_t u, uint64_t word0, uint64_t* __restrict__ out, uint64_t at, uint64_t end) {
    const int k = V.k, hi_n = k / 2, lo_n = k - hi_n;
    const KM one = 1, lomask = (one << (2 * lo_n)) - one, himask = (one << (2 * hi_n)) - one, m55 = ~static_cast<KM>(0) / static_cast<KM>(3); // 0101...01
    uint32_t c = 0;
    auto entry = [&](KM y, uint32_t w) { // y: a canonical k-mer of unitig w
        const KM d = y ^ x; if (d == 0 || w == u) return;
        const KM m = (d | (d >> 1)) & m55; if (m & (m - one)) return; // more than one base differs
        const int bit = snp_ctz(m); uint32_t j = static_cast<uint32_t>(k - 1 - bit / 2), base = static_cast<uint32_t>(y >> bit) & 3u;
        if (flipped) { j = static_cast<uint32_t>(k - 1) - j; base = 3u - base; }
        if (out && at + c < end) { out[2 * (at + c)] = word0; out[2 * (at + c) + 1] = (static_cast<uint64_t>(j) << 40) | (static_cast<uint64_t>(base) << 32) | w; }
        ++c;
    };
    { // same first half: the differing base lies in the last lo_n bases
        const KM lo_key = x & ~lomask, hi_key = x | lomask;
        uint64_t i = snp_first<PART>(V.ta, static_cast<uint64_t>(lo_key >> V.shift), V.r.a_lo, V.r.a_hi); const uint64_t e = snp_first<PART>(V.ta, static_cast<uint64_t>(hi_key >> V.shift) + 1, V.r.a_lo, V.r.a_hi);
        { uint64_t hi = e; while (i < hi) { const uint64_t mid = i + (hi - i) / 2; if (V.a[mid] < lo_key) i = mid + 1; else hi = mid; } }
        for (; i < e; ++i) { const KM y = V.a[i]; if (y > hi_key) break; entry(y, V.ia[i]); }
    }
    { // same last half: the differing base lies in the first hi_n bases
        const KM r = ((x & lomask) << (2 * hi_n)) | (x >> (2 * lo_n)), lo_key = r & ~himask, hi_key = r | himask;
        uint64_t i = snp_first<PART>(V.tb, static_cast<uint64_t>(lo_key >> V.shift), V.r.b_lo, V.r.b_hi); const uint64_t e = snp_first<PART>(V.tb, static_cast<uint64_t>(hi_key >> V.shift) + 1, V.r.b_lo, V.r.b_hi);
        { uint64_t hi = e; while (i < hi) { const uint64_t mid = i + (hi - i) / 2; if (V.b[mid] < lo_key) i = mid + 1; else hi = mid; } }
        for (; i < e; ++i) { const KM y = V.b[i]; if (y > hi_key) break; entry(((y & himask) << (2 * lo_n)) | (y >> (2 * hi_n)), V.ib[i]); }
    }
    return c;
}
// list[s] = the s-th searched unitig, woff[s] = the windows of the searched unitigs before it. Count pass (out == nullptr): counts[g] = the candidates of window g.
// Write pass: the candidates of window g at offs[g] .. offs[g + 1], in the order the scans find them.
template <class KM, bool PART>
__global__ void k_snp_scan(const char* __restrict__ pool, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ list, const uint64_t* __restrict__ woff, uint64_t n_s, uint64_t n_win,
                           SnpViews<KM> V, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offs, uint64_t* __restrict__ out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < n_win; g += stride) {
        uint64_t at = 0, end = 0;
        if (out) { at = offs[g]; end = offs[g + 1]; if (at == end) continue; }
        const uint64_t s = snp_locate(woff, n_s, g), p = g - woff[s]; const uint32_t u = list[s]; bool bad = false;
        const KM x = snp_window<KM>(pool, seq_off[u] + p, V.k, &bad), rc = idx_revcomp(x, V.k);
        const uint64_t word0 = (static_cast<uint64_t>(u) << 32) | p;
        const uint32_t c = snp_scan<KM, PART>(V, x, false, u, word0, out, at, end);
        const uint32_t c2 = snp_scan<KM, PART>(V, rc, true, u, word0, out, at + c, end);
        if (!out) counts[g] = c + c2;
    }
}
struct SnpCountAt { const uint32_t* c; uint64_t n; __device__ uint64_t operator()(uint64_t i) const { return i < n ? static_cast<uint64_t>(c[i]) : 0ull; } };
// candidates (two words each) -> keys (u, p + j, alt, p) with the unitig w beside them
__global__ void k_snp_site_keys(const uint64_t* __restrict__ cand, uint64_t n, km2_t* __restrict__ keys, uint32_t* __restrict__ w) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t w0 = cand[2 * i], w1 = cand[2 * i + 1], p = w0 & 0xFFFFFFFFull, j = w1 >> 40, alt = (w1 >> 32) & 3ull;
        keys[i] = (static_cast<km2_t>(w0 >> 32) << 66) | (static_cast<km2_t>(p + j) << 34) | (static_cast<km2_t>(alt) << 32) | static_cast<km2_t>(p);
        w[i] = static_cast<uint32_t>(w1);
    }
}
struct SnpSiteHead { const km2_t* keys; __device__ bool operator()(uint64_t i) const { return i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32); } };
// the order keys word0 << 64 | word1: of the kept site keys sel[0 .. n) (sel != nullptr), or of the candidates as they stand
__global__ void k_snp_order_keys(const uint64_t* __restrict__ cand, const km2_t* __restrict__ site, const uint32_t* __restrict__ w, const uint64_t* __restrict__ sel, uint64_t n, km2_t* __restrict__ keys) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        uint64_t w0, w1;
        if (sel) {
            const uint64_t i = sel[r]; const km2_t sk = site[i];
            const uint64_t u = static_cast<uint64_t>(sk >> 66), s = static_cast<uint64_t>(sk >> 34) & 0xFFFFFFFFull, alt = static_cast<uint64_t>(sk >> 32) & 3ull, p = static_cast<uint64_t>(sk) & 0xFFFFFFFFull;
            w0 = (u << 32) | p; w1 = ((s - p) << 40) | (alt << 32) | w[i];
        } else { w0 = cand[2 * r]; w1 = cand[2 * r + 1]; }
        keys[r] = (static_cast<km2_t>(w0) << 64) | static_cast<km2_t>(w1);
    }
}

// A stage's device buffers as one list of (name, bytes): the memory the stage asks for is the sum over the list, and a buffer is allocated with the size the list
// gives it, so the two cannot drift apart.
template <int N> struct DevPlan {
    struct Item { const char* name; uint64_t bytes; };
    Item item[N]; DevArr<char> buf[N];
    DevPlan() { for (int i = 0; i < N; ++i) item[i] = Item{"", 0}; }
    DevPlan(std::initializer_list<Item> l) { int i = 0; for (const Item& it : l) if (i < N) item[i++] = it; for (; i < N; ++i) item[i] = Item{"", 0}; }
    uint64_t bytes() const { uint64_t s = 0; for (int i = 0; i < N; ++i) s += item[i].bytes; return s; }
    template <class T> T* alloc(int i) { buf[i].alloc(item[i].bytes); return reinterpret_cast<T*>(buf[i].p); }
    void release(int i) { buf[i].release(); }
};
enum { SNP_POOL, SNP_OFF, SNP_WOFF, SNP_K0, SNP_K1, SNP_K2, SNP_V0, SNP_V1, SNP_V2, SNP_TMP, SNP_TA, SNP_TB, SNP_LIST, SNP_SWOFF, SNP_CNT, SNP_OFFS, SNP_BUFS };
enum { SNPC_CAND, SNPC_S0, SNPC_S1, SNPC_W0, SNPC_W1, SNPC_SEL, SNPC_O0, SNPC_O1, SNPC_BUFS };
#define RTK_SNP_SLACK 4096ull          // on top of the views' list: the flag word, the granularity of the allocations
#define RTK_SNP_CAND_SLACK (64ull << 20) // on top of the candidates' list: the temporaries of its sorts and selection

// what is to be had: the free device memory, or RTK_INDEX_SNP_MEM; room for `need` bytes?
inline uint64_t snp_room() { size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo"); return rtk_knob_index_snp_mem(static_cast<uint64_t>(fr)); }
inline bool snp_room(uint64_t need, uint64_t* room) { *room = snp_room(); return need <= *room; }

// the windows of every unitig (the views: woff) and of the searched ones (the queries: list, swoff)
struct SnpWindows { std::vector<uint64_t> woff, swoff; std::vector<uint32_t> list; uint64_t N = 0, n_s = 0, W = 0; };
inline int snp_windows(int k, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, SnpWindows* w) {
    w->woff.assign(n_unitigs + 1, 0); w->swoff.assign(1, 0);
    for (uint64_t u = 0; u < n_unitigs; ++u) {
        if (seq_off[u + 1] < seq_off[u] + static_cast<uint64_t>(k)) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a unitig of fewer than k characters");
        const uint64_t nw = seq_off[u + 1] - seq_off[u] - static_cast<uint64_t>(k) + 1;
        if (nw + static_cast<uint64_t>(k) > (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_candidates: a unitig of 2^32 characters or more");
        w->woff[u + 1] = w->woff[u] + nw;
        if (!searched || searched[u]) { w->list.push_back(static_cast<uint32_t>(u)); w->swoff.push_back(w->swoff.back() + nw); }
    }
    w->N = w->woff[n_unitigs]; w->n_s = w->list.size(); w->W = w->swoff.back();
    return RTK_OK;
}

// The two rocPRIM primitives of the views, each spelt once: sized on null buffers for the plan, run on the real ones.
template <class KM> auto snp_sort_view(rocprim::double_buffer<KM>& keys, rocprim::double_buffer<uint32_t>& ids, uint64_t n, int k) {
    return [&keys, &ids, n, k](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keys, ids, n, 0, 2 * k); };
}
inline auto snp_scan_counts(const uint32_t* counts, uint64_t* offs, uint64_t W) {
    return [counts, offs, W](void* t, size_t& b) {
        SnpCountAt at; at.c = counts; at.n = W;
        auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), at);
        return rocprim::exclusive_scan(t, b, it, offs, 0ull, W + 1, rocprim::plus<uint64_t>());
    };
}
// What the stage is asked: k, the text, the windows.
struct SnpShape { int k; uint64_t n_bases, n_unitigs, N, n_s, W; };
inline int snp_bits(int k) { return 2 * k < 24 ? 2 * k : 24; }
#define RTK_SNP_MAX_PASSES 256ull
inline uint32_t snp_max_passes(int k) { return static_cast<uint32_t>(std::min<uint64_t>(RTK_SNP_MAX_PASSES, 1ull << snp_bits(k))); } // (a partition is at least one prefix value)
// What the stage needs with views of at most M keys each (one pass: M = N), before anything is allocated: text and offsets, three arrays of (key, id) -- two views and the
// sorts' other buffer --, the primitives' temporary, two prefix tables (the histograms of the prefixes lie in them first), the searched unitigs, the counts and their
// running sums. The candidates come on top once they are counted (checked again there).
template <class KM> void snp_plan_fill(const SnpShape& s, uint64_t M, DevPlan<SNP_BUFS>& plan) {
    rocprim::double_buffer<KM> no_keys(nullptr, nullptr); rocprim::double_buffer<uint32_t> no_ids(nullptr, nullptr);
    const size_t tb_sort = prim_bytes("rocprim::radix_sort_pairs (size)", snp_sort_view(no_keys, no_ids, M, s.k)), tb_scan = prim_bytes("rocprim::exclusive_scan (size)", snp_scan_counts(nullptr, nullptr, s.W));
    const uint64_t n_pref = 1ull << snp_bits(s.k);
    const typename DevPlan<SNP_BUFS>::Item items[SNP_BUFS] = {{"unitig text", s.n_bases}, {"unitig offsets", 8 * (s.n_unitigs + 1)}, {"window offsets", 8 * (s.n_unitigs + 1)},
        {"keys 0", sizeof(KM) * M}, {"keys 1", sizeof(KM) * M}, {"keys 2", sizeof(KM) * M}, {"ids 0", 4 * M}, {"ids 1", 4 * M}, {"ids 2", 4 * M},
        {"temporary", std::max<uint64_t>(tb_sort, tb_scan)}, {"prefix table one", 8 * (n_pref + 1)}, {"prefix table two", 8 * (n_pref + 1)},
        {"searched unitigs", 4 * s.n_s}, {"searched window offsets", 8 * (s.n_s + 1)}, {"counts", 4 * s.W}, {"candidate offsets", 8 * (s.W + 1)}};
    for (int i = 0; i < SNP_BUFS; ++i) plan.item[i] = items[i];
}
template <class KM> uint64_t snp_need(const SnpShape& s, uint64_t M) { DevPlan<SNP_BUFS> plan; snp_plan_fill<KM>(s, M, plan); return plan.bytes() + RTK_SNP_SLACK; }
// The number of passes for `room` bytes: the smallest P whose plan fits when every partition holds its even share ceil(N / P) of the keys -- what can be said before the
// keys are seen; the stage takes more passes when the histograms show a heavier partition. forced != 0 (RTK_INDEX_SNP_PASSES): that many and no other.
// passes == 0: nothing fits, and `need` is the smallest plan (that of `forced` passes, when forced).
struct SnpChoice { uint32_t passes; uint64_t need, need_one, need_min; };
template <class KM> SnpChoice snp_choose(const SnpShape& s, uint64_t room, uint32_t forced) {
    const uint32_t p_max = snp_max_passes(s.k), first = forced ? std::min(forced, p_max) : 1u, last = forced ? first : p_max;
    auto share = [&](uint32_t P) { return (s.N + P - 1) / P; };
    SnpChoice c; c.passes = 0; c.need_one = snp_need<KM>(s, s.N); c.need_min = snp_need<KM>(s, share(p_max)); c.need = forced ? snp_need<KM>(s, share(first)) : c.need_min;
    for (uint32_t P = first; P <= last; ++P) {
        const uint64_t need = snp_need<KM>(s, share(P));
        if (need <= room) { c.passes = P; c.need = need; break; }
    }
    return c;
}
// P partitions of a view from its histogram summed up (below[v] = the keys whose prefix is under v, for v in 0 .. n_pref): bound[i] = the first prefix with i N / P keys
// below it (bound[0] = 0, bound[P] = n_pref), so that partition i = [bound[i], bound[i + 1]) holds about N / P keys, or none. Returns the keys of the largest.
inline uint64_t snp_bounds(const std::vector<uint64_t>& below, uint64_t N, uint32_t P, std::vector<uint64_t>* bound) {
    const uint64_t n_pref = below.size() - 1; uint64_t largest = 0;
    bound->assign(P + 1, n_pref); (*bound)[0] = 0;
    for (uint32_t i = 1; i < P; ++i) (*bound)[i] = static_cast<uint64_t>(std::lower_bound(below.begin(), below.end(), i * N / P) - below.begin()); // (i <= 256: no overflow below 2^56 keys)
    for (uint32_t i = 0; i < P; ++i) largest = std::max(largest, below[(*bound)[i + 1]] - below[(*bound)[i]]);
    return largest;
}

// The C candidates at `raw` (two words each) in the order of the host rule's visits, first_per_site: only the first of every (u, p + j, alt). They are left as
// 128-bit keys word0 << 64 | word1 in plan buffer SNPC_O0 or SNPC_O1: *keys. Returns how many are kept, or a count above C: more kept than found.
inline uint64_t snp_order(DevPlan<SNPC_BUFS>& plan, const uint64_t* raw, uint64_t C, bool first_per_site, const km2_t** keys) {
    uint64_t R = C; DevArr<char> tmp;
    const km2_t* site = nullptr; const uint32_t* site_w = nullptr; const uint64_t* sel = nullptr;
    if (first_per_site) {
        rocprim::double_buffer<km2_t> sk(plan.alloc<km2_t>(SNPC_S0), plan.alloc<km2_t>(SNPC_S1)); rocprim::double_buffer<uint32_t> sw(plan.alloc<uint32_t>(SNPC_W0), plan.alloc<uint32_t>(SNPC_W1));
        uint64_t* kept = plan.alloc<uint64_t>(SNPC_SEL); DevArr<unsigned long long> n_kept; n_kept.alloc(1);
        launch("k_snp_site_keys", k_snp_site_keys, idx_grid(C, 2048), 0, raw, C, sk.current(), sw.current());
        prim(tmp, "rocprim::radix_sort_pairs", [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, sk, sw, C, 0, 98); });
        SnpSiteHead head; head.keys = sk.current();
        auto idx = rocprim::make_counting_iterator<uint64_t>(0); auto heads = rocprim::make_transform_iterator(idx, head);
        prim(tmp, "rocprim::select", [&](void* t, size_t& b) { return rocprim::select(t, b, idx, heads, kept, n_kept.p, C); });
        R = read_word(n_kept.p, "first candidate of every site");
        if (R > C) return R;
        site = sk.current(); site_w = sw.current(); sel = kept;
    }
    plan.item[SNPC_O0].bytes = plan.item[SNPC_O1].bytes = 16 * R; // (asked for at 16 C each: R <= C)
    rocprim::double_buffer<km2_t> ok(plan.alloc<km2_t>(SNPC_O0), plan.alloc<km2_t>(SNPC_O1));
    launch("k_snp_order_keys", k_snp_order_keys, idx_grid(R, 2048), 0, raw, site, site_w, sel, R, ok.current());
    if (first_per_site) { rtk_check(hipDeviceSynchronize(), "k_snp_order_keys"); for (int i = SNPC_S0; i <= SNPC_SEL; ++i) plan.release(i); } // (the site keys have served)
    prim(tmp, "rocprim::radix_sort_keys", [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, ok, R, 0, 128); });
    rtk_check(hipDeviceSynchronize(), "candidates ordered");
    *keys = ok.current();
    return R;
}

template <class KM>
int snp_candidates(int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint32_t flags, uint64_t** cand_out, uint64_t* n_cand) {
    const StageClock clk;
    SnpWindows win;
    if (const int rc = snp_windows(k, seq_off, n_unitigs, searched, &win)) return rc;
    const uint64_t n_bases = seq_off[n_unitigs], N = win.N, n_s = win.n_s, W = win.W;
    if (N == 0 || W == 0) { // nothing to find, or nobody asks
        if (clk.trace) fprintf(stderr, "rtk_index_snps: %llu windows of %llu unitigs searched against %llu k-mers, 0 candidates (0 kept); views 0.00 s, scan 0.00 s\n", static_cast<unsigned long long>(W), static_cast<unsigned long long>(n_s), static_cast<unsigned long long>(N));
        return RTK_OK;
    }
    const SnpShape shape = {k, n_bases, n_unitigs, N, n_s, W};
    const int bits = snp_bits(k), shift = 2 * k - bits; const uint64_t n_pref = 1ull << bits, room = snp_room();
    const uint32_t forced = rtk_knob_index_snp_passes();
    const SnpChoice choice = snp_choose<KM>(shape, room, forced);
    auto refusal = [&](uint64_t need, uint32_t passes) {
        return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: the two views of " + std::to_string(N) + " k-mers need " + std::to_string(need) + " bytes of device memory, " + std::to_string(room) + " are to be had (in " + std::to_string(passes) + " passes over the key space)");
    };
    if (!choice.passes) return refusal(choice.need, forced ? std::min(forced, snp_max_passes(k)) : snp_max_passes(k));
    uint32_t P = choice.passes;
    DevPlan<SNP_BUFS> plan; snp_plan_fill<KM>(shape, (N + P - 1) / P, plan);

    // what every pass reads: the text and the windows, the flag word, the tables' memory
    const char* pool = plan.alloc<char>(SNP_POOL); const uint64_t* off = plan.alloc<uint64_t>(SNP_OFF); const uint64_t* d_woff = plan.alloc<uint64_t>(SNP_WOFF);
    DevArr<uint32_t> flag; flag.alloc(2);
    uint64_t* ta = plan.alloc<uint64_t>(SNP_TA); uint64_t* tb = plan.alloc<uint64_t>(SNP_TB);
    rtk_check(hipMemcpy(plan.buf[SNP_POOL].p, seq_pool, n_bases, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemcpy(plan.buf[SNP_OFF].p, seq_off, 8 * (n_unitigs + 1), hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemcpy(plan.buf[SNP_WOFF].p, win.woff.data(), 8 * (n_unitigs + 1), hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemset(flag.p, 0, 8), "hipMemset");
    auto flag_errors = [&](const char* synced) {
        const uint32_t fl = read_word(flag.p, synced);
        if (fl & 1u) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a unitig holds a character that is no base");
        if (fl & 2u) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a k-mer occurs twice in the unitigs");
        return RTK_OK;
    };

    // More than one pass: the partitions of either view from the histograms of the prefixes, and the plan with the largest of them -- more passes when that does not fit
    std::vector<uint64_t> bound_a(2, n_pref), bound_b(2, n_pref), below_a, below_b; bound_a[0] = bound_b[0] = 0;
    uint64_t largest = N; DevArr<unsigned long long> cursor;
    if (P > 1) {
        rtk_check(hipMemset(ta, 0, 8 * n_pref), "hipMemset"); rtk_check(hipMemset(tb, 0, 8 * n_pref), "hipMemset");
        launch("k_snp_hist", k_snp_hist<KM>, idx_grid(N, 2048), 0, pool, off, d_woff, n_unitigs, N, k, shift, reinterpret_cast<unsigned long long*>(ta), reinterpret_cast<unsigned long long*>(tb), flag.p);
        if (const int rc = flag_errors("prefixes of the k-mers counted")) return rc;
        for (int v = 0; v < 2; ++v) { // counts -> the keys below every prefix
            std::vector<uint64_t>& below = v ? below_b : below_a;
            below.assign(n_pref + 1, 0);
            rtk_check(hipMemcpy(below.data() + 1, v ? tb : ta, 8 * n_pref, hipMemcpyDeviceToHost), "hipMemcpy");
            for (uint64_t i = 1; i <= n_pref; ++i) below[i] += below[i - 1];
            if (below[n_pref] != N) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: the prefixes counted are not the windows");
        }
        for (;; ++P) {
            largest = std::max(snp_bounds(below_a, N, P, &bound_a), snp_bounds(below_b, N, P, &bound_b));
            snp_plan_fill<KM>(shape, largest, plan);
            if (plan.bytes() + RTK_SNP_SLACK <= room) break;
            if (forced || P == snp_max_passes(k)) return refusal(plan.bytes() + RTK_SNP_SLACK, P);
        }
        cursor.alloc(2);
    }
    KM* d_k[3]; uint32_t* d_v[3];
    for (int i = 0; i < 3; ++i) { d_k[i] = plan.alloc<KM>(SNP_K0 + i); d_v[i] = plan.alloc<uint32_t>(SNP_V0 + i); }
    void* tmp = plan.alloc<char>(SNP_TMP); const size_t tmp_bytes = plan.item[SNP_TMP].bytes;
    uint32_t* list = plan.alloc<uint32_t>(SNP_LIST); uint64_t* swoff = plan.alloc<uint64_t>(SNP_SWOFF); uint32_t* counts = plan.alloc<uint32_t>(SNP_CNT); uint64_t* offs = plan.alloc<uint64_t>(SNP_OFFS);
    rtk_check(hipMemcpy(list, win.list.data(), 4 * n_s, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemcpy(swoff, win.swoff.data(), 8 * (n_s + 1), hipMemcpyHostToDevice), "hipMemcpy");
    // a view of n <= `largest` keys sorted: in the plan's temporary, which was sized for `largest` keys (should fewer keys ever ask for more: in one of its own)
    auto sort_view = [&](rocprim::double_buffer<KM>& keys, rocprim::double_buffer<uint32_t>& ids, uint64_t n) {
        const size_t bytes = prim_bytes("rocprim::radix_sort_pairs (size)", snp_sort_view(keys, ids, n, k));
        if (bytes <= tmp_bytes) { prim(tmp, tmp_bytes, "rocprim::radix_sort_pairs", snp_sort_view(keys, ids, n, k)); return; }
        DevArr<char> own; prim(own, "rocprim::radix_sort_pairs", snp_sort_view(keys, ids, n, k)); rtk_check(hipDeviceSynchronize(), "rocprim::radix_sort_pairs");
    };

    SnpViews<KM> V; V.ta = ta; V.tb = tb; V.k = k; V.shift = shift;
    std::vector<uint64_t> gathered; // the candidates of the passes so far (P > 1)
    uint64_t C = 0; double t_scan = 0; // (the seconds between a pass's views and its end)
    for (uint32_t pass = 0; pass < P; ++pass) {
        V.r.a_lo = bound_a[pass]; V.r.a_hi = bound_a[pass + 1]; V.r.b_lo = bound_b[pass]; V.r.b_hi = bound_b[pass + 1];
        uint64_t n_a = N, n_b = N;
        rocprim::double_buffer<KM> k1(d_k[0], d_k[1]); rocprim::double_buffer<uint32_t> v1(d_v[0], d_v[1]);
        if (P == 1) { // the keys of all windows; view one: (keys 0, keys 1) sorted; view two: its rotated copy in keys 2 sorted with the buffer view one left free
            launch("k_snp_keys", k_snp_keys<KM>, idx_grid(N, 2048), 0, pool, off, d_woff, n_unitigs, N, k, d_k[0], d_v[0], flag.p);
            sort_view(k1, v1, N);
            launch("k_snp_rot", k_snp_rot<KM>, idx_grid(N, 2048), 0, k1.current(), v1.current(), N, k, d_k[2], d_v[2]);
        } else { // the keys of this pass's partitions: view one into keys 0, view two into keys 2
            n_a = below_a[V.r.a_hi] - below_a[V.r.a_lo]; n_b = below_b[V.r.b_hi] - below_b[V.r.b_lo];
            if (n_a == 0 && n_b == 0) continue; // (nothing to be found in empty views)
            rtk_check(hipMemset(cursor.p, 0, 16), "hipMemset");
            launch("k_snp_keys_part", k_snp_keys_part<KM>, idx_grid(N, 2048), 0, pool, off, d_woff, n_unitigs, N, k, shift, V.r, d_k[0], d_v[0], n_a, d_k[2], d_v[2], n_b, cursor.p, flag.p);
            unsigned long long got[2] = {0, 0};
            rtk_check(hipDeviceSynchronize(), "k_snp_keys_part"); rtk_check(hipMemcpy(got, cursor.p, 16, hipMemcpyDeviceToHost), "hipMemcpy");
            if (got[0] != n_a || got[1] != n_b) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: a partition does not hold the keys that were counted for it");
            if (n_a) sort_view(k1, v1, n_a);
        }
        rocprim::double_buffer<KM> k2(d_k[2], k1.alternate()); rocprim::double_buffer<uint32_t> v2(d_v[2], v1.alternate());
        if (n_b) sort_view(k2, v2, n_b);
        launch("k_snp_table", k_snp_table<KM>, idx_grid(n_a + 1, 2048), 0, k1.current(), n_a, shift, V.r.a_lo, V.r.a_hi, ta, flag.p);
        launch("k_snp_table", k_snp_table<KM>, idx_grid(n_b + 1, 2048), 0, k2.current(), n_b, shift, V.r.b_lo, V.r.b_hi, tb, nullptr);
        if (const int rc = flag_errors("views of the k-mers")) return rc;
        const double t_viewed = clk.since();
        if (P == 1) { // the buffer neither view ended up in is free again
            for (int i = 0; i < 3; ++i) if (d_k[i] != k1.current() && d_k[i] != k2.current()) plan.release(SNP_K0 + i);
            for (int i = 0; i < 3; ++i) if (d_v[i] != v1.current() && d_v[i] != v2.current()) plan.release(SNP_V0 + i);
        }

        // the candidates of every window counted, and their places
        V.a = k1.current(); V.ia = v1.current(); V.b = k2.current(); V.ib = v2.current();
        if (P == 1) launch("k_snp_scan", k_snp_scan<KM, false>, idx_grid(W, 2048), 0, pool, off, list, swoff, n_s, W, V, counts, nullptr, nullptr);
        else launch("k_snp_scan", k_snp_scan<KM, true>, idx_grid(W, 2048), 0, pool, off, list, swoff, n_s, W, V, counts, nullptr, nullptr);
        prim(tmp, tmp_bytes, "rocprim::exclusive_scan", snp_scan_counts(counts, offs, W));
        const uint64_t c_pass = read_word(offs + W, "candidates counted");
        C += c_pass;
        if (P > 1 && c_pass) { // written, and kept on the host until every pass has run
            const uint64_t need_c = 16 * c_pass + RTK_SNP_SLACK; uint64_t room_c = 0;
            if (!snp_room(need_c, &room_c)) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: " + std::to_string(c_pass) + " candidates of one pass need " + std::to_string(need_c) + " bytes of device memory, " + std::to_string(room_c) + " are to be had");
            DevArr<uint64_t> raw; raw.alloc(2 * c_pass);
            launch("k_snp_scan", k_snp_scan<KM, true>, idx_grid(W, 2048), 0, pool, off, list, swoff, n_s, W, V, nullptr, offs, raw.p);
            try { gathered.resize(2 * C); } catch (const std::bad_alloc&) { return rtk_fail(RTK_ERR_IO, "rtk_index_snp_candidates: out of host memory"); }
            rtk_check(hipMemcpy(gathered.data() + 2 * (C - c_pass), raw.p, 16 * c_pass, hipMemcpyDeviceToHost), "hipMemcpy");
        }
        t_scan += clk.since() - t_viewed;
    }
    const double t_views = clk.since() - t_scan; // uploads, histograms and views: what is not search
    if (P > 1) for (int i = 0; i < SNP_BUFS; ++i) plan.release(i); // the views have served: the candidates are ordered in their place
    uint64_t R = C; HostOut<uint64_t> res;
    if (!res.alloc(2 * C)) return rtk_fail(RTK_ERR_IO, "rtk_index_snp_candidates: out of host memory");
    if (C) {
        // the candidates, their site keys and ids (both twice: the sort's other buffer), the kept indices, the order keys (twice)
        DevPlan<SNPC_BUFS> cplan({{"candidates", 16 * C}, {"site keys 0", 16 * C}, {"site keys 1", 16 * C}, {"site ids 0", 4 * C}, {"site ids 1", 4 * C}, {"kept", 8 * C}, {"order keys 0", 16 * C}, {"order keys 1", 16 * C}});
        const uint64_t need_c = cplan.bytes() + RTK_SNP_CAND_SLACK; uint64_t room_c = 0;
        if (!snp_room(need_c, &room_c)) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: " + std::to_string(C) + " candidates need " + std::to_string(need_c) + " bytes of device memory, " + std::to_string(room_c) + " are to be had");
        uint64_t* raw = cplan.alloc<uint64_t>(SNPC_CAND);
        if (P == 1) launch("k_snp_scan", k_snp_scan<KM, false>, idx_grid(W, 2048), 0, pool, off, list, swoff, n_s, W, V, nullptr, offs, raw);
        else rtk_check(hipMemcpy(raw, gathered.data(), 16 * C, hipMemcpyHostToDevice), "hipMemcpy");
        const km2_t* ordered = nullptr;
        R = snp_order(cplan, raw, C, (flags & RTK_SNP_FIRST_PER_SITE) != 0, &ordered);
        if (R > C) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: more candidates kept than found");
        rtk_check(hipMemcpy(res.p, ordered, 16 * R, hipMemcpyDeviceToHost), "hipMemcpy");
        for (uint64_t i = 0; i < R; ++i) std::swap(res.p[2 * i], res.p[2 * i + 1]); // (a 128-bit key lies low word first)
    }
    *cand_out = res.release(); *n_cand = R;
    if (clk.trace) fprintf(stderr, "rtk_index_snps: %llu windows of %llu unitigs searched against %llu k-mers, %llu candidates (%llu kept); views %.2f s, scan %.2f s\n", static_cast<unsigned long long>(W), static_cast<unsigned long long>(n_s),
                           static_cast<unsigned long long>(N), static_cast<unsigned long long>(C), static_cast<unsigned long long>(R), t_views, clk.since() - t_views);
    if (clk.trace && P > 1) fprintf(stderr, "rtk_index_snps: %u passes over the key space, the largest partition holds %llu of %llu k-mers; %llu of %llu bytes of device memory\n", P, static_cast<unsigned long long>(largest),
                                    static_cast<unsigned long long>(N), static_cast<unsigned long long>(plan.bytes() + RTK_SNP_SLACK), static_cast<unsigned long long>(room));
    return RTK_OK;
}

// rtk_index_snp_plan: what snp_candidates would do with `room` bytes (0: with what is to be had now), from the offsets alone; nothing is allocated.
template <class KM>
int snp_plan(int k, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint64_t room, uint32_t* passes, uint64_t* need_one, uint64_t* need_min) {
    SnpWindows win;
    if (const int rc = snp_windows(k, seq_off, n_unitigs, searched, &win)) return rc;
    const SnpShape shape = {k, seq_off[n_unitigs], n_unitigs, win.N, win.n_s, win.W};
    const SnpChoice c = snp_choose<KM>(shape, room ? room : snp_room(), rtk_knob_index_snp_passes());
    *passes = c.passes; *need_one = c.need_one; *need_min = c.need_min;
    return RTK_OK;
}
} // namespace
#endif
