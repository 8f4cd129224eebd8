// rtk_index_colour_end_subsampled / rtk_index_subsample_events: the events thinned out by coverage and their ids renumbered before they leave the device (k_sub_*).
#ifndef RTK_INDEX_SUBSAMPLE_H
#define RTK_INDEX_SUBSAMPLE_H
#include <stdexcept>
#include <rocprim/rocprim.hpp>
#include "rtk_index_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ colours subsampled by coverage (k_sub_*)
// The rule is that of the index tool's host step (csrc/tools/index/subsample.hpp; the reference: addCoverage, src/Graph.cpp:2312-2870; DESIGN.md section 4 [A12]),
// and the two give the same words. The host works out what needs coverage and structure: the bin of every unitig (0 .. n_bins - 1, 255: none), which unitigs force
// ids (the non-branching ones), which bins are sampled and the rate. Everything that touches an event or an id happens here, on the sorted distinct events
// unitig << 32 | id in HBM:
//   k_sub_first_bin  one lane per event: the smallest bin among the unitigs an id colours, one byte per id (255: the id colours nothing, 254: only unitigs of no bin)
//   k_sub_forced     the events of a unitig are one segment; its first lane finds the end by bisection. Up to mcv events: all forced. Up to 64: the lane selects the
//                    mcv smallest (h(id), id) itself. Longer: the wave selects them together, mcv laps of a strided sweep and a minimum across the lanes.
//   k_sub_keep       one wave per word of the keep bitmap: an id is kept when its bin is not sampled, or u(id) <= rate; OR-ed onto the forced bits
//   ranks            exclusive scan of the population counts of the bitmap words (rocPRIM); the new id of a kept id = prefix of its word + the kept bits below it
//   compaction       rocprim::select over the events with the id replaced by its rank; renumbering is monotone, so the output is ascending and distinct
// h(id) = splitmix64 finalizer of id + seed * 0x9E3779B97F4A7C15; u(id) = (h >> 11) * 2^-53: an integer below 2^53 converted and scaled by a power of two, both exact,
// so host and device agree bit for bit. Bounds: events < the caller's count, ids < n_ids (tables of n_ids bytes / bits), unitigs < n_unitigs; an event that breaks
// one is skipped and reported.
#define RTK_SUB_MAX_MCV 64u
__device__ __forceinline__ uint64_t sub_hash(uint64_t id, uint64_t seed) {
    uint64_t z = id + seed * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ bool sub_key_less(uint64_t h1, uint64_t id1, uint64_t h2, uint64_t id2) { return h1 < h2 || (h1 == h2 && id1 < id2); }

__global__ void k_sub_first_bin(const uint64_t* __restrict__ ev, uint64_t n, const uint8_t* __restrict__ bin_of_unitig, uint32_t n_unitigs, uint32_t n_bins, uint64_t n_ids,
                                uint32_t* __restrict__ first_bin, uint32_t* __restrict__ bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t e = ev[i], u = e >> 32, id = e & 0xFFFFFFFFull;
        if (u >= n_unitigs || id >= n_ids) { atomicOr(bad, 1u); continue; }
        uint32_t v = bin_of_unitig[u];
        if (v == 255u) v = 254u; else if (v >= n_bins) { atomicOr(bad, 2u); continue; }
        uint32_t* w = first_bin + (id >> 2); const uint32_t sh = static_cast<uint32_t>(id & 3u) * 8u; // (the table is a whole number of words)
        uint32_t old = *w;
        while (((old >> sh) & 255u) > v) { const uint32_t seen = atomicCAS(w, old, (old & ~(255u << sh)) | (v << sh)); if (seen == old) break; old = seen; }
    }
}

__global__ void k_sub_forced(const uint64_t* __restrict__ ev, uint64_t n, const uint8_t* __restrict__ forced_candidate, uint32_t n_unitigs, uint32_t mcv, uint64_t seed, uint64_t n_ids,
                             unsigned long long* __restrict__ keep) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    auto force = [&](uint64_t id) { if (id < n_ids) atomicOr(keep + (id >> 6), 1ull << (id & 63ull)); };
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) { // (whole waves take part in every round)
        const uint64_t i = i0 + threadIdx.x;
        bool head = false; uint64_t len = 0;
        if (i < n) { const uint64_t u = ev[i] >> 32; head = (i == 0 || (ev[i - 1] >> 32) != u) && u < n_unitigs && forced_candidate[u] != 0;
            if (head) { // the end of the segment: the first event of a later unitig
                const uint64_t key = (u + 1) << 32; uint64_t lo = i + 1, hi = n;
                while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (ev[mid] < key) lo = mid + 1; else hi = mid; }
                len = lo - i;
            } }
        if (head && len <= mcv) for (uint64_t j = 0; j < len; ++j) force(ev[i + j] & 0xFFFFFFFFull);
        else if (head && len <= 64) { // the lane alone: mcv laps, each takes the smallest key above the one before
            uint64_t ph = 0, pid = 0;
            for (uint32_t r = 0; r < mcv; ++r) {
                uint64_t bh = ~0ull, bid = 1ull << 32;
                for (uint64_t j = 0; j < len; ++j) { const uint64_t id = ev[i + j] & 0xFFFFFFFFull, h = sub_hash(id, seed); if ((r == 0 || sub_key_less(ph, pid, h, id)) && sub_key_less(h, id, bh, bid)) { bh = h; bid = id; } }
                force(bid); ph = bh; pid = bid;
            }
        }
        uint64_t wide = __ballot(head && len > 64 && len > mcv ? 1 : 0);
        while (wide) { // the wave together, one long segment after the other
            const int src = __ffsll(static_cast<unsigned long long>(wide)) - 1; wide &= wide - 1;
            const uint64_t s0 = __shfl(static_cast<unsigned long long>(i), src, 64), sl = __shfl(static_cast<unsigned long long>(len), src, 64);
            uint64_t ph = 0, pid = 0;
            for (uint32_t r = 0; r < mcv; ++r) {
                uint64_t bh = ~0ull, bid = 1ull << 32;
                for (uint64_t j = static_cast<uint64_t>(lane); j < sl; j += 64) { const uint64_t id = ev[s0 + j] & 0xFFFFFFFFull, h = sub_hash(id, seed); if ((r == 0 || sub_key_less(ph, pid, h, id)) && sub_key_less(h, id, bh, bid)) { bh = h; bid = id; } }
                for (int d = 32; d >= 1; d >>= 1) { const uint64_t oh = __shfl_xor(static_cast<unsigned long long>(bh), d, 64), oid = __shfl_xor(static_cast<unsigned long long>(bid), d, 64); if (sub_key_less(oh, oid, bh, bid)) { bh = oh; bid = oid; } }
                if (lane == 0) force(bid);
                ph = bh; pid = bid;
            }
        }
    }
}

__global__ void k_sub_keep(const uint8_t* __restrict__ first_bin, uint64_t n_ids, uint64_t n_words, const uint8_t* __restrict__ bin_is_sampled, uint32_t n_bins, double rate, uint64_t seed,
                           unsigned long long* __restrict__ keep, unsigned long long* __restrict__ n_present) {
    const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, n_waves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long present = 0;
    for (uint64_t w = wave; w < n_words; w += n_waves) {
        const uint64_t id = 64 * w + static_cast<uint64_t>(lane);
        const uint32_t fb = id < n_ids ? first_bin[id] : 255u;
        bool kept = fb < n_bins;
        if (kept && bin_is_sampled[fb]) kept = static_cast<double>(sub_hash(id, seed) >> 11) * (1.0 / 9007199254740992.0) <= rate;
        const uint64_t bits = __ballot(kept ? 1 : 0), there = __ballot(fb != 255u ? 1 : 0);
        if (lane == 0) { if (bits) atomicOr(keep + w, static_cast<unsigned long long>(bits)); present += static_cast<unsigned long long>(__popcll(there)); }
    }
    if (lane == 0 && present) atomicAdd(n_present, present);
}

struct SubPopc { const unsigned long long* keep; uint64_t n_words; __device__ uint64_t operator()(uint64_t w) const { return w < n_words ? static_cast<uint64_t>(__popcll(keep[w])) : 0ull; } };
struct SubKept { const uint64_t* ev; const unsigned long long* keep; uint64_t n_ids; __device__ bool operator()(uint64_t i) const { const uint64_t id = ev[i] & 0xFFFFFFFFull; return id < n_ids && ((keep[id >> 6] >> (id & 63ull)) & 1ull) != 0; } };
struct SubRenumber { const uint64_t* ev; const unsigned long long* keep; const uint64_t* prefix; uint64_t n_ids;
    __device__ uint64_t operator()(uint64_t i) const { const uint64_t e = ev[i], id = e & 0xFFFFFFFFull; if (id >= n_ids) return e;
        return (e & 0xFFFFFFFF00000000ull) | (prefix[id >> 6] + static_cast<uint64_t>(__popcll(keep[id >> 6] & ((1ull << (id & 63ull)) - 1ull)))); } };

struct SubsampleRule { const uint8_t* bin_of_unitig; const uint8_t* forced_candidate; const uint8_t* bin_is_sampled; uint32_t n_bins, mcv; double rate; uint64_t seed; }; // (the caller's host arrays)
struct SubsampleResult { uint64_t n_out = 0, ids_before = 0, ids_after = 0; };

// d_ev: n sorted distinct events in device memory; d_out: room for n events there. Throws.
SubsampleResult subsample_events_device(const uint64_t* d_ev, uint64_t n, uint64_t* d_out, uint32_t n_unitigs, uint64_t n_ids, const SubsampleRule& rule) {
    SubsampleResult res;
    if (n == 0 || n_ids == 0) return res;
    const uint64_t n_words = (n_ids + 63) / 64, fb_words = (n_ids + 3) / 4; // the keep bitmap; the first-bin bytes, a whole number of 32-bit words
    const uint32_t n_bins = rule.n_bins;
    DevArr<uint8_t> bin, forced, sampled; DevArr<uint32_t> first_bin; DevArr<unsigned long long> keep, cnt; DevArr<uint64_t> prefix; DevArr<char> tmp; // cnt: ids present, events kept, flags of broken bounds
    bin.alloc(n_unitigs); forced.alloc(n_unitigs); sampled.alloc(n_bins); first_bin.alloc(fb_words); keep.alloc(n_words); prefix.alloc(n_words + 1); cnt.alloc(3);
    rtk_check(hipMemcpy(bin.p, rule.bin_of_unitig, n_unitigs, hipMemcpyHostToDevice), "hipMemcpy"); rtk_check(hipMemcpy(forced.p, rule.forced_candidate, n_unitigs, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemcpy(sampled.p, rule.bin_is_sampled, n_bins, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemset(first_bin.p, 0xFF, 4 * fb_words), "hipMemset"); rtk_check(hipMemset(keep.p, 0, 8 * n_words), "hipMemset"); rtk_check(hipMemset(cnt.p, 0, 24), "hipMemset");
    // which ids are kept
    launch("k_sub_first_bin", k_sub_first_bin, idx_grid(n), 0, d_ev, n, bin.p, n_unitigs, n_bins, n_ids, first_bin.p, reinterpret_cast<uint32_t*>(cnt.p + 2));
    if (rule.mcv) launch("k_sub_forced", k_sub_forced, idx_grid(n), 0, d_ev, n, forced.p, n_unitigs, rule.mcv, rule.seed, n_ids, keep.p);
    launch("k_sub_keep", k_sub_keep, idx_grid(64 * n_words), 0, reinterpret_cast<const uint8_t*>(first_bin.p), n_ids, n_words, sampled.p, n_bins, rule.rate, rule.seed, keep.p, cnt.p);
    // their ranks, and the events of the kept ids with the rank in place of the id
    auto idx = rocprim::make_counting_iterator<uint64_t>(0);
    SubPopc pc; pc.keep = keep.p; pc.n_words = n_words;
    auto counts = rocprim::make_transform_iterator(idx, pc);
    prim(tmp, "rocprim::exclusive_scan", [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, counts, prefix.p, 0ull, n_words + 1, rocprim::plus<uint64_t>()); });
    SubKept kp; kp.ev = d_ev; kp.keep = keep.p; kp.n_ids = n_ids;
    SubRenumber rn; rn.ev = d_ev; rn.keep = keep.p; rn.prefix = prefix.p; rn.n_ids = n_ids;
    auto flags = rocprim::make_transform_iterator(idx, kp); auto vals = rocprim::make_transform_iterator(idx, rn);
    prim(tmp, "rocprim::select", [&](void* t, size_t& b) { return rocprim::select(t, b, vals, flags, d_out, cnt.p + 1, n); });
    rtk_check(hipDeviceSynchronize(), "colours subsampled");
    unsigned long long h_cnt[3] = {0, 0, 0}; rtk_check(hipMemcpy(h_cnt, cnt.p, 24, hipMemcpyDeviceToHost), "hipMemcpy");
    if (h_cnt[2]) throw std::runtime_error("an event names a unitig, an id or a bin outside the tables");
    if (h_cnt[1] > n) throw std::runtime_error("more events kept than there were");
    res.n_out = h_cnt[1]; res.ids_before = h_cnt[0]; res.ids_after = read_word(prefix.p + n_words);
    return res;
}
const char* subsample_rule_bad(const SubsampleRule& r) {
    if (!r.bin_of_unitig || !r.forced_candidate || !r.bin_is_sampled) return "null argument";
    if (r.n_bins < 1 || r.n_bins > 64) return "1 to 64 bins";
    if (r.mcv > RTK_SUB_MAX_MCV) return "at most 64 forced ids per unitig";
    if (!(r.rate >= 0.0)) return "the rate is not a number >= 0";
    return nullptr;
}
} // namespace
#endif
