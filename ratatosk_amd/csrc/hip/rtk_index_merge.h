// rtk_index_colour_merge / rtk_index_merge_events: the ids of read pairs on the same unitigs merged in place before the events leave the device (k_merge_*).
#ifndef RTK_INDEX_MERGE_H
#define RTK_INDEX_MERGE_H
#include <stdexcept>
#include <rocprim/rocprim.hpp>
#include "rtk_index_colour.h"    // sort_unique_events
#include "rtk_index_subsample.h" // sub_hash

namespace {
// ------------------------------------------------------------------------------------------------ ids of pairs on the same unitigs merged (k_merge_*)
// The rule is that of the index tool's host step (csrc/tools/index/merge.hpp; the reference: "Detecting and removing duplicated reads", src/Graph.cpp:1630-1705 and
// 2089-2134; DESIGN.md section 4 [A13]), and the two give the same words: ids whose unitig sets have the same sum S of g(u) = splitmix64 finalizer of u + 1 (modulo
// 2^64) and the same smallest unitig `low` are one class and take the number of the class's smallest id, the leaders numbered from 0 in ascending order.
// On the n sorted distinct events unitig << 32 | id, in the job's two event buffers and in tables of R entries, R = the ids that have events (never the largest id):
//   re-key + sort       the events as id << 32 | unitig, sorted (rocPRIM): an id is one run with its unitigs ascending; the other buffer takes the number of every
//                       event's run, counted from 1 (inclusive scan of the run heads), so R is its last word
//   k_merge_signature   one lane per event: the lanes of a run inside a wave are a segment (ballot of the segment heads), summed by a segmented shuffle sum; one
//                       64-bit add per run and wave into the high word of the run's key, the run's first event writes the low word low << 32 | id
//   sort                the R keys S << 64 | low << 32 | id with the run numbers as values (rocPRIM, 128-bit keys): a class is a stretch, its smallest id first
//   k_merge_leaders     one lane per sorted run: a class starts where (S, low) differs from the entry before; the leader comes from the head lane of the wave, and a
//                       wave whose first entry is no head finds the start of that class by bisection over the entries before it. Writes the leader's run for
//                       every run and the leader flags; the last entry of a class counts the classes above one id and the largest
//   ranks               exclusive scan of the leader flags in run (= id) order (rocPRIM)
//   k_merge_relabel     the id-major events rewritten in place to unitig << 32 | new id; the job's sort-and-unique brings them back to ascending and distinct
// No scratch, no LDS. Bounds: events < n, runs < R, unitigs < n_unitigs; an event that breaks one is skipped and reported.
struct MergeRekey { __device__ uint64_t operator()(uint64_t e) const { return (e << 32) | (e >> 32); } };
struct MergeRunHead { const uint64_t* ev; __device__ uint64_t operator()(uint64_t i) const { return i == 0 || (ev[i] >> 32) != (ev[i - 1] >> 32) ? 1ull : 0ull; } };
struct MergeLeaderFlag { const uint32_t* flag; uint64_t R; __device__ uint32_t operator()(uint64_t r) const { return r < R ? flag[r] : 0u; } };

__global__ void k_merge_signature(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ run_of, uint64_t n, uint64_t R, uint32_t n_unitigs, unsigned long long* __restrict__ keys, uint32_t* __restrict__ bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) { // (whole waves take part in every round)
        const uint64_t i = i0 + threadIdx.x;
        uint64_t run = ~0ull, g = 0, e = 0; // (a lane past the end, or with a broken event: a segment of its own that adds nothing)
        if (i < n) {
            e = ev[i]; run = run_of[i] - 1;
            if (run >= R || (e & 0xFFFFFFFFull) >= n_unitigs) { atomicOr(bad, 1u); run = ~0ull; }
            else g = sub_hash((e & 0xFFFFFFFFull) + 1, 0);
        }
        const uint64_t before = __shfl_up(static_cast<unsigned long long>(run), 1, 64);
        const bool head = lane == 0 || before != run;
        const uint64_t heads = __ballot(head ? 1 : 0);
        const uint64_t above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1); // the next segment head of the wave, if any
        const int end = above ? __ffsll(static_cast<unsigned long long>(above)) - 1 : 64;
        uint64_t sum = g; // after the laps: the sum over the lanes from this one to the end of its segment
        for (int d = 1; d < 64; d <<= 1) { const uint64_t t = __shfl_down(static_cast<unsigned long long>(sum), d, 64); if (lane + d < end) sum += t; }
        if (head && run != ~0ull) {
            atomicAdd(keys + 2 * run + 1, static_cast<unsigned long long>(sum));
            if (i == 0 || run_of[i - 1] != run_of[i]) keys[2 * run] = ((e & 0xFFFFFFFFull) << 32) | (e >> 32); // the run's first event: its smallest unitig, and the id
        }
    }
}

// (S, low) of entry a below that of entry b
__device__ __forceinline__ bool merge_class_less(uint64_t a_hi, uint64_t a_lo, uint64_t b_hi, uint64_t b_lo) { return a_hi < b_hi || (a_hi == b_hi && (a_lo >> 32) < (b_lo >> 32)); }

__global__ void k_merge_leaders(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order, uint64_t R, uint32_t* __restrict__ leader_of, uint32_t* __restrict__ is_leader,
                                unsigned long long* __restrict__ counts, uint32_t* __restrict__ bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; j0 < R; j0 += stride) { // (whole waves take part in every round)
        const uint64_t w0 = j0 + (threadIdx.x & ~63u), j = w0 + static_cast<uint64_t>(lane); // w0: the wave's first entry
        const bool there = j < R;
        uint64_t hi = 0, lo = 0; uint32_t ord = 0; bool head = false, last = false;
        if (there) {
            lo = keys[2 * j]; hi = keys[2 * j + 1]; ord = order[j];
            head = j == 0 || keys[2 * j - 1] != hi || (keys[2 * j - 2] >> 32) != (lo >> 32);
            last = j + 1 == R || keys[2 * j + 3] != hi || (keys[2 * j + 2] >> 32) != (lo >> 32);
        }
        // the class of the wave's first entry starts before the wave: the first entry that is not below it, found by bisection by lane 0
        uint64_t start0 = w0; uint32_t ord0 = 0;
        if (lane == 0 && there && !head) {
            uint64_t a = 0, b = w0;
            while (a < b) { const uint64_t mid = a + (b - a) / 2; if (merge_class_less(keys[2 * mid + 1], keys[2 * mid], hi, lo)) a = mid + 1; else b = mid; }
            start0 = a; ord0 = order[a];
        }
        start0 = __shfl(static_cast<unsigned long long>(start0), 0, 64); ord0 = __shfl(ord0, 0, 64);
        const uint64_t heads = __ballot(head ? 1 : 0), below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull)); // the heads at or below this lane
        const int src = below ? 63 - __clzll(static_cast<unsigned long long>(below)) : 0;
        const uint32_t ord_head = __shfl(ord, src, 64);
        const uint64_t start = below ? w0 + static_cast<uint64_t>(src) : start0;
        const uint32_t leader = below ? ord_head : ord0;
        const bool ok = there && ord < R && leader < R;
        if (there && !ok) atomicOr(bad, 2u);
        if (ok) { leader_of[ord] = leader; is_leader[ord] = head ? 1u : 0u; }
        // the last entry of a class knows its size: the wave's count of classes above one id and its largest, one atomic each
        unsigned long long size = ok && last ? j - start + 1 : 0ull;
        const uint64_t above_one = __ballot(size > 1 ? 1 : 0);
        for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(size, d, 64); size = o > size ? o : size; }
        if (lane == 0) { if (above_one) atomicAdd(counts, static_cast<unsigned long long>(__popcll(above_one))); if (size) atomicMax(counts + 1, size); }
    }
}

__global__ void k_merge_relabel(uint64_t* __restrict__ ev, const uint64_t* __restrict__ run_of, uint64_t n, uint64_t R, const uint32_t* __restrict__ leader_of, const uint32_t* __restrict__ rank) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t e = ev[i], run = run_of[i] - 1;
        if (run >= R) continue; // (reported by k_merge_signature)
        const uint32_t ld = leader_of[run];
        ev[i] = (e << 32) | static_cast<uint64_t>(ld < R ? rank[ld] : 0u);
    }
}

struct MergeResult { uint64_t n_out = 0, ids_before = 0, ids_after = 0, classes_above_one = 0, largest = 0; };

// the events at `a` re-keyed to id << 32 | unitig and sorted (`b`: the sort's other buffer); the other buffer then takes the number of every event's run, counted
// from 1. *ev, *run_of: where the two ended up. Returns R, the number of runs (= ids that have events).
uint64_t merge_runs_of_ids(uint64_t* a, uint64_t* b, uint64_t n, DevArr<char>& tmp, uint64_t** ev, uint64_t** run_of) {
    rtk_check(rocprim::transform(a, a, n, MergeRekey()), "rocprim::transform");
    rocprim::double_buffer<uint64_t> db(a, b);
    prim(tmp, "rocprim::radix_sort_keys", [&](void* t, size_t& s) { return rocprim::radix_sort_keys(t, s, db, n, 0, 64); });
    *ev = db.current(); *run_of = db.alternate();
    MergeRunHead rh; rh.ev = *ev;
    auto run_heads = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), rh);
    uint64_t* runs = *run_of;
    prim(tmp, "rocprim::inclusive_scan", [&](void* t, size_t& s) { return rocprim::inclusive_scan(t, s, run_heads, runs, n, rocprim::plus<uint64_t>()); });
    const uint64_t R = read_word(runs + (n - 1), "runs of the ids");
    if (R == 0 || R > n || R > (1ull << 32)) throw std::runtime_error("the runs of the ids do not add up");
    return R;
}

// a: n sorted distinct events in device memory, b: room for n words there. The merged events, ascending and distinct, end up in a or in b: the place is returned. Throws.
uint64_t* merge_events_device(uint64_t* a, uint64_t* b, uint64_t n, uint32_t n_unitigs, DevArr<char>& tmp, MergeResult* res) {
    *res = MergeResult();
    if (n == 0) return a;
    uint64_t* ev = nullptr; uint64_t* run_of = nullptr;
    const uint64_t R = merge_runs_of_ids(a, b, n, tmp, &ev, &run_of);
    DevArr<km2_t> keys, keys_sorted; DevArr<uint32_t> order, leader, is_leader, rank; DevArr<unsigned long long> cnt; // keys: S << 64 | low << 32 | id, in memory {low word, S}; cnt: classes above one id, the largest class, flags of broken bounds
    keys.alloc(R); keys_sorted.alloc(R); order.alloc(R); leader.alloc(R); is_leader.alloc(R); rank.alloc(R + 1); cnt.alloc(3);
    rtk_check(hipMemset(keys.p, 0, 16 * R), "hipMemset"); rtk_check(hipMemset(cnt.p, 0, 24), "hipMemset");
    uint32_t* bad = reinterpret_cast<uint32_t*>(cnt.p + 2);
    // the signature of every id, the classes of equal signatures and their leaders
    launch("k_merge_signature", k_merge_signature, idx_grid(n), 0, ev, run_of, n, R, n_unitigs, reinterpret_cast<unsigned long long*>(keys.p), bad);
    auto idx = rocprim::make_counting_iterator<uint64_t>(0);
    auto iota = rocprim::make_transform_iterator(idx, Iota32());
    prim(tmp, "rocprim::radix_sort_pairs", [&](void* t, size_t& s) { return rocprim::radix_sort_pairs(t, s, keys.p, keys_sorted.p, iota, order.p, R, 0, 128); });
    launch("k_merge_leaders", k_merge_leaders, idx_grid(R), 0, reinterpret_cast<const uint64_t*>(keys_sorted.p), order.p, R, leader.p, is_leader.p, cnt.p, bad);
    // the leaders numbered in id order, the events relabelled
    MergeLeaderFlag lf; lf.flag = is_leader.p; lf.R = R;
    auto flags = rocprim::make_transform_iterator(idx, lf);
    prim(tmp, "rocprim::exclusive_scan", [&](void* t, size_t& s) { return rocprim::exclusive_scan(t, s, flags, rank.p, 0u, R + 1, rocprim::plus<uint32_t>()); });
    launch("k_merge_relabel", k_merge_relabel, idx_grid(n), 0, ev, run_of, n, R, leader.p, rank.p);
    rtk_check(hipDeviceSynchronize(), "ids merged");
    unsigned long long h_cnt[3] = {0, 0, 0}; rtk_check(hipMemcpy(h_cnt, cnt.p, 24, hipMemcpyDeviceToHost), "hipMemcpy");
    if (h_cnt[2]) throw std::runtime_error("an event names a unitig or a run outside the tables");
    res->ids_before = R; res->ids_after = read_word(rank.p + R); res->classes_above_one = h_cnt[0]; res->largest = h_cnt[1];
    return sort_unique_events(ev, run_of, n, tmp, &res->n_out);
}
} // namespace
#endif
