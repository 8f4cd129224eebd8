// rtk_index_pair_ids: the colour id of every read from the hash of its name -- the rank of the name by first appearance (k_pair_*).
#ifndef RTK_INDEX_PAIRS_H
#define RTK_INDEX_PAIRS_H
#include <cstdio>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "rtk_index_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ ids of the read pairs by name (rtk_index_pair_ids)
// The reference hands a read pair its id by name (addCoverage, src/Graph.cpp:1595-1608, 1800-1804: name_hmap.insert({wyhash(name), nextID})): ids in the order in which
// names are first seen, every later record of the name gets the id of the first. Here (DESIGN.md section 4 [A18]; the host rule: csrc/tools/index/colour.hpp) the caller
// hashes the names, record r of the input has the ordinal r and the hash name_hash[r], and
//   sort          (hash, ordinal) radix-sorted by the hash (rocPRIM; stable, and the ordinals go in ascending: equal hashes stay in ordinal order)
//   k_pair_heads  position i of the sorted order is a head where i = 0 or key[i] != key[i - 1]: head[i] = i, else 0
//   max-scan      an inclusive maximum scan of head[] (rocPRIM): every position gets the position of the head of its run -- the first appearance of its name
//   k_pair_leader leader[ordinal[i]] = ordinal[head[i]]
//   rank          an exclusive scan over the ordinals j of (leader[j] == j) (rocPRIM): rank[j] = the names first seen before record j; rank[n] = the number of names
//   k_pair_spread ids[i] = rank[leader[i]]
// When (hash, ordinal) twice over plus the sort's temporary do not fit the device (or RTK_INDEX_PAIR_PASSES says so) the hash space is cut into P equal ranges: pass p
// holds the hashes h with floor(h P / 2^64) = p. Equal hashes meet in one pass, and leader[] -- 4 bytes per record, the only array that lives across the passes -- is
// complete after the last. The hashes stay on the host and are streamed through a staging buffer in chunks of RTK_PAIR_CHUNK, every pass:
//   k_pair_count  the records of every pass counted (P <= 256 counters; a block counts in LDS first): the buffers of a pass are sized by the largest count, so a
//                 range that holds more than its even share (crafted input: the hashes are uniform otherwise) is seen before anything is written
//   select        of a chunk, the records of the pass KEEPING THEIR ORDER: an exclusive scan of the in-range flags (rocPRIM), then k_pair_select writes record i of the
//                 chunk to place (records of the pass so far) + offs[i]. No atomics: the order of the ordinals is what makes the sort's ties right.
// One pass (P = 1) copies the hashes into the sort's buffer and numbers them (k_pair_iota). The ids are the same words for every P.
// Bounds: an ordinal is chunk base + i < n; k_pair_select writes below the pass's count from k_pair_count (the host compares the two before it sorts); head[i] <= i < m;
// leader[] is zeroed first and holds ordinals < n; rank[] has n + 1 entries.
#define RTK_PAIR_MAX_PASSES 256u
#define RTK_PAIR_CHUNK (1ull << 20) // hashes per staging copy
#define RTK_PAIR_SLACK 4096ull      // on top of the list: the counters, the granularity of the allocations

__device__ __forceinline__ uint32_t pair_pass_of(uint64_t h, uint32_t P) { return static_cast<uint32_t>(__umul64hi(h, static_cast<uint64_t>(P))); }

__global__ void k_pair_count(const uint64_t* __restrict__ hash, uint64_t n, uint32_t P, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t c[RTK_PAIR_MAX_PASSES];
    for (uint32_t i = threadIdx.x; i < RTK_PAIR_MAX_PASSES; i += blockDim.x) c[i] = 0;
    __syncthreads();
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x; // (a launch counts one chunk, at most 2^20 records: the 32-bit counters in LDS cannot wrap)
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&c[pair_pass_of(hash[i], P)], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < P; i += blockDim.x) if (c[i]) atomicAdd(counts + i, static_cast<unsigned long long>(c[i]));
}
struct PairInPass { const uint64_t* hash; uint64_t n; uint32_t P, pass; __device__ uint32_t operator()(uint64_t i) const { return i < n && pair_pass_of(hash[i], P) == pass ? 1u : 0u; } };
// record i of the chunk (ordinal base + i), when it belongs to the pass, to place at + offs[i] of the pass's arrays, below cap
__global__ void k_pair_select(const uint64_t* __restrict__ hash, const uint32_t* __restrict__ offs, uint64_t n, uint64_t base, uint32_t P, uint32_t pass, uint64_t at, uint64_t cap,
                              uint64_t* __restrict__ keys, uint32_t* __restrict__ ords) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t h = hash[i], to = at + offs[i];
        if (pair_pass_of(h, P) == pass && to < cap) { keys[to] = h; ords[to] = static_cast<uint32_t>(base + i); }
    }
}
__global__ void k_pair_iota(uint32_t* __restrict__ ords, uint64_t n) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) ords[i] = static_cast<uint32_t>(i);
}
__global__ void k_pair_heads(const uint64_t* __restrict__ keys, uint64_t m, uint32_t* __restrict__ head) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? static_cast<uint32_t>(i) : 0u;
}
__global__ void k_pair_leader(const uint32_t* __restrict__ ords, const uint32_t* __restrict__ head, uint64_t m, uint32_t* __restrict__ leader) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += stride) leader[ords[i]] = ords[head[i]];
}
struct PairIsLeader { const uint32_t* leader; uint64_t n; __device__ uint32_t operator()(uint64_t j) const { return j < n && leader[j] == j ? 1u : 0u; } };
__global__ void k_pair_spread(const uint32_t* __restrict__ leader, const uint32_t* __restrict__ rank, uint64_t n, uint32_t* __restrict__ ids) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) ids[i] = rank[leader[i]];
}

// The rocPRIM primitives of the stage, each spelt once: sized on null buffers for the plan, run on the real ones.
inline auto pair_sort(rocprim::double_buffer<uint64_t>& keys, rocprim::double_buffer<uint32_t>& ords, uint64_t m) {
    return [&keys, &ords, m](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keys, ords, m, 0, 64); };
}
inline auto pair_head_scan(const uint32_t* head, uint32_t* out, uint64_t m) {
    return [head, out, m](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, head, out, m, rocprim::maximum<uint32_t>()); };
}
inline auto pair_select_scan(const uint64_t* hash, uint64_t n, uint32_t P, uint32_t pass, uint32_t* offs) {
    return [=](void* t, size_t& b) {
        PairInPass in; in.hash = hash; in.n = n; in.P = P; in.pass = pass;
        auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), in);
        return rocprim::exclusive_scan(t, b, it, offs, 0u, n + 1, rocprim::plus<uint32_t>());
    };
}
inline auto pair_rank_scan(const uint32_t* leader, uint64_t n, uint32_t* rank) {
    return [=](void* t, size_t& b) {
        PairIsLeader is; is.leader = leader; is.n = n;
        auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), is);
        return rocprim::exclusive_scan(t, b, it, rank, 0u, n + 1, rocprim::plus<uint32_t>());
    };
}

// What the stage needs for n records with passes of at most M records each (one pass: M = n), before anything is allocated. leader[] lives throughout; a pass has
// (hash, ordinal) twice over -- the sort's two buffers; heads and their scan lie in the buffers the sort left free -- and, with more than one pass, the staging chunk
// and its offsets; the end has rank[] and ids[]. The temporary is the largest any primitive asks for.
struct PairPlan { uint64_t leader, keys, ords, stage, offs, rank, ids, tmp; uint64_t bytes() const { return leader + std::max(2 * keys + 2 * ords + stage + offs, rank + ids) + tmp + RTK_PAIR_SLACK; } };
inline PairPlan pair_plan(uint64_t n, uint64_t M, bool one_pass) {
    rocprim::double_buffer<uint64_t> no_keys(nullptr, nullptr); rocprim::double_buffer<uint32_t> no_ords(nullptr, nullptr);
    const uint64_t chunk = std::min<uint64_t>(RTK_PAIR_CHUNK, n);
    size_t tmp = prim_bytes("rocprim::radix_sort_pairs (size)", pair_sort(no_keys, no_ords, M));
    tmp = std::max(tmp, prim_bytes("rocprim::inclusive_scan (size)", pair_head_scan(nullptr, nullptr, M)));
    tmp = std::max(tmp, prim_bytes("rocprim::exclusive_scan (size)", pair_rank_scan(nullptr, n, nullptr)));
    if (!one_pass) tmp = std::max(tmp, prim_bytes("rocprim::exclusive_scan (size)", pair_select_scan(nullptr, chunk, 1, 0, nullptr)));
    PairPlan p; p.leader = 4 * n; p.keys = 8 * M; p.ords = 4 * M; p.stage = one_pass ? 0 : 8 * chunk; p.offs = one_pass ? 0 : 4 * (chunk + 1); p.rank = 4 * (n + 1); p.ids = 4 * n; p.tmp = tmp;
    return p;
}
inline uint64_t pair_need(uint64_t n, uint32_t P) { return pair_plan(n, (n + P - 1) / P, P == 1).bytes(); }
// what is to be had: the free device memory, or RTK_INDEX_PAIR_MEM when that is lower
inline uint64_t pair_room() { size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo"); return rtk_knob_index_pair_mem(static_cast<uint64_t>(fr)); }
// The number of passes for `room` bytes: the smallest P whose plan fits when every pass holds its even share ceil(n / P) of the records; the stage takes more when
// k_pair_count shows a heavier pass. forced != 0 (RTK_INDEX_PAIR_PASSES): that many and no other. passes == 0: nothing fits, and `need` is the smallest plan.
struct PairChoice { uint32_t passes; uint64_t need, need_one, need_min; };
inline PairChoice pair_choose(uint64_t n, uint64_t room, uint32_t forced) {
    const uint32_t first = forced ? std::min(forced, RTK_PAIR_MAX_PASSES) : 1u, last = forced ? first : RTK_PAIR_MAX_PASSES;
    PairChoice c; c.passes = 0; c.need_one = pair_need(n, 1); c.need_min = pair_need(n, RTK_PAIR_MAX_PASSES); c.need = forced ? pair_need(n, first) : c.need_min;
    for (uint32_t P = first; P <= last; ++P) {
        const uint64_t need = pair_need(n, P);
        if (need <= room) { c.passes = P; c.need = need; break; }
    }
    return c;
}

inline int pair_ids_device(const uint64_t* name_hash, uint64_t n, uint32_t* ids, uint64_t* n_ids) {
    const StageClock clk;
    (void)hipGetLastError(); // (what an earlier call of the process left behind -- a colouring job refused for memory -- is not this stage's: launch() asks for the last error)
    const uint64_t room = pair_room(); const uint32_t forced = rtk_knob_index_pair_passes();
    const PairChoice choice = pair_choose(n, room, forced);
    auto refusal = [&](uint64_t need, uint32_t passes) {
        return rtk_fail(RTK_ERR_DEVICE, "rtk_index_pair_ids: the names of " + std::to_string(n) + " records need " + std::to_string(need) + " bytes of device memory, " + std::to_string(room) + " are to be had (in " + std::to_string(passes) + " passes over the hash space)");
    };
    if (!choice.passes) return refusal(choice.need, forced ? std::min(forced, RTK_PAIR_MAX_PASSES) : RTK_PAIR_MAX_PASSES);
    uint32_t P = choice.passes;
    double t_copy = 0; // the seconds in copies between host and device
    auto copy = [&](void* to, const void* from, uint64_t bytes, hipMemcpyKind kind) { const double t = clk.since(); rtk_check(hipMemcpy(to, from, bytes, kind), "hipMemcpy"); t_copy += clk.since() - t; };
    const uint64_t chunk = std::min<uint64_t>(RTK_PAIR_CHUNK, n);

    // More than one pass: the records of every pass counted, and the plan with the largest of them -- more passes when that does not fit
    std::vector<unsigned long long> count(1, n); uint64_t largest = n;
    DevArr<uint64_t> stage; DevArr<uint32_t> offs;
    if (P > 1) {
        DevArr<unsigned long long> d_count; d_count.alloc(RTK_PAIR_MAX_PASSES); stage.alloc(chunk); offs.alloc(chunk + 1);
        for (;; ++P) {
            rtk_check(hipMemset(d_count.p, 0, 8 * RTK_PAIR_MAX_PASSES), "hipMemset");
            for (uint64_t b = 0; b < n; b += chunk) {
                const uint64_t c = std::min(chunk, n - b);
                copy(stage.p, name_hash + b, 8 * c, hipMemcpyHostToDevice);
                launch("k_pair_count", k_pair_count, idx_grid(c, 1024), 0, stage.p, c, P, d_count.p);
                rtk_check(hipDeviceSynchronize(), "k_pair_count"); // (the staging buffer is written again)
            }
            count.assign(P, 0); copy(count.data(), d_count.p, 8 * P, hipMemcpyDeviceToHost);
            uint64_t sum = 0; largest = 0; for (uint32_t p = 0; p < P; ++p) { sum += count[p]; largest = std::max<uint64_t>(largest, count[p]); }
            if (sum != n) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_pair_ids: the records counted for the passes are not the records");
            const uint64_t need = pair_plan(n, largest, false).bytes();
            if (need <= room) break;
            if (forced || P == RTK_PAIR_MAX_PASSES) return refusal(need, P);
        }
    }
    const PairPlan plan = pair_plan(n, largest, P == 1);
    DevArr<uint32_t> leader; leader.alloc(n); rtk_check(hipMemset(leader.p, 0, 4 * n), "hipMemset");
    DevArr<char> tmp; tmp.alloc(plan.tmp);
    {
        DevArr<uint64_t> k0, k1; DevArr<uint32_t> o0, o1; k0.alloc(largest); k1.alloc(largest); o0.alloc(largest); o1.alloc(largest);
        for (uint32_t pass = 0; pass < P; ++pass) {
            const uint64_t m = count[pass];
            if (m == 0) continue;
            rocprim::double_buffer<uint64_t> keys(k0.p, k1.p); rocprim::double_buffer<uint32_t> ords(o0.p, o1.p);
            if (P == 1) { copy(k0.p, name_hash, 8 * n, hipMemcpyHostToDevice); launch("k_pair_iota", k_pair_iota, idx_grid(n, 2048), 0, o0.p, n); }
            else {
                uint64_t at = 0;
                for (uint64_t b = 0; b < n; b += chunk) {
                    const uint64_t c = std::min(chunk, n - b);
                    copy(stage.p, name_hash + b, 8 * c, hipMemcpyHostToDevice);
                    prim(tmp.p, plan.tmp, "rocprim::exclusive_scan", pair_select_scan(stage.p, c, P, pass, offs.p));
                    launch("k_pair_select", k_pair_select, idx_grid(c, 2048), 0, stage.p, offs.p, c, b, P, pass, at, m, k0.p, o0.p);
                    at += read_word(offs.p + c, "records of a pass selected");
                    if (at > m) break;
                }
                if (at != m) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_pair_ids: a pass does not hold the records that were counted for it");
            }
            prim(tmp.p, plan.tmp, "rocprim::radix_sort_pairs", pair_sort(keys, ords, m));
            // heads in the ordinals' other buffer, their scan in the keys' other buffer (8 m bytes: room for m words)
            uint32_t* head = ords.alternate(); uint32_t* first = reinterpret_cast<uint32_t*>(keys.alternate());
            launch("k_pair_heads", k_pair_heads, idx_grid(m, 2048), 0, keys.current(), m, head);
            prim(tmp.p, plan.tmp, "rocprim::inclusive_scan", pair_head_scan(head, first, m));
            launch("k_pair_leader", k_pair_leader, idx_grid(m, 2048), 0, ords.current(), first, m, leader.p);
            rtk_check(hipDeviceSynchronize(), "first appearance of every name");
        }
    }
    stage.release(); offs.release();
    DevArr<uint32_t> rank, d_ids; rank.alloc(n + 1); d_ids.alloc(n);
    prim(tmp.p, plan.tmp, "rocprim::exclusive_scan", pair_rank_scan(leader.p, n, rank.p));
    launch("k_pair_spread", k_pair_spread, idx_grid(n, 2048), 0, leader.p, rank.p, n, d_ids.p);
    *n_ids = read_word(rank.p + n, "ids of the names");
    copy(ids, d_ids.p, 4 * n, hipMemcpyDeviceToHost);
    if (clk.trace) fprintf(stderr, "rtk_index_pairs: %llu records, %llu names, %u pass%s over the hash space (the largest holds %llu records); copies %.3f s, device stage %.3f s; %llu of %llu bytes of device memory\n",
                           static_cast<unsigned long long>(n), static_cast<unsigned long long>(*n_ids), P, P == 1 ? "" : "es", static_cast<unsigned long long>(largest), t_copy, clk.since() - t_copy,
                           static_cast<unsigned long long>(plan.bytes()), static_cast<unsigned long long>(room));
    return RTK_OK;
}

// rtk_index_pair_plan: what pair_ids_device would do for n records with `room` bytes (0: with what is to be had now); nothing is allocated.
inline int pair_plan_entry(uint64_t n, uint64_t room, uint32_t* passes, uint64_t* need_one, uint64_t* need_min) {
    const PairChoice c = pair_choose(n, room ? room : pair_room(), rtk_knob_index_pair_passes());
    *passes = c.passes; *need_one = c.need_one; *need_min = c.need_min;
    return RTK_OK;
}
} // namespace
#endif
