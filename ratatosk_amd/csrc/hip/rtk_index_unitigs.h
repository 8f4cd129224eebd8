// rtk_index_unitigs: the chains of the compacted graph walked, numbered and spelt on the device (k_ut_*).
#ifndef RTK_INDEX_UNITIGS_H
#define RTK_INDEX_UNITIGS_H
#include <string.h>
#include <cstdio>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "rtk_index_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ unitigs (rtk_index_unitigs)
// The solid k-mers in a table of slots {canonical k-mer, value}: value bits 0..3 = which of the four successors (x << 2 | b) of the canonical
// orientation are solid, bits 4..7 = which of the four predecessors (b in front), bit 8 = the k-mer lies on a unitig written here.
// One-word k-mers: 16-byte slots {key, value}. Two-word k-mers: 32-byte slots {hi, lo, value, unused}; the high word of a 2k-bit code (k <= 63) is
// never all ones, so it doubles as the state word: a slot is claimed by one 64-bit compare-and-swap on it (keys are distinct and the table is filled
// by a kernel of its own, before anything reads it) and the low word is written afterwards. Every lookup compares both words.
#define RTK_UT_CLAIMED 256ull
template <class KM> struct UtSlot { static const int W = 2, V = 1; };         // words per slot, word of the value
template <> struct UtSlot<km2_t> { static const int W = 4, V = 2; };
__device__ __forceinline__ uint64_t ut_find(const uint64_t* __restrict__ T, uint64_t slots, uint64_t can) {
    uint64_t s = __umul64hi(idx_hash(can), slots);
    for (;;) { const uint64_t key = T[2 * s]; if (key == can) return s; if (key == RTK_IDX_SENTINEL) return RTK_IDX_SENTINEL; s = s + 1 == slots ? 0 : s + 1; }
}
__device__ __forceinline__ uint64_t ut_find(const uint64_t* __restrict__ T, uint64_t slots, km2_t can) {
    const uint64_t hi = static_cast<uint64_t>(can >> 64), lo = static_cast<uint64_t>(can);
    uint64_t s = __umul64hi(idx_hash(can), slots);
    for (;;) { const uint64_t h = T[4 * s]; if (h == hi && T[4 * s + 1] == lo) return s; if (h == RTK_IDX_SENTINEL) return RTK_IDX_SENTINEL; s = s + 1 == slots ? 0 : s + 1; }
}
template <class KM> __device__ __forceinline__ uint64_t ut_vi(uint64_t s) { return UtSlot<KM>::W * s + UtSlot<KM>::V; } // word of slot s's value
__device__ __forceinline__ uint32_t rev4(uint32_t n) { return ((n & 1u) << 3) | ((n & 2u) << 1) | ((n & 4u) >> 1) | ((n & 8u) >> 3); }
// edge bits of an ORIENTED k-mer from those of its canonical form: the successor by base b of the reverse complement is the predecessor by base 3 - b
__device__ __forceinline__ uint32_t ut_omask(uint32_t m, bool is_can) { return is_can ? (m & 255u) : (rev4((m >> 4) & 15u) | (rev4(m & 15u) << 4)); }
template <class KM> __device__ __forceinline__ uint32_t ut_mask_of(const uint64_t* __restrict__ T, uint64_t slots, KM x, int k, uint64_t* slot_out) {
    const KM rc = idx_revcomp(x, k), can = x <= rc ? x : rc;
    const uint64_t s = ut_find(T, slots, can); if (slot_out) *slot_out = s;
    return ut_omask(static_cast<uint32_t>(T[ut_vi<KM>(s)]), x == can);
}
// the link the construction follows forwards from x (its oriented edge bits mx): the only successor of x, if x is its only predecessor
template <class KM> __device__ __forceinline__ bool ut_next(const uint64_t* __restrict__ T, uint64_t slots, int k, KM kmask, KM x, uint32_t mx, KM* y, uint32_t* my, uint64_t* slot_y) {
    const uint32_t sc = mx & 15u; if (__popc(sc) != 1) return false;
    const KM yy = ((x << 2) | static_cast<KM>(__ffs(sc) - 1)) & kmask;
    const uint32_t m = ut_mask_of(T, slots, yy, k, slot_y); if (__popc(m >> 4) != 1) return false;
    *y = yy; *my = m; return true;
}
template <class KM> __device__ __forceinline__ bool ut_prev(const uint64_t* __restrict__ T, uint64_t slots, int k, KM x, uint32_t mx) {
    const uint32_t pc = mx >> 4; if (__popc(pc) != 1) return false;
    const KM yy = (x >> 2) | (static_cast<KM>(__ffs(pc) - 1) << (2 * (k - 1)));
    return __popc(ut_mask_of(T, slots, yy, k, nullptr) & 15u) == 1;
}

template <class KM> __global__ void k_ut_fill(uint64_t* __restrict__ T, uint64_t slots) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < slots; i += stride) {
        T[UtSlot<KM>::W * i] = RTK_IDX_SENTINEL; for (int w = 1; w < UtSlot<KM>::W; ++w) T[UtSlot<KM>::W * i + w] = 0;
    }
}
template <class KM> __global__ void k_ut_insert(const KM* __restrict__ solid, uint64_t n, uint64_t* __restrict__ T, uint64_t slots) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const KM c = solid[i]; uint64_t s = __umul64hi(idx_hash(c), slots);
        const uint64_t w0 = sizeof(KM) == 8 ? static_cast<uint64_t>(c) : static_cast<uint64_t>(c >> (sizeof(KM) == 8 ? 0 : 64)); // key word / high word
        while (atomicCAS(reinterpret_cast<unsigned long long*>(T + UtSlot<KM>::W * s), static_cast<unsigned long long>(RTK_IDX_SENTINEL), static_cast<unsigned long long>(w0)) != RTK_IDX_SENTINEL) s = s + 1 == slots ? 0 : s + 1;
        if (sizeof(KM) != 8) T[UtSlot<KM>::W * s + 1] = static_cast<uint64_t>(c); // the low word of a slot this lane owns
    }
}
template <class KM> __global__ void k_ut_edges(const KM* __restrict__ solid, uint64_t n, int k, uint64_t* __restrict__ T, uint64_t slots) {
    const KM kmask = idx_kmask<KM>(k); const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const KM c = solid[i]; uint64_t m = 0;
        for (uint64_t b = 0; b < 4; ++b) {
            const KM y = ((c << 2) | static_cast<KM>(b)) & kmask, yr = idx_revcomp(y, k); if (ut_find(T, slots, y <= yr ? y : yr) != RTK_IDX_SENTINEL) m |= 1ull << b;
            const KM z = (c >> 2) | (static_cast<KM>(b) << (2 * (k - 1))), zr = idx_revcomp(z, k); if (ut_find(T, slots, z <= zr ? z : zr) != RTK_IDX_SENTINEL) m |= 16ull << b;
        }
        T[ut_vi<KM>(ut_find(T, slots, c))] = m;
    }
}
// Every maximal chain of mutually unique links is walked from both of its end k-mers; the end whose canonical k-mer is the smaller one owns it (tools/
// build_index.cpp fast_unitigs: the same rules, so that the two produce the same unitigs). An owner reports the oriented k-mer it starts from, the number of
// k-mers, the smallest canonical k-mer on the chain (its seed: unitigs are numbered by it) and whether that one reads backwards on the walk (the unitig is
// then the reverse complement of the walk). record == nullptr: count the owners only.
template <class KM>
__global__ void k_ut_chains(const KM* __restrict__ solid, uint64_t n, int k, const uint64_t* __restrict__ T, uint64_t slots,
                            unsigned long long* __restrict__ n_chains, uint64_t cap, KM* __restrict__ start, KM* __restrict__ seed, uint32_t* __restrict__ len_rev, uint32_t* __restrict__ too_long) {
    const KM kmask = idx_kmask<KM>(k); const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const KM s = solid[i];
        const uint32_t ms = ut_mask_of(T, slots, s, k, nullptr);
        KM y = 0; uint32_t my = 0;
        const bool has_fw = ut_next(T, slots, k, kmask, s, ms, &y, &my, nullptr), has_bw = ut_prev(T, slots, k, s, ms);
        if (has_fw && has_bw) continue; // inside a chain (or on a closed loop)
        KM x = has_bw ? idx_revcomp(s, k) : s; uint32_t mx = has_bw ? ut_omask(ms, false) : ms; // walk inwards from this end
        const KM x0 = x;
        uint64_t len = 1; KM mc = s; bool m_fw = (x == s);
        while (ut_next(T, slots, k, kmask, x, mx, &y, &my, nullptr)) {
            x = y; mx = my; ++len;
            const KM r = idx_revcomp(x, k), c = x <= r ? x : r;
            if (c < mc) { mc = c; m_fw = (x == c); }
            if (len > n) break;
        }
        const KM xr = idx_revcomp(x, k), end_c = x <= xr ? x : xr;
        if (len > 1 && end_c == s) continue; // the chain comes back to its own first k-mer (hairpin): left to the plain construction
        if (end_c < s) continue;            // the other end owns the chain
        if (len > n) continue;
        if (len >= (1ull << 31)) { atomicOr(too_long, 1u); continue; }
        const unsigned long long at = atomicAdd(n_chains, 1ull);
        if (start && at < cap) { start[at] = x0; seed[at] = mc; len_rev[at] = static_cast<uint32_t>(len) | (m_fw ? 0u : 0x80000000u); }
    }
}
struct ChainBases { const uint32_t* len_rev; const uint32_t* order; int k; __device__ uint64_t operator()(uint64_t j) const { return static_cast<uint64_t>(len_rev[order[j]] & 0x7FFFFFFFu) + static_cast<uint64_t>(k - 1); } };
// chain order[j] written as unitig j at seq_off[j]: walked again from its start, every k-mer claimed (a k-mer claimed twice: *clash)
template <class KM>
__global__ void k_ut_write(uint64_t n_ch, const uint32_t* __restrict__ order, const KM* __restrict__ start, const uint32_t* __restrict__ len_rev, const uint64_t* __restrict__ seq_off,
                           int k, uint64_t* __restrict__ T, uint64_t slots, char* __restrict__ pool, uint32_t* __restrict__ clash) {
    const KM kmask = idx_kmask<KM>(k); const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < n_ch; j += stride) {
        const uint32_t c = order[j]; const uint64_t len = len_rev[c] & 0x7FFFFFFFu; const bool rev = (len_rev[c] >> 31) != 0;
        const uint64_t L = len + static_cast<uint64_t>(k - 1); char* out = pool + seq_off[j];
        auto put = [&](uint64_t pos, uint32_t b) { if (!rev) out[pos] = "ACGT"[b]; else out[L - 1 - pos] = "TGCA"[b]; }; // base b at position pos of the walk
        KM x = start[c]; uint64_t slot = 0; uint32_t mx = ut_mask_of(T, slots, x, k, &slot);
        for (int q = 0; q < k; ++q) put(static_cast<uint64_t>(q), static_cast<uint32_t>((x >> (2 * (k - 1 - q))) & static_cast<KM>(3)));
        if (atomicOr(reinterpret_cast<unsigned long long*>(T + ut_vi<KM>(slot)), static_cast<unsigned long long>(RTK_UT_CLAIMED)) & RTK_UT_CLAIMED) atomicOr(clash, 1u);
        for (uint64_t q = 1; q < len; ++q) {
            KM y = 0; uint32_t my = 0;
            if (!ut_next(T, slots, k, kmask, x, mx, &y, &my, &slot)) { atomicOr(clash, 2u); break; }
            x = y; mx = my; put(static_cast<uint64_t>(k - 1) + q, static_cast<uint32_t>(x & static_cast<KM>(3)));
            if (atomicOr(reinterpret_cast<unsigned long long*>(T + ut_vi<KM>(slot)), static_cast<unsigned long long>(RTK_UT_CLAIMED)) & RTK_UT_CLAIMED) atomicOr(clash, 1u);
        }
    }
}
template <class KM> struct Unclaimed { const KM* solid; const uint64_t* T; uint64_t slots; __device__ bool operator()(uint64_t i) const { return !(T[ut_vi<KM>(ut_find(T, slots, solid[i]))] & RTK_UT_CLAIMED); } };

// Unitigs of the solid k-mers: every maximal chain of mutually unique links that does not meet itself, oriented so that its smallest canonical k-mer reads
// forwards, in the order of those k-mers -- what tools/build_index.cpp fast_unitigs builds on the host threads (the rules are restated there and here;
// tests/test_index_build.py holds both to the plain construction and to oracle/oracle_index.py). Chains that meet themselves (closed loops, hairpins through
// a reverse complement) are not built: their k-mers come back in *left (sorted) for the caller's plain construction.
template <class KM> struct UnitigStage {
    const int k; const uint64_t n, slots; // n solid k-mers in a table of `slots` slots
    DevArr<KM> solid, start, seed, seed_sorted, left; DevArr<uint64_t> T, off; DevArr<unsigned long long> n_chains, n_left;
    DevArr<uint32_t> flags, len_rev, order; DevArr<char> pool, tmp; // flags[0]: a chain of 2^31 k-mers or more, flags[1]: a k-mer claimed twice
    UnitigStage(int k_, uint64_t n_) : k(k_), n(n_), slots(n_ + n_ * 3 / 7 + 16) {}

    void build_table(const KM* h_solid) {
        solid.alloc(n); T.alloc(UtSlot<KM>::W * slots); n_chains.alloc(1); flags.alloc(2);
        rtk_check(hipMemcpy(solid.p, h_solid, sizeof(KM) * n, hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemset(flags.p, 0, 8), "hipMemset");
        launch("unitig table", k_ut_fill<KM>, idx_grid(slots), 0, T.p, slots);
        launch("unitig table", k_ut_insert<KM>, idx_grid(n), 0, solid.p, n, T.p, slots);
        launch("unitig table", k_ut_edges<KM>, idx_grid(n), 0, solid.p, n, k, T.p, slots);
        rtk_check(hipDeviceSynchronize(), "unitig table");
    }
    // the owners counted (cap == 0: nothing is recorded) or recorded
    uint64_t chains(uint64_t cap) {
        rtk_check(hipMemset(n_chains.p, 0, 8), "hipMemset");
        launch("k_ut_chains", k_ut_chains<KM>, idx_grid(n), 0, solid.p, n, k, T.p, slots, n_chains.p, cap, cap ? start.p : nullptr, cap ? seed.p : nullptr, cap ? len_rev.p : nullptr, flags.p);
        return read_word(n_chains.p, "k_ut_chains");
    }
    void alloc_chains(uint64_t n_ch) { start.alloc(n_ch); seed.alloc(n_ch); seed_sorted.alloc(n_ch); len_rev.alloc(n_ch); order.alloc(n_ch); off.alloc(n_ch + 1); }
    // the chains in the order of their seeds (one chain per seed: a k-mer lies on one chain) and the place of every sequence: h_off[0 .. n_ch], h_seed[0 .. n_ch)
    void order_chains(uint64_t n_ch, std::vector<uint64_t>& h_off, std::vector<KM>& h_seed) {
        auto iota = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), Iota32());
        prim(tmp, "rocprim::radix_sort_pairs", [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, seed.p, seed_sorted.p, iota, order.p, n_ch, 0, 2 * k); });
        ChainBases cb; cb.len_rev = len_rev.p; cb.order = order.p; cb.k = k;
        auto lens = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), cb);
        prim(tmp, "rocprim::exclusive_scan", [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, lens, off.p, 0ull, n_ch, rocprim::plus<uint64_t>()); });
        rtk_check(hipDeviceSynchronize(), "chain order");
        rtk_check(hipMemcpy(h_off.data(), off.p, 8 * n_ch, hipMemcpyDeviceToHost), "hipMemcpy");
        rtk_check(hipMemcpy(h_seed.data(), seed_sorted.p, sizeof(KM) * n_ch, hipMemcpyDeviceToHost), "hipMemcpy");
        const uint32_t last_lr = read_word(len_rev.p + read_word(order.p + (n_ch - 1)));
        h_off[n_ch] = h_off[n_ch - 1] + (last_lr & 0x7FFFFFFFu) + static_cast<uint64_t>(k - 1);
    }
    void write_sequences(uint64_t n_ch, uint64_t total) {
        pool.alloc(total);
        if (n_ch) { launch("k_ut_write", k_ut_write<KM>, idx_grid(n_ch), 0, n_ch, order.p, start.p, len_rev.p, off.p, k, T.p, slots, pool.p, flags.p + 1); rtk_check(hipDeviceSynchronize(), "k_ut_write"); }
    }
    // the k-mers on no unitig written here, in sorted order: how many
    uint64_t select_left() {
        left.alloc(n); n_left.alloc(1);
        Unclaimed<KM> un; un.solid = solid.p; un.T = T.p; un.slots = slots;
        auto flags_it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), un);
        const KM* ds = solid.p;
        prim(tmp, "rocprim::select", [&](void* t, size_t& b) { return rocprim::select(t, b, ds, flags_it, left.p, n_left.p, n); });
        return read_word(n_left.p, "left-over k-mers");
    }
    uint32_t flag(int i) { return read_word(flags.p + i); }
};

template <class KM> int unitigs(int k, const KM* solid, uint64_t n_solid, char** seq_pool, uint64_t** seq_off, uint64_t** seeds, uint64_t* n_unitigs, uint64_t** left, uint64_t* n_left) {
    const StageClock clk;
    UnitigStage<KM> S(k, n_solid);
    S.build_table(solid);
    const double t_table = clk.since();
    const uint64_t n_ch = S.chains(0);
    if (S.flag(0)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: a unitig of more than 2^31 k-mers");
    if (n_ch >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: more than 2^32 unitigs");
    S.alloc_chains(n_ch);
    S.chains(n_ch);
    const double t_chains = clk.since();
    std::vector<uint64_t> h_off(n_ch + 1, 0); std::vector<KM> h_seed(n_ch);
    if (n_ch) S.order_chains(n_ch, h_off, h_seed);
    const uint64_t total = h_off[n_ch];
    S.write_sequences(n_ch, total);
    if (S.flag(1)) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_unitigs: a k-mer ended up on two unitigs"); // (the tool then runs its plain construction)
    const double t_write = clk.since();
    const uint64_t nl = S.select_left();
    HostOut<char> o_pool; HostOut<uint64_t> o_off; HostOut<KM> o_seed, o_left;
    if (!o_pool.alloc(total) || !o_off.alloc(n_ch + 1) || !o_seed.alloc(n_ch) || !o_left.alloc(nl)) return rtk_fail(RTK_ERR_IO, "rtk_index_unitigs: out of host memory");
    if (total) rtk_check(hipMemcpy(o_pool.p, S.pool.p, total, hipMemcpyDeviceToHost), "hipMemcpy");
    memcpy(o_off.p, h_off.data(), 8 * (n_ch + 1)); if (n_ch) memcpy(o_seed.p, h_seed.data(), sizeof(KM) * n_ch);
    if (nl) rtk_check(hipMemcpy(o_left.p, S.left.p, sizeof(KM) * nl, hipMemcpyDeviceToHost), "hipMemcpy");
    *seq_pool = o_pool.release(); *seq_off = o_off.release(); *seeds = reinterpret_cast<uint64_t*>(o_seed.release()); *n_unitigs = n_ch; *left = reinterpret_cast<uint64_t*>(o_left.release()); *n_left = nl;
    if (clk.trace) fprintf(stderr, "rtk_index_unitigs: %llu unitigs, %llu bases, %llu k-mers left to the plain construction; table + edge bits %.2f s, chains %.2f s, order + sequences %.2f s, left-overs + copies %.2f s\n",
                           static_cast<unsigned long long>(n_ch), static_cast<unsigned long long>(total), static_cast<unsigned long long>(nl), t_table, t_chains - t_table, t_write - t_chains, clk.since() - t_write);
    return RTK_OK;
}
} // namespace
#endif
