// GPU side of the index build (reference: `Ratatosk index`, src/Ratatosk.cpp:1066-1067 Bifrost build + src/Graph.cpp:1561 addCoverage).
// The reference builds its graph with Bifrost on the CPU; the data-parallel steps of an index build are done here on the device, behind the C ABI
// (include/ratatosk_hip.h), for the index tool (csrc/tools/build_index.cpp --gpu):
//   rtk_index_count_kmers   canonical k-mers of the reads seen >= min_count times: every read position spells its k-mer (one lane per position,
//                           the window packed 2 bits per base without branches), the k-mers of the pass are radix-sorted (rocPRIM) and the first
//                           element of every run of >= min_count equal keys is kept. HBM-bound: 1 byte read + 8 (16) bytes written per base, then the sort.
//   rtk_index_unitigs       the chains of the compacted graph walked, numbered and spelt (k_ut_*)
//   rtk_index_colour_*      every read k-mer mapped onto its unitig: colour events and coverage (k_col_map); with rtk_index_colour_end_subsampled the events
//                           thinned out by coverage and their ids renumbered before they leave the device (k_sub_*); with rtk_index_colour_merge the ids of read
//                           pairs on the same unitigs merged in place before that (k_merge_*); with rtk_index_colour_chunk_q the bases of a chunk whose quality
//                           is below a threshold turned into N ahead of the mapping (k_col_mask)
//   rtk_index_snp_candidates the candidate search of the SNP annotations: the graph k-mers one substitution away from every window of the searched unitigs (k_snp_*)
// Every step serves one-word k-mers (k <= 31, key type uint64_t) and two-word k-mers (33 <= k <= 63, key type unsigned __int128: the 2k-bit code,
// first base in the most significant bits; in memory the low word first). Own translation unit: rocPRIM's templates.
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../../include/ratatosk_hip.h"
#include "../common/fastx.hpp"
#include "../common/kmer.hpp"
#include "rtk_graph_tables.h"
#include "rtk_mem.h"
#include "rtk_types.h"

int rtk_fail(int code, const std::string& msg); // (rtk_device.hip)

namespace {

#define RTK_IDX_SENTINEL 0xFFFFFFFFFFFFFFFFull

typedef unsigned __int128 km2_t; // two-word k-mer (rocprim::uint128_t: radix-sortable)
__device__ __forceinline__ uint64_t idx_revcomp(uint64_t x, int k) { return rtk_revcomp(x, k); }
__device__ __forceinline__ uint64_t idx_hash(uint64_t x) { return rtk_hash64(x); }
__device__ __forceinline__ RtkKm idx_words(km2_t x) { RtkKm r; r.hi = static_cast<uint64_t>(x >> 64); r.lo = static_cast<uint64_t>(x); return r; }
__device__ __forceinline__ km2_t idx_km2(const RtkKm& x) { return (static_cast<km2_t>(x.hi) << 64) | static_cast<km2_t>(x.lo); }
__device__ __forceinline__ km2_t idx_revcomp(km2_t x, int k) { return idx_km2(rtk_km_revcomp(idx_words(x), k)); }
__device__ __forceinline__ uint64_t idx_hash(km2_t x) { return rtk_km_hash(idx_words(x)); } // (the hash of the wide k-mer table of rtk_graph_tables)
template <class KM> __device__ __forceinline__ KM idx_kmask(int k) { return (static_cast<KM>(1) << (2 * k)) - static_cast<KM>(1); }

// code of base c (A/a 0, C/c 1, G/g 2, T/t 3) or 4
__device__ __forceinline__ uint32_t idx_code(unsigned char c) {
    const unsigned char u = c & 0xDF; // upper case
    return u == 'A' ? 0u : (u == 'C' ? 1u : (u == 'G' ? 2u : (u == 'T' ? 3u : 4u)));
}

// One lane per character position of the chunk: the canonical k-mer that starts there (all k characters A/C/G/T, the separator between reads is
// not), kept when its hash falls into partition `part` of `n_part`. Survivors are appended to `keys` (wave-level compaction: one atomic per wave).
template <class KM>
__global__ void k_index_kmers(const char* __restrict__ chars, uint64_t n, int k, uint32_t part, uint32_t n_part, KM* __restrict__ keys, unsigned long long* __restrict__ top, uint64_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) {
        const uint64_t i = i0 + threadIdx.x;
        KM km = 0; bool ok = i + static_cast<uint64_t>(k) <= n;
        if (ok) {
            for (int j = 0; j < k; ++j) { const uint32_t c = idx_code(static_cast<unsigned char>(chars[i + j])); ok = ok && c < 4u; km = (km << 2) | static_cast<KM>(c & 3u); }
        }
        KM can = 0;
        if (ok) { const KM rc = idx_revcomp(km, k); can = km <= rc ? km : rc; ok = n_part <= 1u || (idx_hash(can) >> 40) % n_part == part; }
        const uint64_t bal = __ballot(ok ? 1 : 0);
        if (bal) {
            const int lane = threadIdx.x & 63;
            unsigned long long base = 0;
            if (lane == __ffsll(static_cast<unsigned long long>(bal)) - 1) base = atomicAdd(top, static_cast<unsigned long long>(__popcll(bal)));
            base = __shfl(base, __ffsll(static_cast<unsigned long long>(bal)) - 1, 64);
            const uint64_t at = base + static_cast<uint64_t>(__popcll(bal & ((1ull << lane) - 1ull)));
            if (ok && at < cap) keys[at] = can;
        }
    }
}

// first element of every run of >= min_count equal keys of a sorted array
template <class KM> struct SolidHead {
    const KM* keys; uint64_t n; uint32_t min_count;
    __device__ bool operator()(uint64_t i) const {
        const KM x = keys[i];
        if (i != 0 && keys[i - 1] == x) return false;
        return i + min_count - 1 < n && keys[i + min_count - 1] == x;
    }
};
template <class KM> struct KeyAt { const KM* keys; __device__ KM operator()(uint64_t i) const { return keys[i]; } };

struct DevBuf { void* p = nullptr; ~DevBuf() { if (p) (void)hipFree(p); } void alloc(uint64_t bytes) { if (p) (void)hipFree(p); p = nullptr; rtk_check(hipMalloc(&p, bytes ? bytes : 8), "hipMalloc (index build)"); } };
struct PinBuf { void* p = nullptr; ~PinBuf() { if (p) (void)hipHostFree(p); } void alloc(uint64_t bytes) { rtk_check(hipHostMalloc(&p, bytes, hipHostMallocDefault), "hipHostMalloc (index build)"); } };

// the sequences of the input files, chunk after chunk: a chunk = the read sequences of one byte range of a plain file, separated by '\n'
// (not a base), parsed by `n_threads` threads; handed to `sink(chars, n)` one chunk at a time (calls are serialised).
template <class Sink>
bool for_each_sequence_chunk(const std::vector<std::string>& files, int n_threads, uint64_t chunk_bytes, Sink sink, std::string* err) {
    for (size_t f = 0; f < files.size(); ++f) {
        if (rtk::SampleSource::is_spec(files[f])) { // reads sampled from a reference on the fly (common/sample_source.hpp): pair ranges, generated by the threads
            std::shared_ptr<rtk::SampleSource> ss = rtk::SampleSource::get(files[f], err);
            if (!ss) return false;
            const uint64_t L = ss->read_len(), per = std::max<uint64_t>(1, chunk_bytes / (2 * (L + 1))), n_ch = (ss->n_pairs() + per - 1) / per;
            std::atomic<uint64_t> next(0); std::mutex m_sink;
            std::vector<std::thread> th;
            const int nt = n_threads < 1 ? 1 : n_threads;
            for (int t = 0; t < nt; ++t) th.emplace_back([&]() {
                std::string buf;
                for (;;) {
                    const uint64_t c = next.fetch_add(1);
                    if (c >= n_ch) break;
                    const uint64_t p0 = c * per, p1 = std::min<uint64_t>(ss->n_pairs(), p0 + per);
                    buf.assign(static_cast<size_t>((p1 - p0) * 2 * (L + 1)), '\n');
                    for (uint64_t p = p0; p < p1; ++p) ss->pair(p, &buf[static_cast<size_t>((p - p0) * 2 * (L + 1))], &buf[static_cast<size_t>((p - p0) * 2 * (L + 1) + L + 1)]);
                    std::lock_guard<std::mutex> lk(m_sink);
                    sink(buf.data(), buf.size());
                }
            });
            for (size_t t = 0; t < th.size(); ++t) th[t].join();
            continue;
        }
        if (!rtk::PlainChunks::is_plain(files[f])) { // gzip or unknown: one reader thread
            rtk::FastxReader rd; if (!rd.open(files[f], n_threads < 16 ? n_threads : 16)) { *err = "cannot open " + files[f]; return false; } // (a gzip file of several members is inflated on the threads, common/mgzip.hpp)
            std::string name, seq, qual, buf; buf.reserve(chunk_bytes);
            while (rd.next(name, seq, qual)) { buf += seq; buf.push_back('\n'); if (buf.size() >= chunk_bytes) { sink(buf.data(), buf.size()); buf.clear(); } }
            if (rd.failed()) { *err = files[f] + " ends in a damaged or cut-short gzip stream"; return false; }
            if (!buf.empty()) sink(buf.data(), buf.size());
            continue;
        }
        rtk::PlainChunks pc; if (!pc.open(files[f], chunk_bytes)) { *err = "cannot open " + files[f]; return false; }
        std::atomic<size_t> next(0); std::mutex m_sink; std::atomic<bool> bad(false);
        std::vector<std::thread> th;
        const int nt = n_threads < 1 ? 1 : n_threads;
        for (int t = 0; t < nt; ++t) th.emplace_back([&]() {
            std::string buf;
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= pc.n_chunks() || bad) break;
                rtk::PackedReads r(false);
                if (!pc.parse_chunk(i, r)) { bad = true; break; }
                buf.clear(); buf.reserve(r.n_bases() + r.size());
                for (size_t x = 0; x < r.size(); ++x) { buf.append(r.seq(x), r.seq_len(x)); buf.push_back('\n'); }
                std::lock_guard<std::mutex> lk(m_sink);
                sink(buf.data(), buf.size());
            }
        });
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
        if (bad) { *err = "read error on " + files[f]; return false; }
    }
    return true;
}


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
struct Iota32 { __device__ uint32_t operator()(uint64_t i) const { return static_cast<uint32_t>(i); } };


// ------------------------------------------------------------------------------------------------ colours and coverage (rtk_index_colour_*)
// unitig sequences (characters, unitig u at off[u]) -> the 2-bit pool of the flat graph (base p at bits 2 (p & 31) of word p >> 5)
__global__ void k_col_pack(const char* __restrict__ pool, uint64_t n_bases, uint64_t* __restrict__ useq, uint64_t n_words) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; w < n_words; w += stride) {
        uint64_t x = 0;
        for (uint64_t j = 0; j < 32 && 32 * w + j < n_bases; ++j) x |= static_cast<uint64_t>(idx_code(static_cast<unsigned char>(pool[32 * w + j])) & 3u) << (2 * j);
        useq[w] = x;
    }
}
// One lane per character position of a chunk of reads (sequences separated by '\n'): its k-mer looked up in the unitig table. A run of consecutive
// positions of one read on one unitig is one EVENT (unitig << 32 | id of the read) and one addition of its length to the unitig's coverage, made by
// the first lane of the run inside its wave (a run that crosses a wave boundary gives two events: duplicates go when the events are sorted).
// the unitig of a one-word k-mer: 16-byte slots {canonical k-mer, unitig << 32 | ...}
__device__ __forceinline__ uint32_t col_find(const GraphView& g, uint64_t km, int k) {
    const uint64_t rc = idx_revcomp(km, k), can = km <= rc ? km : rc;
    const uint64_t* __restrict__ ht = g.ht; const uint64_t slots = g.ht_slots;
    uint64_t s = __umul64hi(idx_hash(can), slots);
    for (;;) { const uint64_t key = ht[2 * s]; if (key == can) return static_cast<uint32_t>(ht[2 * s + 1] >> 32); if (key == RTK_IDX_SENTINEL) return 0xFFFFFFFFu; s = s + 1 == slots ? 0 : s + 1; }
}
// the unitig of a two-word k-mer: the slots keep a fingerprint of the canonical k-mer, a match is confirmed against the unitig's bases
// (rtk_find_kmer_wide without the presence filters, which the index build's table does not have)
__device__ __forceinline__ uint32_t col_find(const GraphView& g, km2_t km, int k) {
    const RtkKm fw = idx_words(km), rc = rtk_km_revcomp(fw, k), can = rtk_km_less(fw, rc) ? fw : rc;
    const uint64_t fp = rtk_km_fingerprint(can); const uint64_t* __restrict__ ht = g.ht; const uint64_t slots = g.ht_slots;
    for (uint64_t s = rtk_ht_slot(rtk_km_hash(can), slots);; s = rtk_ht_next(s, slots)) {
        const uint64_t key = ht[2 * s];
        if (key == fp) {
            const uint64_t v = ht[2 * s + 1]; const uint32_t u = static_cast<uint32_t>(v >> 32);
            const RtkKm urc = rtk_km_rc_of_unitig(g, g.uoff[u] + ((v & 0xFFFFFFFFull) >> 1), k);
            if (rtk_km_eq(urc, rc) || rtk_km_eq(urc, fw)) return u;
        }
        if (key == RTK_EMPTY_KEY) return 0xFFFFFFFFu;
    }
}
template <class KM>
__global__ void k_col_map(const char* __restrict__ chars, uint64_t n, int k, const uint64_t* __restrict__ starts, const uint32_t* __restrict__ ids, uint32_t n_reads,
                          GraphView g, unsigned long long* __restrict__ cov, uint64_t* __restrict__ events, unsigned long long* __restrict__ top, uint64_t cap) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * blockDim.x; i0 < n; i0 += stride) { // (whole waves take part in every round)
        const uint64_t i = i0 + threadIdx.x;
        KM km = 0; bool ok = i + static_cast<uint64_t>(k) <= n;
        if (ok) for (int j = 0; j < k; ++j) { const uint32_t c = idx_code(static_cast<unsigned char>(chars[i + j])); ok = ok && c < 4u; km = (km << 2) | static_cast<KM>(c & 3u); }
        uint32_t u = 0xFFFFFFFFu;
        if (ok) u = col_find(g, km, k);
        const bool hit = u != 0xFFFFFFFFu;
        const uint32_t pu = __shfl_up(u, 1, 64); // (position i - 1 with a k-mer on the same unitig: the same read, its k-mer holds no separator)
        const bool head = hit && (lane == 0 || pu != u);
        const uint64_t heads = __ballot(head ? 1 : 0), hits = __ballot(hit ? 1 : 0);
        if (!heads) continue;
        const unsigned long long base = __shfl(lane == 0 ? atomicAdd(top, static_cast<unsigned long long>(__popcll(heads))) : 0ull, 0, 64);
        if (head) {
            const uint64_t above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1); // the next head of the wave, if any
            const int nxt = above ? __ffsll(static_cast<unsigned long long>(above)) - 1 : 64;
            const uint64_t span = (nxt == 64 ? ~0ull : ((1ull << nxt) - 1ull)) & ~((1ull << lane) - 1ull);
            atomicAdd(cov + u, static_cast<unsigned long long>(__popcll(hits & span)));
            uint32_t lo = 0, hi = n_reads; // the read of position i: the last one that starts at or before it
            while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (starts[mid] <= i) lo = mid; else hi = mid; }
            const uint64_t at = base + static_cast<uint64_t>(__popcll(heads & ((1ull << lane) - 1ull)));
            if (at < cap) events[at] = (static_cast<uint64_t>(u) << 32) | ids[lo];
        }
    }
}

// The base-confidence rule of a second-pass index (DESIGN.md section 4 [A14]; the reference: addCoverage, src/Graph.cpp:1806-1814 and 1872-1880): a base whose quality
// byte is below q_min becomes 'N' before the k-mers are looked up, so that k_col_map, which is not changed, gives no event and no coverage for a window over it. In
// place on the chunk's characters, on the chunk's stream, before k_col_map; the separators keep their byte whatever lies beside them in `quals`. Both buffers come from
// hipMalloc (16-byte aligned) and hold n bytes: a body of 16 bytes per lane and round, then the n & 15 bytes of the tail one per lane. Bytes compare unsigned.
__device__ __forceinline__ uint32_t col_mask_word(uint32_t c, uint32_t q, uint32_t q_min) {
    uint32_t r = c;
    for (int b = 0; b < 32; b += 8) if (((c >> b) & 255u) != static_cast<uint32_t>('\n') && ((q >> b) & 255u) < q_min) r = (r & ~(255u << b)) | (static_cast<uint32_t>('N') << b);
    return r;
}
__global__ void k_col_mask(char* __restrict__ chars, const unsigned char* __restrict__ quals, uint64_t n, uint32_t q_min) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x, t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x, n16 = n >> 4;
    uint4* __restrict__ c4 = reinterpret_cast<uint4*>(chars); const uint4* __restrict__ q4 = reinterpret_cast<const uint4*>(quals);
    for (uint64_t v = t; v < n16; v += stride) {
        uint4 c = c4[v]; const uint4 q = q4[v];
        c.x = col_mask_word(c.x, q.x, q_min); c.y = col_mask_word(c.y, q.y, q_min); c.z = col_mask_word(c.z, q.z, q_min); c.w = col_mask_word(c.w, q.w, q_min);
        c4[v] = c;
    }
    for (uint64_t i = (n16 << 4) + t; i < n; i += stride) if (chars[i] != '\n' && quals[i] < q_min) chars[i] = 'N';
}

// n words at `cur` sorted, the distinct ones kept: they end up at `cur` or at `other` (room for n words each; the place is returned), *n_out of them
uint64_t* sort_unique_events(uint64_t* cur, uint64_t* other, uint64_t n, DevBuf& tmp, uint64_t* n_out) {
    rocprim::double_buffer<uint64_t> db(cur, other);
    size_t tb = 0; rtk_check(rocprim::radix_sort_keys(nullptr, tb, db, static_cast<size_t>(n), 0, 64), "rocprim::radix_sort_keys");
    tmp.alloc(tb); rtk_check(rocprim::radix_sort_keys(tmp.p, tb, db, static_cast<size_t>(n), 0, 64), "rocprim::radix_sort_keys");
    uint64_t* sorted = db.current(); uint64_t* out = db.alternate();
    DevBuf d_n; d_n.alloc(8);
    size_t ub = 0; rtk_check(rocprim::unique(nullptr, ub, sorted, out, static_cast<unsigned long long*>(d_n.p), static_cast<size_t>(n)), "rocprim::unique");
    tmp.alloc(ub); rtk_check(rocprim::unique(tmp.p, ub, sorted, out, static_cast<unsigned long long*>(d_n.p), static_cast<size_t>(n)), "rocprim::unique");
    rtk_check(hipDeviceSynchronize(), "events sorted");
    unsigned long long nu = 0; rtk_check(hipMemcpy(&nu, d_n.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
    *n_out = nu; return out;
}

struct ColourJob {
    int device = 0, k = 31; uint32_t n_unitigs = 0; GraphView g; // g: the k-mer table and the packed unitigs (the only fields k_col_map reads)
    DevBuf useq, uoff, ht, cov, events, alt, top, tmp;
    uint64_t slots = 0, cap = 0, n_events = 0; // n_events: sorted, distinct events at the front of `events`
    uint64_t n_ids = 0;                        // largest id fed + 1 (after rtk_index_colour_merge: the number of merged ids): the size of the id tables of the subsampling
    uint64_t merge_classes_above_one = 0, merge_largest = 0; // what the last rtk_index_colour_merge found
    DevBuf d_chars[2], d_starts[2], d_ids[2]; PinBuf h_chars[2], h_starts[2], h_ids[2]; uint64_t chunk_cap = 0, reads_cap = 0;
    DevBuf d_quals[2]; PinBuf h_quals[2]; bool has_quals = false; // one chunk of quality bytes per slot, there from the job's first chunk with qualities on (rtk_index_colour_chunk_q)
    hipStream_t st[2] = {nullptr, nullptr}; int slot = 0;
    std::mutex m; uint64_t bases = 0, chunks = 0, compactions = 0; double t_table = 0.0;
    std::chrono::steady_clock::time_point t0;
    ~ColourJob() { if (st[0]) (void)hipStreamDestroy(st[0]); if (st[1]) (void)hipStreamDestroy(st[1]); }
    // the events so far sorted, the distinct ones kept (both streams idle)
    void compact() {
        rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        unsigned long long n = 0; rtk_check(hipMemcpy(&n, top.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        if (n > cap) throw std::runtime_error("more (unitig, read) events than the device buffer holds between two compactions (RTK_INDEX_EVENTS: number of events to make room for)");
        if (n == n_events) return;
        ++compactions;
        uint64_t nu = 0; const uint64_t* res = sort_unique_events(static_cast<uint64_t*>(events.p), static_cast<uint64_t*>(alt.p), n, tmp, &nu);
        if (res != static_cast<uint64_t*>(events.p)) rtk_check(hipMemcpy(events.p, res, 8 * nu, hipMemcpyDeviceToDevice), "hipMemcpy");
        n_events = nu; rtk_check(hipMemcpy(top.p, &nu, 8, hipMemcpyHostToDevice), "hipMemcpy");
    }
};

} // namespace

namespace {
// KM: uint64_t (k <= 31) or km2_t (33 <= k <= 63); *solid_out holds n_solid keys of sizeof(KM) bytes
template <class KM> int count_kmers(int device, int k, const char* const* files, int n_files, uint32_t min_count, int n_threads, uint64_t** solid_out, uint64_t* n_solid) {
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        std::vector<std::string> fl(files, files + n_files);
        // passes: the k-mers of one pass (one hash partition of the k-mer space) must fit twice (radix sort) next to what else lives on the device
        uint64_t total_bytes = 0;
        for (size_t f = 0; f < fl.size(); ++f) { if (rtk::SampleSource::is_spec(fl[f])) { std::string e_; std::shared_ptr<rtk::SampleSource> ss = rtk::SampleSource::get(fl[f], &e_); if (!ss) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + e_); total_bytes += 2 * ss->n_bases(); continue; } FILE* fp = fopen(fl[f].c_str(), "rb"); if (!fp) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: cannot open " + fl[f]); fseek(fp, 0, SEEK_END); total_bytes += static_cast<uint64_t>(ftell(fp)); fclose(fp); }
        size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
        if (rtk_knob_index_trace()) fprintf(stderr, "rtk_index_count_kmers: inputs sized (%.1f GB), %.1f GB of device memory free\n", total_bytes / 1e9, fr / 1e9);
        const uint64_t est_kmers = total_bytes / 2 + (1u << 20); // FASTQ: half of the bytes are bases (gzip input: a multiple of it; the capacity test below catches that)
        uint64_t cap = static_cast<uint64_t>(fr) / 10 * 7 / (2 * sizeof(KM)); // 70 % of the free memory for keys + their sort buffer (the rest: two chunks of text, the sort's histograms)
        cap = rtk_knob_index_cap(cap);
        if (cap < (1u << 20)) cap = 1u << 20;
        uint32_t n_part = static_cast<uint32_t>((est_kmers + cap - 1) / cap); if (n_part < 1) n_part = 1;
        const uint64_t chunk_bytes = rtk_knob_index_chunk(256ull << 20); // developer / tests: small chunks, so that long records are cut into pieces
        const uint64_t chunk_slack = std::min<uint64_t>(64ull << 20, chunk_bytes / 4);
        std::vector<KM> solid;
        // Several partitions = several passes over the reads. The text of the first pass is kept in host memory when it fits into half of what is free there
        // (a 3 Gb x 30x set: 90 GB of sequences, sampled or parsed ONCE instead of once per partition -- 13 passes at 0.5 Gb/s of host-side sampling were 36 minutes)
        std::vector<std::string> kept; bool keep_text = false, kept_complete = false;
        std::vector<size_t> run_start; // solid[run_start[p] ..): the sorted k-mers of partition p
        const bool trace = rtk_knob_index_trace(); const auto t_begin = std::chrono::steady_clock::now();
        auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
        { uint64_t avail = static_cast<uint64_t>(sysconf(_SC_AVPHYS_PAGES)) * static_cast<uint64_t>(sysconf(_SC_PAGE_SIZE));
          { // a container's memory limit is not what sysconf reports: what is left under the control group's limit, if there is one
            unsigned long long lim = 0, cur = 0; bool have = false;
            if (FILE* f1 = fopen("/sys/fs/cgroup/memory.max", "r")) { have = fscanf(f1, "%llu", &lim) == 1; fclose(f1); if (have) { if (FILE* f2 = fopen("/sys/fs/cgroup/memory.current", "r")) { if (fscanf(f2, "%llu", &cur) != 1) cur = 0; fclose(f2); } } }
            if (have && lim > cur && lim - cur < avail) avail = lim - cur; }
          const int kt = rtk_knob_index_keep_text(); keep_text = kt >= 0 ? kt != 0 : (est_kmers + est_kmers / 8 < avail / 2); // (the caller's own tables come on top of it later: half of what is left, no more)
          if (trace) fprintf(stderr, "rtk_index_count_kmers: %.1f GB of host memory to be had, text %s\n", avail / 1e9, keep_text ? "kept across partitions" : "read again for every partition"); }
        for (bool done = false; !done;) {
            done = true; solid.clear(); run_start.clear(); if (!kept_complete) kept.clear(); // (a restart with more partitions keeps the text of the complete first pass)
            const uint64_t cap_p = n_part == 1 ? std::min<uint64_t>(cap, est_kmers + est_kmers / 8) : cap;
            DevBuf d_keys, d_alt, d_top, d_chars[2], d_sel, d_nsel;
            d_keys.alloc(sizeof(KM) * cap_p); d_alt.alloc(sizeof(KM) * cap_p); d_top.alloc(8); d_nsel.alloc(8);
            d_chars[0].alloc(chunk_bytes + chunk_slack); d_chars[1].alloc(chunk_bytes + chunk_slack);
            PinBuf h_chars[2]; h_chars[0].alloc(chunk_bytes + chunk_slack); h_chars[1].alloc(chunk_bytes + chunk_slack);
            hipStream_t st[2]; rtk_check(hipStreamCreate(&st[0]), "hipStreamCreate"); rtk_check(hipStreamCreate(&st[1]), "hipStreamCreate");
            for (uint32_t part = 0; part < n_part && done; ++part) {
                rtk_check(hipMemset(d_top.p, 0, 8), "hipMemset");
                int slot = 0; std::string err; uint64_t n_sunk = 0, b_sunk = 0;
                if (trace) fprintf(stderr, "rtk_index_count_kmers: partition %u of %u starts at %.1f s (room for %llu k-mers)\n", part + 1, n_part, since(), static_cast<unsigned long long>(cap_p));
                auto sink = [&](const char* chars, size_t n) {
                    if (trace && (++n_sunk & 31u) == 0) fprintf(stderr, "rtk_index_count_kmers:   %llu chunks, %.1f GB of text at %.1f s\n", static_cast<unsigned long long>(n_sunk), b_sunk / 1e9, since());
                    b_sunk += n; // one chunk: pinned copy, H2D and the k-mer kernel on the slot's stream (the other slot's work overlaps the next parse)
                    for (size_t off = 0; off < n;) {
                        const size_t piece = std::min<size_t>(n - off, chunk_bytes + chunk_slack);
                        rtk_check(hipStreamSynchronize(st[slot]), "hipStreamSynchronize");
                        memcpy(h_chars[slot].p, chars + off, piece);
                        rtk_check(hipMemcpyAsync(d_chars[slot].p, h_chars[slot].p, piece, hipMemcpyHostToDevice, st[slot]), "hipMemcpyAsync");
                        hipLaunchKernelGGL(k_index_kmers<KM>, dim3(4096), dim3(256), 0, st[slot], static_cast<const char*>(d_chars[slot].p), static_cast<uint64_t>(piece), k, part, n_part,
                                           static_cast<KM*>(d_keys.p), static_cast<unsigned long long*>(d_top.p), cap_p);
                        rtk_check(hipGetLastError(), "kernel launch (k_index_kmers)");
                        slot ^= 1; off += (off + piece < n) ? piece - static_cast<size_t>(k - 1) : piece; // a cut inside a sequence: the next piece starts k - 1 characters back, so that every window is seen once
                    }
                };
                if (kept_complete) { for (size_t c = 0; c < kept.size(); ++c) sink(kept[c].data(), kept[c].size()); }
                else if (keep_text && n_part > 1) {
                    auto sink_keep = [&](const char* chars, size_t n) { kept.push_back(std::string(chars, n)); sink(chars, n); };
                    if (!for_each_sequence_chunk(fl, n_threads, chunk_bytes, sink_keep, &err)) { (void)hipStreamDestroy(st[0]); (void)hipStreamDestroy(st[1]); return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + err); }
                    kept_complete = true;
                }
                else if (!for_each_sequence_chunk(fl, n_threads, chunk_bytes, sink, &err)) { (void)hipStreamDestroy(st[0]); (void)hipStreamDestroy(st[1]); return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + err); }
                rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
                unsigned long long n_keys = 0; rtk_check(hipMemcpy(&n_keys, d_top.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
                if (n_keys > cap_p) { // more k-mers than estimated: more partitions, again
                    n_part = static_cast<uint32_t>((n_keys * static_cast<uint64_t>(n_part) + cap - 1) / cap) + 1; done = false; break;
                }
                if (n_keys == 0) continue;
                if (trace) fprintf(stderr, "rtk_index_count_kmers:   %llu k-mers on the device at %.1f s; sorting\n", n_keys, since());
                // sort, then the first key of every run of >= min_count
                rocprim::double_buffer<KM> db(static_cast<KM*>(d_keys.p), static_cast<KM*>(d_alt.p)); // (two-word keys: bits [0, 2k) of the 128-bit value)
                size_t tb = 0; rtk_check(rocprim::radix_sort_keys(nullptr, tb, db, static_cast<size_t>(n_keys), 0, 2 * k), "rocprim::radix_sort_keys");
                DevBuf d_tmp; d_tmp.alloc(tb);
                rtk_check(rocprim::radix_sort_keys(d_tmp.p, tb, db, static_cast<size_t>(n_keys), 0, 2 * k), "rocprim::radix_sort_keys");
                if (trace) { rtk_check(hipDeviceSynchronize(), "radix sort"); fprintf(stderr, "rtk_index_count_kmers:   sorted at %.1f s\n", since()); }
                const KM* sorted = db.current(); KM* other = db.alternate();
                SolidHead<KM> pred; pred.keys = sorted; pred.n = n_keys; pred.min_count = min_count;
                KeyAt<KM> at; at.keys = sorted;
                auto idx = rocprim::make_counting_iterator<uint64_t>(0);
                auto vals = rocprim::make_transform_iterator(idx, at);
                size_t sb = 0; // select with a flag iterator: the flag of element i is the predicate on its index
                auto flags = rocprim::make_transform_iterator(idx, pred);
                rtk_check(rocprim::select(nullptr, sb, vals, flags, other, static_cast<unsigned long long*>(d_nsel.p), static_cast<size_t>(n_keys)), "rocprim::select");
                d_tmp.alloc(sb);
                rtk_check(rocprim::select(d_tmp.p, sb, vals, flags, other, static_cast<unsigned long long*>(d_nsel.p), static_cast<size_t>(n_keys)), "rocprim::select");
                rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
                unsigned long long n_sel = 0; rtk_check(hipMemcpy(&n_sel, d_nsel.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
                const size_t old = solid.size(); solid.resize(old + n_sel); run_start.push_back(old);
                if (trace) fprintf(stderr, "rtk_index_count_kmers: partition %u of %u: %llu k-mers, %llu solid (at %.1f s%s)\n", part + 1, n_part, n_keys, n_sel, since(), kept_complete ? ", text kept in host memory" : "");
                if (n_sel) rtk_check(hipMemcpy(solid.data() + old, other, sizeof(KM) * n_sel, hipMemcpyDeviceToHost), "hipMemcpy");
            }
            (void)hipStreamDestroy(st[0]); (void)hipStreamDestroy(st[1]);
        }
        KM* out = static_cast<KM*>(malloc(sizeof(KM) * (solid.size() ? solid.size() : 1)));
        if (!out) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: out of host memory");
        if (run_start.size() <= 1) { if (!solid.empty()) memcpy(out, solid.data(), sizeof(KM) * solid.size()); }
        else {
            // the partitions are sorted each and a k-mer lives in one of them: merged by ranges of the key space, one range per thread (every thread finds its
            // stretch of every partition by bisection; the ranges before it give it its place in the output)
            const size_t P = run_start.size(); run_start.push_back(solid.size());
            const int T = n_threads < 1 ? 1 : (n_threads > 256 ? 256 : n_threads);
            std::vector<std::vector<size_t> > cut(static_cast<size_t>(T) + 1, std::vector<size_t>(P));
            const unsigned __int128 span = static_cast<unsigned __int128>(1) << (2 * k);
            for (int t = 0; t <= T; ++t) for (size_t r = 0; r < P; ++r) {
                if (t == T) { cut[t][r] = run_start[r + 1]; continue; }
                const KM v = sizeof(KM) == 8 ? static_cast<KM>(span * static_cast<unsigned __int128>(t) / static_cast<unsigned __int128>(T)) : static_cast<KM>(span / static_cast<unsigned __int128>(T) * static_cast<unsigned __int128>(t)); // (2^126 * t would not fit)
                cut[t][r] = static_cast<size_t>(std::lower_bound(solid.begin() + static_cast<std::ptrdiff_t>(run_start[r]), solid.begin() + static_cast<std::ptrdiff_t>(run_start[r + 1]), v) - solid.begin());
            }
            std::vector<std::thread> th;
            for (int t = 0; t < T; ++t) th.emplace_back([&, t]() {
                size_t at = 0; for (size_t r = 0; r < P; ++r) at += cut[t][r] - run_start[r];
                std::vector<size_t> head(cut[t]); const std::vector<size_t>& end = cut[t + 1];
                for (;;) { size_t best = P; KM bv = 0; for (size_t r = 0; r < P; ++r) if (head[r] < end[r] && (best == P || solid[head[r]] < bv)) { best = r; bv = solid[head[r]]; } if (best == P) break; out[at++] = bv; ++head[best]; }
            });
            for (size_t t = 0; t < th.size(); ++t) th[t].join();
        }
        if (trace) fprintf(stderr, "rtk_index_count_kmers: %zu solid k-mers from %u partition(s) in %.1f s\n", solid.size(), n_part, since());
        *solid_out = reinterpret_cast<uint64_t*>(out); *n_solid = solid.size();
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_count_kmers: ") + e.what()); }
    return RTK_OK;
}
} // namespace

extern "C" int rtk_index_count_kmers(int device, int k, const char* const* files, int n_files, uint32_t min_count, int n_threads, uint64_t** solid_out, uint64_t* n_solid) {
    if (!files || n_files <= 0 || !solid_out || !n_solid) return rtk_fail(RTK_ERR_ARG, "rtk_index_count_kmers: null argument");
    if (k < 3 || k > 63 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_count_kmers: odd k <= 63 only");
    if (min_count < 1) min_count = 1;
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_count_kmers: no such HIP device (no CPU fallback)");
    return k <= 31 ? count_kmers<uint64_t>(device, k, files, n_files, min_count, n_threads, solid_out, n_solid) : count_kmers<km2_t>(device, k, files, n_files, min_count, n_threads, solid_out, n_solid);
}


// Unitigs of the solid k-mers: every maximal chain of mutually unique links that does not meet itself, oriented so that its smallest canonical k-mer reads
// forwards, in the order of those k-mers -- what tools/build_index.cpp fast_unitigs builds on the host threads (the rules are restated there and here;
// tests/test_index_build.py holds both to the plain construction and to oracle/oracle_index.py). Chains that meet themselves (closed loops, hairpins through
// a reverse complement) are not built: their k-mers come back in *left (sorted) for the caller's plain construction.
namespace {
template <class KM> int unitigs(int device, int k, const KM* solid, uint64_t n_solid, char** seq_pool, uint64_t** seq_off, uint64_t** seeds, uint64_t* n_unitigs, uint64_t** left, uint64_t* n_left) {
    const bool trace = rtk_knob_index_trace();
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        const auto t0 = std::chrono::steady_clock::now();
        auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        const uint64_t n = n_solid, slots = n + n * 3 / 7 + 16;
        auto grid = [](uint64_t items) { const uint64_t b = (items + 255) / 256; return dim3(static_cast<unsigned>(b < 1 ? 1 : (b > 65536 ? 65536 : b))); };
        DevBuf d_solid, d_T, d_cnt, d_flag;
        d_solid.alloc(sizeof(KM) * n); d_T.alloc(8 * UtSlot<KM>::W * slots); d_cnt.alloc(8); d_flag.alloc(8);
        rtk_check(hipMemcpy(d_solid.p, solid, sizeof(KM) * n, hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemset(d_cnt.p, 0, 8), "hipMemset"); rtk_check(hipMemset(d_flag.p, 0, 8), "hipMemset");
        const KM* ds = static_cast<const KM*>(d_solid.p); uint64_t* T = static_cast<uint64_t*>(d_T.p);
        uint32_t* d_too_long = static_cast<uint32_t*>(d_flag.p); uint32_t* d_clash = d_too_long + 1;
        hipLaunchKernelGGL(k_ut_fill<KM>, grid(slots), dim3(256), 0, 0, T, slots);
        hipLaunchKernelGGL(k_ut_insert<KM>, grid(n), dim3(256), 0, 0, ds, n, T, slots);
        hipLaunchKernelGGL(k_ut_edges<KM>, grid(n), dim3(256), 0, 0, ds, n, k, T, slots);
        rtk_check(hipGetLastError(), "kernel launch (unitig table)"); rtk_check(hipDeviceSynchronize(), "unitig table");
        const double t_table = since();
        // owners counted, then recorded
        hipLaunchKernelGGL(k_ut_chains<KM>, grid(n), dim3(256), 0, 0, ds, n, k, static_cast<const uint64_t*>(T), slots, static_cast<unsigned long long*>(d_cnt.p), 0ull, static_cast<KM*>(nullptr), static_cast<KM*>(nullptr), static_cast<uint32_t*>(nullptr), d_too_long);
        rtk_check(hipGetLastError(), "kernel launch (k_ut_chains)"); rtk_check(hipDeviceSynchronize(), "k_ut_chains");
        unsigned long long n_ch = 0; rtk_check(hipMemcpy(&n_ch, d_cnt.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        uint32_t fl[2] = {0, 0}; rtk_check(hipMemcpy(fl, d_flag.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        if (fl[0]) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: a unitig of more than 2^31 k-mers");
        if (n_ch >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: more than 2^32 unitigs");
        DevBuf d_start, d_seed, d_seed2, d_lr, d_ord, d_ord2, d_off, d_tmp;
        d_start.alloc(sizeof(KM) * n_ch); d_seed.alloc(sizeof(KM) * n_ch); d_seed2.alloc(sizeof(KM) * n_ch); d_lr.alloc(4 * n_ch); d_ord.alloc(4 * n_ch); d_ord2.alloc(4 * n_ch); d_off.alloc(8 * (n_ch + 1));
        rtk_check(hipMemset(d_cnt.p, 0, 8), "hipMemset");
        hipLaunchKernelGGL(k_ut_chains<KM>, grid(n), dim3(256), 0, 0, ds, n, k, static_cast<const uint64_t*>(T), slots, static_cast<unsigned long long*>(d_cnt.p), static_cast<uint64_t>(n_ch), static_cast<KM*>(d_start.p), static_cast<KM*>(d_seed.p), static_cast<uint32_t*>(d_lr.p), d_too_long);
        rtk_check(hipGetLastError(), "kernel launch (k_ut_chains)"); rtk_check(hipDeviceSynchronize(), "k_ut_chains");
        const double t_chains = since();
        std::vector<uint64_t> h_off(n_ch + 1, 0); std::vector<KM> h_seed(n_ch);
        uint64_t total = 0;
        if (n_ch) {
            // the chains in the order of their seeds (one chain per seed: a k-mer lies on one chain)
            auto iota = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), Iota32());
            size_t tb = 0; rtk_check(rocprim::radix_sort_pairs(nullptr, tb, static_cast<KM*>(d_seed.p), static_cast<KM*>(d_seed2.p), iota, static_cast<uint32_t*>(d_ord.p), static_cast<size_t>(n_ch), 0, 2 * k), "rocprim::radix_sort_pairs");
            d_tmp.alloc(tb);
            rtk_check(rocprim::radix_sort_pairs(d_tmp.p, tb, static_cast<KM*>(d_seed.p), static_cast<KM*>(d_seed2.p), iota, static_cast<uint32_t*>(d_ord.p), static_cast<size_t>(n_ch), 0, 2 * k), "rocprim::radix_sort_pairs");
            ChainBases cb; cb.len_rev = static_cast<const uint32_t*>(d_lr.p); cb.order = static_cast<const uint32_t*>(d_ord.p); cb.k = k;
            auto lens = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), cb);
            size_t sb = 0; rtk_check(rocprim::exclusive_scan(nullptr, sb, lens, static_cast<uint64_t*>(d_off.p), 0ull, static_cast<size_t>(n_ch), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan");
            d_tmp.alloc(sb);
            rtk_check(rocprim::exclusive_scan(d_tmp.p, sb, lens, static_cast<uint64_t*>(d_off.p), 0ull, static_cast<size_t>(n_ch), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan");
            rtk_check(hipDeviceSynchronize(), "chain order");
            rtk_check(hipMemcpy(h_off.data(), d_off.p, 8 * n_ch, hipMemcpyDeviceToHost), "hipMemcpy");
            rtk_check(hipMemcpy(h_seed.data(), d_seed2.p, sizeof(KM) * n_ch, hipMemcpyDeviceToHost), "hipMemcpy");
            uint32_t last_c = 0, last_lr = 0; rtk_check(hipMemcpy(&last_c, static_cast<uint32_t*>(d_ord.p) + (n_ch - 1), 4, hipMemcpyDeviceToHost), "hipMemcpy");
            rtk_check(hipMemcpy(&last_lr, static_cast<uint32_t*>(d_lr.p) + last_c, 4, hipMemcpyDeviceToHost), "hipMemcpy");
            total = h_off[n_ch - 1] + (last_lr & 0x7FFFFFFFu) + static_cast<uint64_t>(k - 1); h_off[n_ch] = total;
        }
        DevBuf d_pool; d_pool.alloc(total ? total : 8);
        if (n_ch) {
            hipLaunchKernelGGL(k_ut_write<KM>, grid(n_ch), dim3(256), 0, 0, static_cast<uint64_t>(n_ch), static_cast<const uint32_t*>(d_ord.p), static_cast<const KM*>(d_start.p), static_cast<const uint32_t*>(d_lr.p), static_cast<const uint64_t*>(d_off.p), k, T, slots, static_cast<char*>(d_pool.p), d_clash);
            rtk_check(hipGetLastError(), "kernel launch (k_ut_write)"); rtk_check(hipDeviceSynchronize(), "k_ut_write");
        }
        rtk_check(hipMemcpy(fl, d_flag.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        if (fl[1]) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_unitigs: a k-mer ended up on two unitigs"); // (the tool then runs its plain construction)
        const double t_write = since();
        // the k-mers on no unitig written here, in sorted order
        DevBuf d_left, d_nleft; d_left.alloc(sizeof(KM) * (n ? n : 1)); d_nleft.alloc(8);
        Unclaimed<KM> un; un.solid = ds; un.T = T; un.slots = slots;
        { auto idx = rocprim::make_counting_iterator<uint64_t>(0); auto flags = rocprim::make_transform_iterator(idx, un);
          size_t sb = 0; rtk_check(rocprim::select(nullptr, sb, ds, flags, static_cast<KM*>(d_left.p), static_cast<unsigned long long*>(d_nleft.p), static_cast<size_t>(n)), "rocprim::select");
          d_tmp.alloc(sb);
          rtk_check(rocprim::select(d_tmp.p, sb, ds, flags, static_cast<KM*>(d_left.p), static_cast<unsigned long long*>(d_nleft.p), static_cast<size_t>(n)), "rocprim::select");
          rtk_check(hipDeviceSynchronize(), "left-over k-mers"); }
        unsigned long long nl = 0; rtk_check(hipMemcpy(&nl, d_nleft.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        char* o_pool = static_cast<char*>(malloc(total ? total : 1)); uint64_t* o_off = static_cast<uint64_t*>(malloc(8 * (n_ch + 1))); KM* o_seed = static_cast<KM*>(malloc(sizeof(KM) * (n_ch ? n_ch : 1))); KM* o_left = static_cast<KM*>(malloc(sizeof(KM) * (nl ? nl : 1)));
        if (!o_pool || !o_off || !o_seed || !o_left) { free(o_pool); free(o_off); free(o_seed); free(o_left); return rtk_fail(RTK_ERR_IO, "rtk_index_unitigs: out of host memory"); }
        if (total) rtk_check(hipMemcpy(o_pool, d_pool.p, total, hipMemcpyDeviceToHost), "hipMemcpy");
        memcpy(o_off, h_off.data(), 8 * (n_ch + 1)); if (n_ch) memcpy(o_seed, h_seed.data(), sizeof(KM) * n_ch);
        if (nl) rtk_check(hipMemcpy(o_left, d_left.p, sizeof(KM) * nl, hipMemcpyDeviceToHost), "hipMemcpy");
        *seq_pool = o_pool; *seq_off = o_off; *seeds = reinterpret_cast<uint64_t*>(o_seed); *n_unitigs = n_ch; *left = reinterpret_cast<uint64_t*>(o_left); *n_left = nl;
        if (trace) fprintf(stderr, "rtk_index_unitigs: %llu unitigs, %llu bases, %llu k-mers left to the plain construction; table + edge bits %.2f s, chains %.2f s, order + sequences %.2f s, left-overs + copies %.2f s\n",
                           n_ch, static_cast<unsigned long long>(total), nl, t_table, t_chains - t_table, t_write - t_chains, since() - t_write);
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_unitigs: ") + e.what()); }
    return RTK_OK;
}
} // namespace

extern "C" int rtk_index_unitigs(int device, int k, const uint64_t* solid, uint64_t n_solid, char** seq_pool, uint64_t** seq_off, uint64_t** seeds, uint64_t* n_unitigs, uint64_t** left, uint64_t* n_left) {
    if (!solid || !seq_pool || !seq_off || !seeds || !n_unitigs || !left || !n_left) return rtk_fail(RTK_ERR_ARG, "rtk_index_unitigs: null argument");
    if (k < 3 || k > 63 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: odd k <= 63 only");
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_unitigs: no such HIP device (no CPU fallback)");
    if (n_solid >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: more than 2^32 solid k-mers");
    *seq_pool = nullptr; *seq_off = nullptr; *seeds = nullptr; *left = nullptr; *n_unitigs = 0; *n_left = 0;
    return k <= 31 ? unitigs<uint64_t>(device, k, solid, n_solid, seq_pool, seq_off, seeds, n_unitigs, left, n_left)
                   : unitigs<km2_t>(device, k, reinterpret_cast<const km2_t*>(solid), n_solid, seq_pool, seq_off, seeds, n_unitigs, left, n_left); // (two words per k-mer, low word first)
}


// Colours and coverage of an index build (addCoverage, src/Graph.cpp:1561-1985: every read k-mer mapped onto its unitig) on the device. The caller -- the index
// tool, which owns the numbering of the reads (a pair keeps one id: name changes, or pair numbers of a sampled source) -- opens a job on the unitigs, feeds its
// reads chunk by chunk from any number of threads, and gets back the distinct (unitig, read id) events in sorted order and the k-mer coverage of every unitig.
//   begin  unitig u = seq_pool[seq_off[u] .. seq_off[u + 1]) (characters); the pool is packed to 2 bits and the k-mer table built in HBM (rtk_graph_tables.hip)
//   chunk  chars: sequences separated by '\n' (n_chars characters); read r starts at starts[r] and has the id ids[r]. At most RTK_COLOUR_CHUNK (64 MB) per call.
//   end    *events: n_events words unitig << 32 | id, ascending, distinct; *cov: n_unitigs counts. Freed with rtk_free. The job is gone afterwards (also on error).
extern "C" int rtk_index_colour_begin(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, void** job_out) {
    if (!seq_pool || !seq_off || !job_out || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_begin: null argument");
    if (k < 3 || k > 63 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_colour_begin: odd k <= 63 only");
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_colour_begin: no such HIP device (no CPU fallback)");
    if (n_unitigs >= 0xFFFFFFFFull) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_colour_begin: more than 2^32 - 1 unitigs");
    *job_out = nullptr;
    std::unique_ptr<ColourJob> J(new ColourJob());
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        J->t0 = std::chrono::steady_clock::now();
        J->device = device; J->k = k; J->n_unitigs = static_cast<uint32_t>(n_unitigs);
        const uint64_t n_bases = seq_off[n_unitigs], n_kmers = n_bases - n_unitigs * static_cast<uint64_t>(k - 1), n_words = (n_bases + 31) / 32;
        { DevBuf d_pool; d_pool.alloc(n_bases); rtk_check(hipMemcpy(d_pool.p, seq_pool, n_bases, hipMemcpyHostToDevice), "hipMemcpy");
          J->useq.alloc(8 * (n_words + 2)); rtk_check(hipMemset(J->useq.p, 0, 8 * (n_words + 2)), "hipMemset");
          hipLaunchKernelGGL(k_col_pack, dim3(4096), dim3(256), 0, 0, static_cast<const char*>(d_pool.p), n_bases, static_cast<uint64_t*>(J->useq.p), n_words);
          rtk_check(hipGetLastError(), "kernel launch (k_col_pack)"); rtk_check(hipDeviceSynchronize(), "k_col_pack"); }
        J->uoff.alloc(8 * (n_unitigs + 1)); rtk_check(hipMemcpy(J->uoff.p, seq_off, 8 * (n_unitigs + 1), hipMemcpyHostToDevice), "hipMemcpy");
        void* ht = nullptr; rtk::device_kmer_table(static_cast<const uint64_t*>(J->useq.p), static_cast<const uint64_t*>(J->uoff.p), J->n_unitigs, n_bases, n_kmers, k, &ht, &J->slots);
        J->ht.p = ht;
        memset(&J->g, 0, sizeof(J->g)); J->g.k = k; J->g.n_unitigs = J->n_unitigs; J->g.ht_slots = J->slots; J->g.ht = static_cast<const uint64_t*>(J->ht.p);
        J->g.useq = static_cast<const uint64_t*>(J->useq.p); J->g.uoff = static_cast<const uint64_t*>(J->uoff.p);
        J->cov.alloc(8 * n_unitigs); rtk_check(hipMemset(J->cov.p, 0, 8 * n_unitigs), "hipMemset");
        J->top.alloc(8); rtk_check(hipMemset(J->top.p, 0, 8), "hipMemset");
        J->chunk_cap = 64ull << 20; J->reads_cap = J->chunk_cap / 16; // (a read of fewer than 15 characters per 16 bytes of chunk: the caller splits such chunks)
        for (int i = 0; i < 2; ++i) {
            J->d_chars[i].alloc(J->chunk_cap); J->d_starts[i].alloc(8 * J->reads_cap); J->d_ids[i].alloc(4 * J->reads_cap);
            J->h_chars[i].alloc(J->chunk_cap); J->h_starts[i].alloc(8 * J->reads_cap); J->h_ids[i].alloc(4 * J->reads_cap);
            rtk_check(hipStreamCreate(&J->st[i]), "hipStreamCreate");
        }
        size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
        J->cap = static_cast<uint64_t>(fr) / 10 * 6 / 16; // 60 % of what is left for the events and their sort buffer
        J->cap = rtk_knob_index_events(J->cap);
        if (J->cap < 1024) J->cap = 1024;
        J->events.alloc(8 * J->cap); J->alt.alloc(8 * J->cap);
        J->t_table = std::chrono::duration<double>(std::chrono::steady_clock::now() - J->t0).count();
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_colour_begin: ") + e.what()); }
    *job_out = J.release();
    return RTK_OK;
}

// one chunk of either entry; quals == nullptr: no quality bytes, nothing of the masking step runs
static int colour_chunk(const char* entry, void* job, const char* chars, const unsigned char* quals, unsigned char q_min, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !chars || !starts || !ids) return rtk_fail(RTK_ERR_ARG, std::string(entry) + ": null argument");
    if (n_reads == 0 || n_chars == 0) return RTK_OK;
    if (n_chars > J->chunk_cap || n_reads > J->reads_cap) return rtk_fail(RTK_ERR_ARG, std::string(entry) + ": chunk larger than 64 MB of characters / 4 M reads");
    try {
        std::lock_guard<std::mutex> lk(J->m);
        rtk_check(hipSetDevice(J->device), "hipSetDevice");
        // room for this chunk's events (at most one per position): sort and keep the distinct ones when the buffer is half full
        if (J->chunks && ((J->chunks & 7u) == 0 || J->cap < (1ull << 30))) { // (looked at every 8th chunk: reading the counter waits for the device)
            rtk_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            unsigned long long n = 0; rtk_check(hipMemcpy(&n, J->top.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
            if (n > J->cap / 2) J->compact();
        }
        { uint32_t mx = 0; for (uint32_t r = 0; r < n_reads; ++r) mx = ids[r] > mx ? ids[r] : mx; J->n_ids = std::max<uint64_t>(J->n_ids, static_cast<uint64_t>(mx) + 1); }
        const int sl = J->slot; J->slot ^= 1;
        rtk_check(hipStreamSynchronize(J->st[sl]), "hipStreamSynchronize");
        memcpy(J->h_chars[sl].p, chars, n_chars); memcpy(J->h_starts[sl].p, starts, 8ull * n_reads); memcpy(J->h_ids[sl].p, ids, 4ull * n_reads);
        rtk_check(hipMemcpyAsync(J->d_chars[sl].p, J->h_chars[sl].p, n_chars, hipMemcpyHostToDevice, J->st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(J->d_starts[sl].p, J->h_starts[sl].p, 8ull * n_reads, hipMemcpyHostToDevice, J->st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(J->d_ids[sl].p, J->h_ids[sl].p, 4ull * n_reads, hipMemcpyHostToDevice, J->st[sl]), "hipMemcpyAsync");
        if (quals) { // (the slot's stream is idle since the synchronisation above: its pinned quality bytes are free to be written)
            if (!J->has_quals) { for (int i = 0; i < 2; ++i) { J->d_quals[i].alloc(J->chunk_cap); J->h_quals[i].alloc(J->chunk_cap); } J->has_quals = true; }
            memcpy(J->h_quals[sl].p, quals, n_chars);
            rtk_check(hipMemcpyAsync(J->d_quals[sl].p, J->h_quals[sl].p, n_chars, hipMemcpyHostToDevice, J->st[sl]), "hipMemcpyAsync");
            hipLaunchKernelGGL(k_col_mask, dim3(256), dim3(256), 0, J->st[sl], static_cast<char*>(J->d_chars[sl].p), static_cast<const unsigned char*>(J->d_quals[sl].p), n_chars, static_cast<uint32_t>(q_min));
            rtk_check(hipGetLastError(), "kernel launch (k_col_mask)");
        }
        if (J->k <= 31)
            hipLaunchKernelGGL(k_col_map<uint64_t>, dim3(4096), dim3(256), 0, J->st[sl], static_cast<const char*>(J->d_chars[sl].p), n_chars, J->k, static_cast<const uint64_t*>(J->d_starts[sl].p), static_cast<const uint32_t*>(J->d_ids[sl].p), n_reads,
                               J->g, static_cast<unsigned long long*>(J->cov.p), static_cast<uint64_t*>(J->events.p), static_cast<unsigned long long*>(J->top.p), J->cap);
        else
            hipLaunchKernelGGL(k_col_map<km2_t>, dim3(4096), dim3(256), 0, J->st[sl], static_cast<const char*>(J->d_chars[sl].p), n_chars, J->k, static_cast<const uint64_t*>(J->d_starts[sl].p), static_cast<const uint32_t*>(J->d_ids[sl].p), n_reads,
                               J->g, static_cast<unsigned long long*>(J->cov.p), static_cast<uint64_t*>(J->events.p), static_cast<unsigned long long*>(J->top.p), J->cap);
        rtk_check(hipGetLastError(), "kernel launch (k_col_map)");
        J->bases += n_chars; ++J->chunks;
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string(entry) + ": " + e.what()); }
    return RTK_OK;
}

extern "C" int rtk_index_colour_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads) {
    return colour_chunk("rtk_index_colour_chunk", job, chars, nullptr, 0, n_chars, starts, ids, n_reads);
}
// The same with the quality bytes of the reads beside their characters (a second-pass index coloured by base confidence: DESIGN.md section 4 [A14]). No qualities or
// q_min == 0 (no byte is below it): rtk_index_colour_chunk.
extern "C" int rtk_index_colour_chunk_q(void* job, const char* chars, const unsigned char* quals, unsigned char q_min, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads) {
    return colour_chunk("rtk_index_colour_chunk_q", job, chars, q_min ? quals : nullptr, q_min, n_chars, starts, ids, n_reads);
}

extern "C" int rtk_index_colour_end(void* job, uint64_t** events, uint64_t* n_events, uint64_t** cov) {
    std::unique_ptr<ColourJob> J(static_cast<ColourJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_end: null job");
    if (!events || !n_events || !cov) return RTK_OK; // (abandoned job: released)
    *events = nullptr; *cov = nullptr; *n_events = 0;
    try {
        rtk_check(hipSetDevice(J->device), "hipSetDevice");
        J->compact();
        uint64_t* ev = static_cast<uint64_t*>(malloc(8 * (J->n_events ? J->n_events : 1))); uint64_t* cv = static_cast<uint64_t*>(malloc(8ull * J->n_unitigs));
        if (!ev || !cv) { free(ev); free(cv); return rtk_fail(RTK_ERR_IO, "rtk_index_colour_end: out of host memory"); }
        if (J->n_events) rtk_check(hipMemcpy(ev, J->events.p, 8 * J->n_events, hipMemcpyDeviceToHost), "hipMemcpy");
        rtk_check(hipMemcpy(cv, J->cov.p, 8ull * J->n_unitigs, hipMemcpyDeviceToHost), "hipMemcpy");
        *events = ev; *n_events = J->n_events; *cov = cv;
        if (rtk_knob_index_trace()) fprintf(stderr, "rtk_index_colour: %llu characters in %llu chunks -> %llu distinct (unitig, read) events (sorted and thinned out %llu times); table %.2f s, all %.2f s\n", static_cast<unsigned long long>(J->bases),
                                               static_cast<unsigned long long>(J->chunks), static_cast<unsigned long long>(J->n_events), static_cast<unsigned long long>(J->compactions), J->t_table, std::chrono::duration<double>(std::chrono::steady_clock::now() - J->t0).count());
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_colour_end: ") + e.what()); }
    return RTK_OK;
}


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
namespace {
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

// d_ev: n sorted distinct events in device memory; d_out: room for n events there. The per-unitig and per-bin arrays are the caller's host arrays. Throws.
void subsample_events_device(const uint64_t* d_ev, uint64_t n, uint64_t* d_out, uint32_t n_unitigs, uint64_t n_ids, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled,
                             uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed, uint64_t* n_out, uint64_t* ids_before, uint64_t* ids_after) {
    *n_out = 0; *ids_before = 0; *ids_after = 0;
    if (n == 0 || n_ids == 0) return;
    auto grid = [](uint64_t items) { const uint64_t b = (items + 255) / 256; return dim3(static_cast<unsigned>(b < 1 ? 1 : (b > 65536 ? 65536 : b))); };
    const uint64_t n_words = (n_ids + 63) / 64, fb_bytes = (n_ids + 3) / 4 * 4;
    DevBuf d_bin, d_forced, d_sampled, d_fb, d_keep, d_prefix, d_cnt, d_tmp;
    d_bin.alloc(n_unitigs); d_forced.alloc(n_unitigs); d_sampled.alloc(n_bins); d_fb.alloc(fb_bytes); d_keep.alloc(8 * n_words); d_prefix.alloc(8 * (n_words + 1)); d_cnt.alloc(24);
    rtk_check(hipMemcpy(d_bin.p, bin_of_unitig, n_unitigs, hipMemcpyHostToDevice), "hipMemcpy"); rtk_check(hipMemcpy(d_forced.p, forced_candidate, n_unitigs, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemcpy(d_sampled.p, bin_is_sampled, n_bins, hipMemcpyHostToDevice), "hipMemcpy");
    rtk_check(hipMemset(d_fb.p, 0xFF, fb_bytes), "hipMemset"); rtk_check(hipMemset(d_keep.p, 0, 8 * n_words), "hipMemset"); rtk_check(hipMemset(d_cnt.p, 0, 24), "hipMemset");
    unsigned long long* keep = static_cast<unsigned long long*>(d_keep.p); unsigned long long* cnt = static_cast<unsigned long long*>(d_cnt.p); // cnt: ids present, events kept, flags of broken bounds
    hipLaunchKernelGGL(k_sub_first_bin, grid(n), dim3(256), 0, 0, d_ev, n, static_cast<const uint8_t*>(d_bin.p), n_unitigs, n_bins, n_ids, static_cast<uint32_t*>(d_fb.p), reinterpret_cast<uint32_t*>(cnt + 2));
    rtk_check(hipGetLastError(), "kernel launch (k_sub_first_bin)");
    if (mcv) { hipLaunchKernelGGL(k_sub_forced, grid(n), dim3(256), 0, 0, d_ev, n, static_cast<const uint8_t*>(d_forced.p), n_unitigs, mcv, seed, n_ids, keep); rtk_check(hipGetLastError(), "kernel launch (k_sub_forced)"); }
    hipLaunchKernelGGL(k_sub_keep, grid(64 * n_words), dim3(256), 0, 0, static_cast<const uint8_t*>(d_fb.p), n_ids, n_words, static_cast<const uint8_t*>(d_sampled.p), n_bins, rate, seed, keep, cnt);
    rtk_check(hipGetLastError(), "kernel launch (k_sub_keep)");
    auto idx = rocprim::make_counting_iterator<uint64_t>(0);
    SubPopc pc; pc.keep = keep; pc.n_words = n_words;
    auto counts = rocprim::make_transform_iterator(idx, pc);
    size_t sb = 0; rtk_check(rocprim::exclusive_scan(nullptr, sb, counts, static_cast<uint64_t*>(d_prefix.p), 0ull, static_cast<size_t>(n_words + 1), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan");
    d_tmp.alloc(sb);
    rtk_check(rocprim::exclusive_scan(d_tmp.p, sb, counts, static_cast<uint64_t*>(d_prefix.p), 0ull, static_cast<size_t>(n_words + 1), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan");
    SubKept kp; kp.ev = d_ev; kp.keep = keep; kp.n_ids = n_ids;
    SubRenumber rn; rn.ev = d_ev; rn.keep = keep; rn.prefix = static_cast<const uint64_t*>(d_prefix.p); rn.n_ids = n_ids;
    auto flags = rocprim::make_transform_iterator(idx, kp); auto vals = rocprim::make_transform_iterator(idx, rn);
    size_t lb = 0; rtk_check(rocprim::select(nullptr, lb, vals, flags, d_out, cnt + 1, static_cast<size_t>(n)), "rocprim::select");
    d_tmp.alloc(lb);
    rtk_check(rocprim::select(d_tmp.p, lb, vals, flags, d_out, cnt + 1, static_cast<size_t>(n)), "rocprim::select");
    rtk_check(hipDeviceSynchronize(), "colours subsampled");
    unsigned long long h_cnt[3] = {0, 0, 0}; rtk_check(hipMemcpy(h_cnt, cnt, 24, hipMemcpyDeviceToHost), "hipMemcpy");
    if (h_cnt[2]) throw std::runtime_error("an event names a unitig, an id or a bin outside the tables");
    if (h_cnt[1] > n) throw std::runtime_error("more events kept than there were");
    uint64_t total = 0; rtk_check(hipMemcpy(&total, static_cast<uint64_t*>(d_prefix.p) + n_words, 8, hipMemcpyDeviceToHost), "hipMemcpy");
    *n_out = h_cnt[1]; *ids_before = h_cnt[0]; *ids_after = total;
}
const char* subsample_args_bad(const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled, uint32_t n_bins, uint32_t mcv, double rate) {
    if (!bin_of_unitig || !forced_candidate || !bin_is_sampled) return "null argument";
    if (n_bins < 1 || n_bins > 64) return "1 to 64 bins";
    if (mcv > RTK_SUB_MAX_MCV) return "at most 64 forced ids per unitig";
    if (!(rate >= 0.0)) return "the rate is not a number >= 0";
    return nullptr;
}
} // namespace

// The coverage of every unitig once all chunks are mapped (and the events sorted, the distinct ones kept); the job stays alive for rtk_index_colour_end or
// rtk_index_colour_end_subsampled: the caller needs the coverage to work out the bins before the events can be thinned.
extern "C" int rtk_index_colour_cov(void* job, uint64_t** cov) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !cov) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_cov: null argument");
    *cov = nullptr;
    try {
        std::lock_guard<std::mutex> lk(J->m);
        rtk_check(hipSetDevice(J->device), "hipSetDevice");
        J->compact();
        uint64_t* cv = static_cast<uint64_t*>(malloc(8ull * J->n_unitigs));
        if (!cv) return rtk_fail(RTK_ERR_IO, "rtk_index_colour_cov: out of host memory");
        rtk_check(hipMemcpy(cv, J->cov.p, 8ull * J->n_unitigs, hipMemcpyDeviceToHost), "hipMemcpy");
        *cov = cv;
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_colour_cov: ") + e.what()); }
    return RTK_OK;
}

// rtk_index_colour_end with the events thinned out by coverage and renumbered on the device (the rule above); only the kept events are copied to the host.
extern "C" int rtk_index_colour_end_subsampled(void* job, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled, uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed,
                                               uint64_t** events, uint64_t* n_events, uint64_t* n_events_before, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    std::unique_ptr<ColourJob> J(static_cast<ColourJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_end_subsampled: null job");
    if (!events || !n_events || !n_events_before || !n_ids_before || !n_ids_after) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_end_subsampled: null argument");
    *events = nullptr; *n_events = 0;
    if (const char* bad = subsample_args_bad(bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate)) return rtk_fail(RTK_ERR_ARG, std::string("rtk_index_colour_end_subsampled: ") + bad);
    try {
        rtk_check(hipSetDevice(J->device), "hipSetDevice");
        J->compact();
        const auto t_sub = std::chrono::steady_clock::now();
        uint64_t n_out = 0;
        subsample_events_device(static_cast<const uint64_t*>(J->events.p), J->n_events, static_cast<uint64_t*>(J->alt.p), J->n_unitigs, J->n_ids, bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate, seed, &n_out, n_ids_before, n_ids_after);
        uint64_t* ev = static_cast<uint64_t*>(malloc(8 * (n_out ? n_out : 1)));
        if (!ev) return rtk_fail(RTK_ERR_IO, "rtk_index_colour_end_subsampled: out of host memory");
        if (n_out) { const hipError_t rc = hipMemcpy(ev, J->alt.p, 8 * n_out, hipMemcpyDeviceToHost); if (rc != hipSuccess) { free(ev); rtk_check(rc, "hipMemcpy"); } }
        *events = ev; *n_events = n_out; *n_events_before = J->n_events;
        if (rtk_knob_index_trace()) fprintf(stderr, "rtk_index_colour: %llu characters in %llu chunks -> %llu distinct (unitig, read) events (sorted and thinned out %llu times), %llu left after subsampling (%.3f s); table %.2f s, all %.2f s\n", static_cast<unsigned long long>(J->bases),
                                               static_cast<unsigned long long>(J->chunks), static_cast<unsigned long long>(J->n_events), static_cast<unsigned long long>(J->compactions), static_cast<unsigned long long>(n_out),
                                               std::chrono::duration<double>(std::chrono::steady_clock::now() - t_sub).count(), J->t_table, std::chrono::duration<double>(std::chrono::steady_clock::now() - J->t0).count());
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_colour_end_subsampled: ") + e.what()); }
    return RTK_OK;
}

// Stage entry for tests: the device function behind rtk_index_colour_end_subsampled on events of the caller (host arrays; ascending, distinct, unitigs < n_unitigs);
// events_out has room for n_events words.
extern "C" int rtk_index_subsample_events(int device, const uint64_t* events, uint64_t n_events, uint32_t n_unitigs, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled,
                                          uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed, uint64_t* events_out, uint64_t* n_out, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    if ((!events && n_events) || (!events_out && n_events) || !n_out || !n_ids_before || !n_ids_after || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: null argument");
    if (const char* bad = subsample_args_bad(bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate)) return rtk_fail(RTK_ERR_ARG, std::string("rtk_index_subsample_events: ") + bad);
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_subsample_events: no such HIP device (no CPU fallback)");
    uint64_t n_ids = 0;
    for (uint64_t i = 0; i < n_events; ++i) {
        if (i && events[i] <= events[i - 1]) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: the events are not ascending and distinct");
        if ((events[i] >> 32) >= n_unitigs) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: an event names a unitig >= n_unitigs");
        n_ids = std::max<uint64_t>(n_ids, (events[i] & 0xFFFFFFFFull) + 1);
    }
    for (uint32_t u = 0; u < n_unitigs; ++u) if (bin_of_unitig[u] != 255 && bin_of_unitig[u] >= n_bins) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: a unitig names a bin >= n_bins");
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        DevBuf d_ev, d_out; d_ev.alloc(8 * n_events); d_out.alloc(8 * n_events);
        if (n_events) rtk_check(hipMemcpy(d_ev.p, events, 8 * n_events, hipMemcpyHostToDevice), "hipMemcpy");
        subsample_events_device(static_cast<const uint64_t*>(d_ev.p), n_events, static_cast<uint64_t*>(d_out.p), n_unitigs, n_ids, bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate, seed, n_out, n_ids_before, n_ids_after);
        if (*n_out) rtk_check(hipMemcpy(events_out, d_out.p, 8 * *n_out, hipMemcpyDeviceToHost), "hipMemcpy");
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_subsample_events: ") + e.what()); }
    return RTK_OK;
}


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
namespace {
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
// a: n sorted distinct events in device memory, b: room for n words there. The merged events, ascending and distinct, end up in a or in b: the place is returned. Throws.
uint64_t* merge_events_device(uint64_t* a, uint64_t* b, uint64_t n, uint32_t n_unitigs, DevBuf& tmp, MergeResult* res) {
    *res = MergeResult();
    if (n == 0) return a;
    auto grid = [](uint64_t items) { const uint64_t blocks = (items + 255) / 256; return dim3(static_cast<unsigned>(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks))); };
    rtk_check(rocprim::transform(a, a, static_cast<size_t>(n), MergeRekey()), "rocprim::transform");
    rocprim::double_buffer<uint64_t> db(a, b);
    size_t tb = 0; rtk_check(rocprim::radix_sort_keys(nullptr, tb, db, static_cast<size_t>(n), 0, 64), "rocprim::radix_sort_keys");
    tmp.alloc(tb); rtk_check(rocprim::radix_sort_keys(tmp.p, tb, db, static_cast<size_t>(n), 0, 64), "rocprim::radix_sort_keys");
    uint64_t* ev = db.current(); uint64_t* run_of = db.alternate();
    auto idx = rocprim::make_counting_iterator<uint64_t>(0);
    MergeRunHead rh; rh.ev = ev;
    auto run_heads = rocprim::make_transform_iterator(idx, rh);
    size_t sb = 0; rtk_check(rocprim::inclusive_scan(nullptr, sb, run_heads, run_of, static_cast<size_t>(n), rocprim::plus<uint64_t>()), "rocprim::inclusive_scan");
    tmp.alloc(sb); rtk_check(rocprim::inclusive_scan(tmp.p, sb, run_heads, run_of, static_cast<size_t>(n), rocprim::plus<uint64_t>()), "rocprim::inclusive_scan");
    rtk_check(hipDeviceSynchronize(), "runs of the ids");
    uint64_t R = 0; rtk_check(hipMemcpy(&R, run_of + (n - 1), 8, hipMemcpyDeviceToHost), "hipMemcpy");
    if (R == 0 || R > n || R > (1ull << 32)) throw std::runtime_error("the runs of the ids do not add up");
    DevBuf d_keys, d_keys2, d_order, d_leader, d_flag, d_rank, d_cnt;
    d_keys.alloc(16 * R); d_keys2.alloc(16 * R); d_order.alloc(4 * R); d_leader.alloc(4 * R); d_flag.alloc(4 * R); d_rank.alloc(4 * (R + 1)); d_cnt.alloc(24);
    rtk_check(hipMemset(d_keys.p, 0, 16 * R), "hipMemset"); rtk_check(hipMemset(d_cnt.p, 0, 24), "hipMemset");
    unsigned long long* cnt = static_cast<unsigned long long*>(d_cnt.p); uint32_t* bad = reinterpret_cast<uint32_t*>(cnt + 2); // cnt: classes above one id, the largest class, flags of broken bounds
    hipLaunchKernelGGL(k_merge_signature, grid(n), dim3(256), 0, 0, static_cast<const uint64_t*>(ev), static_cast<const uint64_t*>(run_of), n, R, n_unitigs, static_cast<unsigned long long*>(d_keys.p), bad);
    rtk_check(hipGetLastError(), "kernel launch (k_merge_signature)");
    auto iota = rocprim::make_transform_iterator(idx, Iota32());
    size_t kb = 0; rtk_check(rocprim::radix_sort_pairs(nullptr, kb, static_cast<km2_t*>(d_keys.p), static_cast<km2_t*>(d_keys2.p), iota, static_cast<uint32_t*>(d_order.p), static_cast<size_t>(R), 0, 128), "rocprim::radix_sort_pairs");
    tmp.alloc(kb); rtk_check(rocprim::radix_sort_pairs(tmp.p, kb, static_cast<km2_t*>(d_keys.p), static_cast<km2_t*>(d_keys2.p), iota, static_cast<uint32_t*>(d_order.p), static_cast<size_t>(R), 0, 128), "rocprim::radix_sort_pairs");
    hipLaunchKernelGGL(k_merge_leaders, grid(R), dim3(256), 0, 0, static_cast<const uint64_t*>(d_keys2.p), static_cast<const uint32_t*>(d_order.p), R, static_cast<uint32_t*>(d_leader.p), static_cast<uint32_t*>(d_flag.p), cnt, bad);
    rtk_check(hipGetLastError(), "kernel launch (k_merge_leaders)");
    MergeLeaderFlag lf; lf.flag = static_cast<const uint32_t*>(d_flag.p); lf.R = R;
    auto flags = rocprim::make_transform_iterator(idx, lf);
    size_t rb = 0; rtk_check(rocprim::exclusive_scan(nullptr, rb, flags, static_cast<uint32_t*>(d_rank.p), 0u, static_cast<size_t>(R + 1), rocprim::plus<uint32_t>()), "rocprim::exclusive_scan");
    tmp.alloc(rb); rtk_check(rocprim::exclusive_scan(tmp.p, rb, flags, static_cast<uint32_t*>(d_rank.p), 0u, static_cast<size_t>(R + 1), rocprim::plus<uint32_t>()), "rocprim::exclusive_scan");
    hipLaunchKernelGGL(k_merge_relabel, grid(n), dim3(256), 0, 0, ev, static_cast<const uint64_t*>(run_of), n, R, static_cast<const uint32_t*>(d_leader.p), static_cast<const uint32_t*>(d_rank.p));
    rtk_check(hipGetLastError(), "kernel launch (k_merge_relabel)");
    rtk_check(hipDeviceSynchronize(), "ids merged");
    unsigned long long h_cnt[3] = {0, 0, 0}; rtk_check(hipMemcpy(h_cnt, cnt, 24, hipMemcpyDeviceToHost), "hipMemcpy");
    if (h_cnt[2]) throw std::runtime_error("an event names a unitig or a run outside the tables");
    uint32_t n_leaders = 0; rtk_check(hipMemcpy(&n_leaders, static_cast<uint32_t*>(d_rank.p) + R, 4, hipMemcpyDeviceToHost), "hipMemcpy");
    uint64_t n_out = 0; uint64_t* out = sort_unique_events(ev, run_of, n, tmp, &n_out);
    res->n_out = n_out; res->ids_before = R; res->ids_after = n_leaders; res->classes_above_one = h_cnt[0]; res->largest = h_cnt[1];
    return out;
}
} // namespace

// The ids of an open colouring job merged in place (the rule above): finishes the pending chunks and the last sort-and-unique, merges, and sets the job's events
// and ids, so that rtk_index_colour_end, rtk_index_colour_cov and rtk_index_colour_end_subsampled go on from the merged events. The job stays alive, also on error.
extern "C" int rtk_index_colour_merge(void* job, uint64_t* n_events_before, uint64_t* n_events_after, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !n_events_before || !n_events_after || !n_ids_before || !n_ids_after) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_merge: null argument");
    try {
        std::lock_guard<std::mutex> lk(J->m);
        rtk_check(hipSetDevice(J->device), "hipSetDevice");
        J->compact();
        const auto t_merge = std::chrono::steady_clock::now();
        MergeResult r; const uint64_t before = J->n_events;
        const uint64_t* out = merge_events_device(static_cast<uint64_t*>(J->events.p), static_cast<uint64_t*>(J->alt.p), J->n_events, J->n_unitigs, J->tmp, &r);
        if (before) {
            if (out != static_cast<uint64_t*>(J->events.p)) rtk_check(hipMemcpy(J->events.p, out, 8 * r.n_out, hipMemcpyDeviceToDevice), "hipMemcpy");
            J->n_events = r.n_out; J->n_ids = r.ids_after; rtk_check(hipMemcpy(J->top.p, &r.n_out, 8, hipMemcpyHostToDevice), "hipMemcpy");
        }
        J->merge_classes_above_one = r.classes_above_one; J->merge_largest = r.largest;
        *n_events_before = before; *n_events_after = J->n_events; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
        if (rtk_knob_index_trace()) fprintf(stderr, "rtk_index_colour: ids merged on the device: %llu -> %llu ids, %llu -> %llu events (%.3f s)\n", static_cast<unsigned long long>(r.ids_before), static_cast<unsigned long long>(r.ids_after),
                                               static_cast<unsigned long long>(before), static_cast<unsigned long long>(J->n_events), std::chrono::duration<double>(std::chrono::steady_clock::now() - t_merge).count());
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_colour_merge: ") + e.what()); }
    return RTK_OK;
}

// what the job's last rtk_index_colour_merge found about its classes: how many hold more than one id, and the ids of the largest (0 and 0 before any merge)
extern "C" int rtk_index_colour_merge_classes(void* job, uint64_t* classes_above_one, uint64_t* largest) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !classes_above_one || !largest) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_merge_classes: null argument");
    std::lock_guard<std::mutex> lk(J->m);
    *classes_above_one = J->merge_classes_above_one; *largest = J->merge_largest;
    return RTK_OK;
}

// Stage entry for tests: the device function behind rtk_index_colour_merge on events of the caller (host arrays; ascending, distinct, unitigs < n_unitigs);
// events_out has room for n_events words.
extern "C" int rtk_index_merge_events(int device, const uint64_t* events, uint64_t n_events, uint32_t n_unitigs, uint64_t* events_out, uint64_t* n_out, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    if ((!events && n_events) || (!events_out && n_events) || !n_out || !n_ids_before || !n_ids_after || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_merge_events: null argument");
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_merge_events: no such HIP device (no CPU fallback)");
    for (uint64_t i = 0; i < n_events; ++i) {
        if (i && events[i] <= events[i - 1]) return rtk_fail(RTK_ERR_ARG, "rtk_index_merge_events: the events are not ascending and distinct");
        if ((events[i] >> 32) >= n_unitigs) return rtk_fail(RTK_ERR_ARG, "rtk_index_merge_events: an event names a unitig >= n_unitigs");
    }
    *n_out = 0; *n_ids_before = 0; *n_ids_after = 0;
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        DevBuf d_a, d_b, d_tmp; d_a.alloc(8 * n_events); d_b.alloc(8 * n_events);
        if (n_events) rtk_check(hipMemcpy(d_a.p, events, 8 * n_events, hipMemcpyHostToDevice), "hipMemcpy");
        MergeResult r; const uint64_t* out = merge_events_device(static_cast<uint64_t*>(d_a.p), static_cast<uint64_t*>(d_b.p), n_events, n_unitigs, d_tmp, &r);
        if (r.n_out > n_events) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_merge_events: more events after the merge than before");
        if (r.n_out) rtk_check(hipMemcpy(events_out, out, 8 * r.n_out, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_out = r.n_out; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_merge_events: ") + e.what()); }
    return RTK_OK;
}


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
namespace {

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
inline dim3 snp_grid(uint64_t items) { const uint64_t b = (items + 255) / 256; return dim3(static_cast<unsigned>(b < 1 ? 1 : (b > 2048 ? 2048 : b))); }

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
// T[v] = the first entry whose top bits (key >> shift) are >= v, for v in 0 .. n_pref (n_pref = 2^bits: T[n_pref] = n). Lane i fills the values between the top bits of
// entries i - 1 and i, so every T[v] is written once. flag != nullptr: bit 1 set when two neighbouring keys are equal.
template <class KM> __global__ void k_snp_table(const KM* __restrict__ keys, uint64_t n, int shift, uint64_t n_pref, uint64_t* __restrict__ T, uint32_t* __restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i <= n; i += stride) {
        const uint64_t a = i == 0 ? 0 : static_cast<uint64_t>(keys[i - 1] >> shift) + 1, b = i == n ? n_pref : static_cast<uint64_t>(keys[i] >> shift);
        for (uint64_t v = a; v <= b && v <= n_pref; ++v) T[v] = i;
        if (flag && i != 0 && i < n && keys[i] == keys[i - 1]) atomicOr(flag, 2u);
    }
}

template <class KM> struct SnpViews { const KM* a; const uint32_t* ia; const uint64_t* ta; const KM* b; const uint32_t* ib; const uint64_t* tb; int k, shift; };
// The graph k-mers one substitution away from x (NeighbourIndex::scan): as (offset, base) of the ORIENTED neighbour of the window (flipped: x is the window's reverse
// complement). Those on the window's own unitig u are dropped. out == nullptr: counted only; else candidate number c goes to out[2 (at + c)], below `end`. Returns the count.
template <class KM>
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
        uint64_t i = V.ta[static_cast<uint64_t>(lo_key >> V.shift)]; const uint64_t e = V.ta[static_cast<uint64_t>(hi_key >> V.shift) + 1];
        { uint64_t hi = e; while (i < hi) { const uint64_t mid = i + (hi - i) / 2; if (V.a[mid] < lo_key) i = mid + 1; else hi = mid; } }
        for (; i < e; ++i) { const KM y = V.a[i]; if (y > hi_key) break; entry(y, V.ia[i]); }
    }
    { // same last half: the differing base lies in the first hi_n bases
        const KM r = ((x & lomask) << (2 * hi_n)) | (x >> (2 * lo_n)), lo_key = r & ~himask, hi_key = r | himask;
        uint64_t i = V.tb[static_cast<uint64_t>(lo_key >> V.shift)]; const uint64_t e = V.tb[static_cast<uint64_t>(hi_key >> V.shift) + 1];
        { uint64_t hi = e; while (i < hi) { const uint64_t mid = i + (hi - i) / 2; if (V.b[mid] < lo_key) i = mid + 1; else hi = mid; } }
        for (; i < e; ++i) { const KM y = V.b[i]; if (y > hi_key) break; entry(((y & himask) << (2 * lo_n)) | (y >> (2 * hi_n)), V.ib[i]); }
    }
    return c;
}
// list[s] = the s-th searched unitig, woff[s] = the windows of the searched unitigs before it. Count pass (out == nullptr): counts[g] = the candidates of window g.
// Write pass: the candidates of window g at offs[g] .. offs[g + 1], in the order the scans find them.
template <class KM>
__global__ void k_snp_scan(const char* __restrict__ pool, const uint64_t* __restrict__ seq_off, const uint32_t* __restrict__ list, const uint64_t* __restrict__ woff, uint64_t n_s, uint64_t n_win,
                           SnpViews<KM> V, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offs, uint64_t* __restrict__ out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; g < n_win; g += stride) {
        uint64_t at = 0, end = 0;
        if (out) { at = offs[g]; end = offs[g + 1]; if (at == end) continue; }
        const uint64_t s = snp_locate(woff, n_s, g), p = g - woff[s]; const uint32_t u = list[s]; bool bad = false;
        const KM x = snp_window<KM>(pool, seq_off[u] + p, V.k, &bad), rc = idx_revcomp(x, V.k);
        const uint64_t word0 = (static_cast<uint64_t>(u) << 32) | p;
        const uint32_t c = snp_scan(V, x, false, u, word0, out, at, end);
        const uint32_t c2 = snp_scan(V, rc, true, u, word0, out, at + c, end);
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

template <class KM>
int snp_candidates(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint32_t flags, uint64_t** cand_out, uint64_t* n_cand) {
    const bool trace = rtk_knob_index_trace();
    try {
        rtk_check(hipSetDevice(device), "hipSetDevice");
        const auto t0 = std::chrono::steady_clock::now();
        auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        // the windows of every unitig (the views) and of the searched ones (the queries)
        const uint64_t n_bases = seq_off[n_unitigs];
        std::vector<uint64_t> woff(n_unitigs + 1, 0), swoff(1, 0); std::vector<uint32_t> list;
        for (uint64_t u = 0; u < n_unitigs; ++u) {
            if (seq_off[u + 1] < seq_off[u] + static_cast<uint64_t>(k)) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a unitig of fewer than k characters");
            const uint64_t nw = seq_off[u + 1] - seq_off[u] - static_cast<uint64_t>(k) + 1;
            if (nw + static_cast<uint64_t>(k) > (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_candidates: a unitig of 2^32 characters or more");
            woff[u + 1] = woff[u] + nw;
            if (!searched || searched[u]) { list.push_back(static_cast<uint32_t>(u)); swoff.push_back(swoff.back() + nw); }
        }
        const uint64_t N = woff[n_unitigs], n_s = list.size(), W = swoff.back();
        if (N == 0 || W == 0) { // nothing to find, or nobody asks
            if (trace) fprintf(stderr, "rtk_index_snps: %llu windows of %llu unitigs searched against %llu k-mers, 0 candidates (0 kept); views 0.00 s, scan 0.00 s\n", static_cast<unsigned long long>(W), static_cast<unsigned long long>(n_s), static_cast<unsigned long long>(N));
            return RTK_OK;
        }
        // what the stage needs, before anything is allocated: text and offsets, three arrays of (key, id) -- two views and the sorts' other buffer --, the sort's
        // temporary, two prefix tables, the counts and their running sums; the candidates come on top once they are counted (checked again there)
        const int bits = 2 * k < 24 ? 2 * k : 24, shift = 2 * k - bits; const uint64_t n_pref = 1ull << bits;
        size_t tb_sort = 0, tb_scan = 0;
        { rocprim::double_buffer<KM> qk(nullptr, nullptr); rocprim::double_buffer<uint32_t> qv(nullptr, nullptr);
          rtk_check(rocprim::radix_sort_pairs(nullptr, tb_sort, qk, qv, static_cast<size_t>(N), 0, 2 * k), "rocprim::radix_sort_pairs (size)"); }
        SnpCountAt cnt_at; cnt_at.c = nullptr; cnt_at.n = W;
        { auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), cnt_at);
          rtk_check(rocprim::exclusive_scan(nullptr, tb_scan, it, static_cast<uint64_t*>(nullptr), 0ull, static_cast<size_t>(W + 1), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan (size)"); }
        const uint64_t need = n_bases + 16 * (n_unitigs + 1) + 3 * N * (sizeof(KM) + 4) + std::max<uint64_t>(tb_sort, tb_scan) + 2 * 8 * (n_pref + 1) + 4 * n_s + 8 * (n_s + 1) + 4 * W + 8 * (W + 1) + 4096;
        size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
        const uint64_t room = rtk_knob_index_snp_mem(static_cast<uint64_t>(fr));
        if (need > room) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: the two views of " + std::to_string(N) + " k-mers need " + std::to_string(need) + " bytes of device memory, " + std::to_string(room) + " are to be had (the key space is not partitioned)");

        DevBuf d_pool, d_off, d_woff, d_k[3], d_v[3], d_tmp, d_ta, d_tb, d_flag;
        d_pool.alloc(n_bases); d_off.alloc(8 * (n_unitigs + 1)); d_woff.alloc(8 * (n_unitigs + 1)); d_flag.alloc(8);
        for (int i = 0; i < 3; ++i) { d_k[i].alloc(sizeof(KM) * N); d_v[i].alloc(4 * N); }
        d_tmp.alloc(std::max<uint64_t>(tb_sort, tb_scan)); d_ta.alloc(8 * (n_pref + 1)); d_tb.alloc(8 * (n_pref + 1));
        rtk_check(hipMemcpy(d_pool.p, seq_pool, n_bases, hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemcpy(d_off.p, seq_off, 8 * (n_unitigs + 1), hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemcpy(d_woff.p, woff.data(), 8 * (n_unitigs + 1), hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemset(d_flag.p, 0, 8), "hipMemset");
        uint32_t* flag = static_cast<uint32_t*>(d_flag.p);
        const char* pool = static_cast<const char*>(d_pool.p); const uint64_t* off = static_cast<const uint64_t*>(d_off.p);
        hipLaunchKernelGGL(k_snp_keys<KM>, snp_grid(N), dim3(256), 0, 0, pool, off, static_cast<const uint64_t*>(d_woff.p), n_unitigs, N, k, static_cast<KM*>(d_k[0].p), static_cast<uint32_t*>(d_v[0].p), flag);
        rtk_check(hipGetLastError(), "kernel launch (k_snp_keys)");
        // view one: (d_k[0], d_k[1]) sorted; view two: its rotated copy in d_k[2] sorted with the buffer view one left free
        rocprim::double_buffer<KM> k1(static_cast<KM*>(d_k[0].p), static_cast<KM*>(d_k[1].p)); rocprim::double_buffer<uint32_t> v1(static_cast<uint32_t*>(d_v[0].p), static_cast<uint32_t*>(d_v[1].p));
        rtk_check(rocprim::radix_sort_pairs(d_tmp.p, tb_sort, k1, v1, static_cast<size_t>(N), 0, 2 * k), "rocprim::radix_sort_pairs");
        hipLaunchKernelGGL(k_snp_rot<KM>, snp_grid(N), dim3(256), 0, 0, static_cast<const KM*>(k1.current()), static_cast<const uint32_t*>(v1.current()), N, k, static_cast<KM*>(d_k[2].p), static_cast<uint32_t*>(d_v[2].p));
        rtk_check(hipGetLastError(), "kernel launch (k_snp_rot)");
        rocprim::double_buffer<KM> k2(static_cast<KM*>(d_k[2].p), k1.alternate()); rocprim::double_buffer<uint32_t> v2(static_cast<uint32_t*>(d_v[2].p), v1.alternate());
        rtk_check(rocprim::radix_sort_pairs(d_tmp.p, tb_sort, k2, v2, static_cast<size_t>(N), 0, 2 * k), "rocprim::radix_sort_pairs");
        hipLaunchKernelGGL(k_snp_table<KM>, snp_grid(N + 1), dim3(256), 0, 0, static_cast<const KM*>(k1.current()), N, shift, n_pref, static_cast<uint64_t*>(d_ta.p), flag);
        hipLaunchKernelGGL(k_snp_table<KM>, snp_grid(N + 1), dim3(256), 0, 0, static_cast<const KM*>(k2.current()), N, shift, n_pref, static_cast<uint64_t*>(d_tb.p), static_cast<uint32_t*>(nullptr));
        rtk_check(hipGetLastError(), "kernel launch (k_snp_table)"); rtk_check(hipDeviceSynchronize(), "views of the k-mers");
        uint32_t fl = 0; rtk_check(hipMemcpy(&fl, d_flag.p, 4, hipMemcpyDeviceToHost), "hipMemcpy");
        if (fl & 1u) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a unitig holds a character that is no base");
        if (fl & 2u) return rtk_fail(RTK_ERR_FORMAT, "rtk_index_snp_candidates: a k-mer occurs twice in the unitigs");
        const double t_views = since();
        // the buffer neither view ended up in is free again
        for (int i = 0; i < 3; ++i) if (d_k[i].p != k1.current() && d_k[i].p != k2.current()) { (void)hipFree(d_k[i].p); d_k[i].p = nullptr; }
        for (int i = 0; i < 3; ++i) if (d_v[i].p != v1.current() && d_v[i].p != v2.current()) { (void)hipFree(d_v[i].p); d_v[i].p = nullptr; }

        DevBuf d_list, d_swoff, d_cnt, d_offs;
        d_list.alloc(4 * n_s); d_swoff.alloc(8 * (n_s + 1)); d_cnt.alloc(4 * W); d_offs.alloc(8 * (W + 1));
        rtk_check(hipMemcpy(d_list.p, list.data(), 4 * n_s, hipMemcpyHostToDevice), "hipMemcpy");
        rtk_check(hipMemcpy(d_swoff.p, swoff.data(), 8 * (n_s + 1), hipMemcpyHostToDevice), "hipMemcpy");
        SnpViews<KM> V; V.a = k1.current(); V.ia = v1.current(); V.ta = static_cast<const uint64_t*>(d_ta.p); V.b = k2.current(); V.ib = v2.current(); V.tb = static_cast<const uint64_t*>(d_tb.p); V.k = k; V.shift = shift;
        hipLaunchKernelGGL(k_snp_scan<KM>, snp_grid(W), dim3(256), 0, 0, pool, off, static_cast<const uint32_t*>(d_list.p), static_cast<const uint64_t*>(d_swoff.p), n_s, W, V,
                           static_cast<uint32_t*>(d_cnt.p), static_cast<const uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr));
        rtk_check(hipGetLastError(), "kernel launch (k_snp_scan)");
        cnt_at.c = static_cast<const uint32_t*>(d_cnt.p);
        { auto it = rocprim::make_transform_iterator(rocprim::make_counting_iterator<uint64_t>(0), cnt_at);
          rtk_check(rocprim::exclusive_scan(d_tmp.p, tb_scan, it, static_cast<uint64_t*>(d_offs.p), 0ull, static_cast<size_t>(W + 1), rocprim::plus<uint64_t>()), "rocprim::exclusive_scan"); }
        rtk_check(hipDeviceSynchronize(), "candidates counted");
        uint64_t C = 0; rtk_check(hipMemcpy(&C, static_cast<uint64_t*>(d_offs.p) + W, 8, hipMemcpyDeviceToHost), "hipMemcpy");
        uint64_t R = C; uint64_t* res = static_cast<uint64_t*>(malloc(16 * (C ? C : 1)));
        if (!res) return rtk_fail(RTK_ERR_IO, "rtk_index_snp_candidates: out of host memory");
        std::unique_ptr<uint64_t, void (*)(void*)> res_guard(res, free);
        if (C) {
            // the candidates, their site keys and ids (both twice: the sort's other buffer), the kept indices, the order keys (twice)
            const uint64_t need_c = C * (16 + 2 * 16 + 2 * 4 + 8 + 2 * 16) + (64u << 20);
            rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
            const uint64_t room_c = rtk_knob_index_snp_mem(static_cast<uint64_t>(fr));
            if (need_c > room_c) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: " + std::to_string(C) + " candidates need " + std::to_string(need_c) + " bytes of device memory, " + std::to_string(room_c) + " are to be had");
            DevBuf d_cand, d_o[2], d_t2; d_cand.alloc(16 * C);
            hipLaunchKernelGGL(k_snp_scan<KM>, snp_grid(W), dim3(256), 0, 0, pool, off, static_cast<const uint32_t*>(d_list.p), static_cast<const uint64_t*>(d_swoff.p), n_s, W, V,
                               static_cast<uint32_t*>(nullptr), static_cast<const uint64_t*>(d_offs.p), static_cast<uint64_t*>(d_cand.p));
            rtk_check(hipGetLastError(), "kernel launch (k_snp_scan)");
            const uint64_t* raw = static_cast<const uint64_t*>(d_cand.p);
            if (flags & RTK_SNP_FIRST_PER_SITE) {
                DevBuf d_s[2], d_w[2], d_sel, d_nsel; d_s[0].alloc(16 * C); d_s[1].alloc(16 * C); d_w[0].alloc(4 * C); d_w[1].alloc(4 * C); d_sel.alloc(8 * C); d_nsel.alloc(8);
                hipLaunchKernelGGL(k_snp_site_keys, snp_grid(C), dim3(256), 0, 0, raw, C, static_cast<km2_t*>(d_s[0].p), static_cast<uint32_t*>(d_w[0].p));
                rtk_check(hipGetLastError(), "kernel launch (k_snp_site_keys)");
                rocprim::double_buffer<km2_t> sk(static_cast<km2_t*>(d_s[0].p), static_cast<km2_t*>(d_s[1].p)); rocprim::double_buffer<uint32_t> sw(static_cast<uint32_t*>(d_w[0].p), static_cast<uint32_t*>(d_w[1].p));
                size_t tb = 0; rtk_check(rocprim::radix_sort_pairs(nullptr, tb, sk, sw, static_cast<size_t>(C), 0, 98), "rocprim::radix_sort_pairs");
                d_t2.alloc(tb); rtk_check(rocprim::radix_sort_pairs(d_t2.p, tb, sk, sw, static_cast<size_t>(C), 0, 98), "rocprim::radix_sort_pairs");
                SnpSiteHead head; head.keys = sk.current();
                auto idx = rocprim::make_counting_iterator<uint64_t>(0); auto heads = rocprim::make_transform_iterator(idx, head);
                size_t sb = 0; rtk_check(rocprim::select(nullptr, sb, idx, heads, static_cast<uint64_t*>(d_sel.p), static_cast<unsigned long long*>(d_nsel.p), static_cast<size_t>(C)), "rocprim::select");
                d_t2.alloc(sb); rtk_check(rocprim::select(d_t2.p, sb, idx, heads, static_cast<uint64_t*>(d_sel.p), static_cast<unsigned long long*>(d_nsel.p), static_cast<size_t>(C)), "rocprim::select");
                rtk_check(hipDeviceSynchronize(), "first candidate of every site");
                unsigned long long ns = 0; rtk_check(hipMemcpy(&ns, d_nsel.p, 8, hipMemcpyDeviceToHost), "hipMemcpy");
                if (ns > C) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_snp_candidates: more candidates kept than found");
                R = ns; d_o[0].alloc(16 * R); d_o[1].alloc(16 * R);
                hipLaunchKernelGGL(k_snp_order_keys, snp_grid(R), dim3(256), 0, 0, raw, static_cast<const km2_t*>(sk.current()), static_cast<const uint32_t*>(sw.current()), static_cast<const uint64_t*>(d_sel.p), R, static_cast<km2_t*>(d_o[0].p));
                rtk_check(hipGetLastError(), "kernel launch (k_snp_order_keys)"); rtk_check(hipDeviceSynchronize(), "k_snp_order_keys");
            } else {
                d_o[0].alloc(16 * R); d_o[1].alloc(16 * R);
                hipLaunchKernelGGL(k_snp_order_keys, snp_grid(R), dim3(256), 0, 0, raw, static_cast<const km2_t*>(nullptr), static_cast<const uint32_t*>(nullptr), static_cast<const uint64_t*>(nullptr), R, static_cast<km2_t*>(d_o[0].p));
                rtk_check(hipGetLastError(), "kernel launch (k_snp_order_keys)");
            }
            rocprim::double_buffer<km2_t> ok(static_cast<km2_t*>(d_o[0].p), static_cast<km2_t*>(d_o[1].p));
            size_t tb = 0; rtk_check(rocprim::radix_sort_keys(nullptr, tb, ok, static_cast<size_t>(R), 0, 128), "rocprim::radix_sort_keys");
            d_t2.alloc(tb); rtk_check(rocprim::radix_sort_keys(d_t2.p, tb, ok, static_cast<size_t>(R), 0, 128), "rocprim::radix_sort_keys");
            rtk_check(hipDeviceSynchronize(), "candidates ordered");
            rtk_check(hipMemcpy(res, ok.current(), 16 * R, hipMemcpyDeviceToHost), "hipMemcpy");
            for (uint64_t i = 0; i < R; ++i) std::swap(res[2 * i], res[2 * i + 1]); // (a 128-bit key lies low word first)
        }
        *cand_out = res_guard.release(); *n_cand = R;
        if (trace) fprintf(stderr, "rtk_index_snps: %llu windows of %llu unitigs searched against %llu k-mers, %llu candidates (%llu kept); views %.2f s, scan %.2f s\n", static_cast<unsigned long long>(W), static_cast<unsigned long long>(n_s),
                           static_cast<unsigned long long>(N), static_cast<unsigned long long>(C), static_cast<unsigned long long>(R), t_views, since() - t_views);
    } catch (const std::exception& e) { return rtk_fail(RTK_ERR_DEVICE, std::string("rtk_index_snp_candidates: ") + e.what()); }
    return RTK_OK;
}
} // namespace

extern "C" int rtk_index_snp_candidates(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint32_t flags, uint64_t** cand, uint64_t* n_cand) {
    if (!cand || !n_cand || (n_unitigs && (!seq_pool || !seq_off))) return rtk_fail(RTK_ERR_ARG, "rtk_index_snp_candidates: null argument");
    if (k < 3 || k > 63 || !(k & 1)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_candidates: odd k <= 63 only");
    if (rtk_device_count() <= device || device < 0) return rtk_fail(RTK_ERR_NO_DEVICE, "rtk_index_snp_candidates: no such HIP device (no CPU fallback)");
    if (n_unitigs >= 0xFFFFFFFFull) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_candidates: more than 2^32 - 1 unitigs");
    *cand = nullptr; *n_cand = 0;
    if (n_unitigs == 0) return RTK_OK;
    return k <= 31 ? snp_candidates<uint64_t>(device, k, seq_pool, seq_off, n_unitigs, searched, flags, cand, n_cand) : snp_candidates<km2_t>(device, k, seq_pool, seq_off, n_unitigs, searched, flags, cand, n_cand);
}
