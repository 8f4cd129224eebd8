// rtk_index_colour_*: every read k-mer mapped onto its unitig -- colour events and coverage (k_col_map), behind an optional quality mask (k_col_mask).
// Colours and coverage of an index build (addCoverage, src/Graph.cpp:1561-1985) on the device. The caller -- the index tool, which owns the numbering of the reads
// (a pair keeps one id: name changes, or pair numbers of a sampled source) -- opens a job on the unitigs, feeds its reads chunk by chunk from any number of threads,
// and gets back the distinct (unitig, read id) events in sorted order and the k-mer coverage of every unitig.
//   begin  unitig u = seq_pool[seq_off[u] .. seq_off[u + 1]) (characters); the pool is packed to 2 bits and the k-mer table built in HBM (rtk_graph_tables.hip)
//   chunk  chars: sequences separated by '\n' (n_chars characters); read r starts at starts[r] and has the id ids[r]. At most RTK_COLOUR_CHUNK (64 MB) per call.
//   end    *events: n_events words unitig << 32 | id, ascending, distinct; *cov: n_unitigs counts. Freed with rtk_free. The job is gone afterwards (also on error).
#ifndef RTK_INDEX_COLOUR_H
#define RTK_INDEX_COLOUR_H
#include <string.h>
#include <cstdio>
#include <mutex>
#include <rocprim/rocprim.hpp>
#include "rtk_graph_tables.h"
#include "rtk_index_common.h"

namespace {
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
// Where a k-mer lies: its unitig (0xFFFFFFFF: not in the graph), its offset there, and whether the unitig spells it as given (fw) or its reverse complement. The slot's
// value holds all three (unitig << 32 | offset << 1 | the unitig spells the canonical form): nothing is searched a second time.
struct ColPlace { uint32_t u, off; bool fw; };
// a one-word k-mer: 16-byte slots {canonical k-mer, value}
__device__ __forceinline__ ColPlace col_place(const GraphView& g, uint64_t km, int k) {
    const uint64_t rc = idx_revcomp(km, k), can = km <= rc ? km : rc;
    const uint64_t* __restrict__ ht = g.ht; const uint64_t slots = g.ht_slots;
    uint64_t s = __umul64hi(idx_hash(can), slots);
    for (;;) {
        const uint64_t key = ht[2 * s];
        if (key == can) { const uint64_t v = ht[2 * s + 1]; ColPlace r; r.u = static_cast<uint32_t>(v >> 32); r.off = static_cast<uint32_t>((v & 0xFFFFFFFFull) >> 1); r.fw = ((v & 1ull) != 0) == (km <= rc); return r; }
        if (key == RTK_IDX_SENTINEL) { ColPlace r; r.u = 0xFFFFFFFFu; r.off = 0; r.fw = true; return r; }
        s = s + 1 == slots ? 0 : s + 1;
    }
}
// the unitig of a two-word k-mer: the slots keep a fingerprint of the canonical k-mer, a match is confirmed against the unitig's bases
// (rtk_find_kmer_wide without the presence filters, which the index build's table does not have)
__device__ __forceinline__ ColPlace col_place(const GraphView& g, km2_t km, int k) {
    const RtkKm fw = idx_words(km), rc = rtk_km_revcomp(fw, k), can = rtk_km_less(fw, rc) ? fw : rc;
    const uint64_t fp = rtk_km_fingerprint(can); const uint64_t* __restrict__ ht = g.ht; const uint64_t slots = g.ht_slots;
    for (uint64_t s = rtk_ht_slot(rtk_km_hash(can), slots);; s = rtk_ht_next(s, slots)) {
        const uint64_t key = ht[2 * s];
        if (key == fp) {
            const uint64_t v = ht[2 * s + 1]; const uint32_t u = static_cast<uint32_t>(v >> 32);
            const RtkKm urc = rtk_km_rc_of_unitig(g, g.uoff[u] + ((v & 0xFFFFFFFFull) >> 1), k);
            const bool same = rtk_km_eq(urc, rc); // (the reverse complement of the unitig's window is that of the k-mer: the unitig spells it as given)
            if (same || rtk_km_eq(urc, fw)) { ColPlace r; r.u = u; r.off = static_cast<uint32_t>((v & 0xFFFFFFFFull) >> 1); r.fw = same; return r; }
        }
        if (key == RTK_EMPTY_KEY) { ColPlace r; r.u = 0xFFFFFFFFu; r.off = 0; r.fw = true; return r; }
    }
}
// the unitig alone
template <class KM> __device__ __forceinline__ uint32_t col_find(const GraphView& g, KM km, int k) { return col_place(g, km, k).u; }
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
uint64_t* sort_unique_events(uint64_t* cur, uint64_t* other, uint64_t n, DevArr<char>& tmp, uint64_t* n_out) {
    rocprim::double_buffer<uint64_t> db(cur, other);
    prim(tmp, "rocprim::radix_sort_keys", [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, db, n, 0, 64); });
    uint64_t* sorted = db.current(); uint64_t* out = db.alternate();
    DevArr<unsigned long long> d_n; d_n.alloc(1);
    prim(tmp, "rocprim::unique", [&](void* t, size_t& b) { return rocprim::unique(t, b, sorted, out, d_n.p, n); });
    *n_out = read_word(d_n.p, "events sorted"); return out;
}

// The unitigs of a job in HBM: packed to 2 bits, their offsets, and their k-mer table (rtk_graph_tables.hip); g holds the fields the mapping kernels read
// (k_col_map here, k_cover_map of rtk_index_cover.h).
struct DeviceUnitigs : Owner {
    DevArr<uint64_t> useq, uoff, ht; uint64_t slots = 0; GraphView g;
    void build(int k, uint32_t n_unitigs, const char* seq_pool, const uint64_t* seq_off) {
        const uint64_t n_bases = seq_off[n_unitigs], n_kmers = n_bases - n_unitigs * static_cast<uint64_t>(k - 1), n_words = (n_bases + 31) / 32;
        { DevArr<char> d_pool; d_pool.alloc(n_bases); rtk_check(hipMemcpy(d_pool.p, seq_pool, n_bases, hipMemcpyHostToDevice), "hipMemcpy");
          useq.alloc(n_words + 2); rtk_check(hipMemset(useq.p, 0, 8 * (n_words + 2)), "hipMemset");
          launch("k_col_pack", k_col_pack, dim3(4096), 0, d_pool.p, n_bases, useq.p, n_words); rtk_check(hipDeviceSynchronize(), "k_col_pack"); }
        uoff.alloc(n_unitigs + 1ull); rtk_check(hipMemcpy(uoff.p, seq_off, 8 * (n_unitigs + 1ull), hipMemcpyHostToDevice), "hipMemcpy");
        void* table = nullptr; rtk::device_kmer_table(useq.p, uoff.p, n_unitigs, n_bases, n_kmers, k, &table, &slots);
        ht.adopt(table);
        memset(&g, 0, sizeof(g)); g.k = k; g.n_unitigs = n_unitigs; g.ht_slots = slots; g.ht = ht.p; g.useq = useq.p; g.uoff = uoff.p;
    }
};

struct ColourJob {
    int device = 0, k = 31; uint32_t n_unitigs = 0; DeviceUnitigs du; GraphView& g = du.g; // g: the k-mer table and the packed unitigs (the only fields k_col_map reads)
    DevArr<uint64_t> events, alt; DevArr<unsigned long long> cov, top; DevArr<char> tmp;
    uint64_t cap = 0, n_events = 0; // n_events: sorted, distinct events at the front of `events`
    uint64_t n_ids = 0;                        // largest id fed + 1 (after rtk_index_colour_merge: the number of merged ids): the size of the id tables of the subsampling
    uint64_t merge_classes_above_one = 0, merge_largest = 0; // what the last rtk_index_colour_merge found
    DevArr<char> d_chars[2]; DevArr<uint64_t> d_starts[2]; DevArr<uint32_t> d_ids[2]; PinArr<char> h_chars[2]; PinArr<uint64_t> h_starts[2]; PinArr<uint32_t> h_ids[2]; uint64_t chunk_cap = 0, reads_cap = 0;
    DevArr<unsigned char> d_quals[2]; PinArr<unsigned char> h_quals[2]; bool has_quals = false; // one chunk of quality bytes per slot, there from the job's first chunk with qualities on (rtk_index_colour_chunk_q)
    Stream st[2]; int slot = 0;
    std::mutex m; uint64_t bases = 0, chunks = 0, compactions = 0; double t_table = 0.0;
    StageClock clk;

    uint64_t events_on_device() { return read_word(top.p, "hipDeviceSynchronize"); }
    void set_events(const uint64_t* at, uint64_t n) { // the job's events from now on: n sorted distinct words at `at` (in `events` or in `alt`)
        if (at != events.p) rtk_check(hipMemcpy(events.p, at, 8 * n, hipMemcpyDeviceToDevice), "hipMemcpy");
        n_events = n; rtk_check(hipMemcpy(top.p, &n, 8, hipMemcpyHostToDevice), "hipMemcpy");
    }
    // the events so far sorted, the distinct ones kept (both streams idle)
    void compact() {
        const uint64_t n = events_on_device();
        if (n > cap) throw std::runtime_error("more (unitig, read) events than the device buffer holds between two compactions (RTK_INDEX_EVENTS: number of events to make room for)");
        if (n == n_events) return;
        ++compactions;
        uint64_t nu = 0; const uint64_t* res = sort_unique_events(events.p, alt.p, n, tmp, &nu);
        set_events(res, nu);
    }

    // the unitigs packed to 2 bits, their k-mer table, the coverage counters
    void build_graph(const char* seq_pool, const uint64_t* seq_off) {
        du.build(k, n_unitigs, seq_pool, seq_off);
        cov.alloc(n_unitigs); rtk_check(hipMemset(cov.p, 0, 8ull * n_unitigs), "hipMemset");
        top.alloc(1); rtk_check(hipMemset(top.p, 0, 8), "hipMemset");
    }
    // two slots of a chunk each (pinned and device, a stream each) and, from what is left, the events
    void alloc_buffers() {
        chunk_cap = 64ull << 20; reads_cap = chunk_cap / 16; // (a read of fewer than 15 characters per 16 bytes of chunk: the caller splits such chunks)
        for (int i = 0; i < 2; ++i) {
            d_chars[i].alloc(chunk_cap); d_starts[i].alloc(reads_cap); d_ids[i].alloc(reads_cap);
            h_chars[i].alloc(chunk_cap); h_starts[i].alloc(reads_cap); h_ids[i].alloc(reads_cap);
            st[i].create();
        }
        size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
        cap = static_cast<uint64_t>(fr) / 10 * 6 / 16; // 60 % of what is left for the events and their sort buffer
        cap = rtk_knob_index_events(cap);
        if (cap < 1024) cap = 1024;
        events.alloc(cap); alt.alloc(cap);
    }
    void begin(int device_, int k_, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs_) {
        device = device_; k = k_; n_unitigs = static_cast<uint32_t>(n_unitigs_);
        build_graph(seq_pool, seq_off);
        alloc_buffers();
        t_table = clk.since();
    }

    // room for a chunk's events (at most one per position): sort and keep the distinct ones when the buffer is half full
    void make_room() {
        if (chunks && ((chunks & 7u) == 0 || cap < (1ull << 30))) { // (looked at every 8th chunk: reading the counter waits for the device)
            if (events_on_device() > cap / 2) compact();
        }
    }
    // the base-confidence mask of slot sl's characters, on its stream (idle since the caller's synchronisation: its pinned quality bytes are free to be written)
    void mask(int sl, const unsigned char* quals, unsigned char q_min, uint64_t n_chars) {
        if (!has_quals) { for (int i = 0; i < 2; ++i) { d_quals[i].alloc(chunk_cap); h_quals[i].alloc(chunk_cap); } has_quals = true; }
        memcpy(h_quals[sl].p, quals, n_chars);
        rtk_check(hipMemcpyAsync(d_quals[sl].p, h_quals[sl].p, n_chars, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        launch("k_col_mask", k_col_mask, dim3(256), st[sl], d_chars[sl].p, d_quals[sl].p, n_chars, q_min);
    }
    template <class KM> void map(int sl, uint64_t n_chars, uint32_t n_reads) {
        launch("k_col_map", k_col_map<KM>, dim3(4096), st[sl], d_chars[sl].p, n_chars, k, d_starts[sl].p, d_ids[sl].p, n_reads, g, cov.p, events.p, top.p, cap);
    }
    // one chunk; quals == nullptr: no quality bytes, nothing of the masking step runs
    void chunk(const char* chars, const unsigned char* quals, unsigned char q_min, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads) {
        make_room();
        { uint32_t mx = 0; for (uint32_t r = 0; r < n_reads; ++r) mx = ids[r] > mx ? ids[r] : mx; n_ids = std::max<uint64_t>(n_ids, static_cast<uint64_t>(mx) + 1); }
        const int sl = slot; slot ^= 1;
        rtk_check(hipStreamSynchronize(st[sl]), "hipStreamSynchronize");
        memcpy(h_chars[sl].p, chars, n_chars); memcpy(h_starts[sl].p, starts, 8ull * n_reads); memcpy(h_ids[sl].p, ids, 4ull * n_reads);
        rtk_check(hipMemcpyAsync(d_chars[sl].p, h_chars[sl].p, n_chars, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_starts[sl].p, h_starts[sl].p, 8ull * n_reads, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        rtk_check(hipMemcpyAsync(d_ids[sl].p, h_ids[sl].p, 4ull * n_reads, hipMemcpyHostToDevice, st[sl]), "hipMemcpyAsync");
        if (quals) mask(sl, quals, q_min, n_chars);
        by_key_type(k, [&](auto km) { map<decltype(km)>(sl, n_chars, n_reads); return 0; });
        bases += n_chars; ++chunks;
    }

    // the coverage of every unitig for the caller; false: out of host memory
    bool coverage(HostOut<uint64_t>& cv) {
        if (!cv.alloc(n_unitigs)) return false;
        rtk_check(hipMemcpy(cv.p, cov.p, 8ull * n_unitigs, hipMemcpyDeviceToHost), "hipMemcpy");
        return true;
    }
    // n events at `at` (device) for the caller; false: out of host memory
    bool events_out(const uint64_t* at, uint64_t n, HostOut<uint64_t>& ev) {
        if (!ev.alloc(n)) return false;
        if (n) rtk_check(hipMemcpy(ev.p, at, 8 * n, hipMemcpyDeviceToHost), "hipMemcpy");
        return true;
    }
    // the trace line of either end; `thinned`: what the subsampling says between the events and the times
    void trace_end(const std::string& thinned) {
        if (clk.trace) fprintf(stderr, "rtk_index_colour: %llu characters in %llu chunks -> %llu distinct (unitig, read) events (sorted and thinned out %llu times)%s; table %.2f s, all %.2f s\n", static_cast<unsigned long long>(bases),
                               static_cast<unsigned long long>(chunks), static_cast<unsigned long long>(n_events), static_cast<unsigned long long>(compactions), thinned.c_str(), t_table, clk.since());
    }
};
} // namespace
#endif
