// rtk_index_count_kmers: the canonical k-mers of the reads seen >= min_count times. Every read position spells its k-mer (one lane per position, the window packed
// 2 bits per base without branches), the k-mers of a pass are radix-sorted (rocPRIM) and the first element of every run of >= min_count equal keys is kept.
// HBM-bound: 1 byte read + 8 (16) bytes written per base, then the sort. A pass = one hash partition of the k-mer space; the sorted partitions are merged on the host.
#ifndef RTK_INDEX_COUNT_H
#define RTK_INDEX_COUNT_H
#include <string.h>
#include <unistd.h>
#include <cstdio>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "../common/sequence_chunks.hpp"
#include "../common/sorted_runs.hpp"
#include "rtk_index_common.h"

namespace {
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

// bytes of the inputs (a sampled source: of the text it stands for); false: *err
// *fasta_kmers: of those bytes, the ones of FASTA files (records start with '>': a unitig file handed in as the graph), left OUT of *total and given as the k-mers
// they stand for: nearly every byte of FASTA text starts a window, and gzip packs such text to a quarter (2 bits a base), where half of a FASTQ file's bytes are bases.
inline bool count_input_bytes(const std::vector<std::string>& files, uint64_t* total, uint64_t* fasta_kmers, std::string* err) {
    *total = 0; *fasta_kmers = 0;
    for (size_t f = 0; f < files.size(); ++f) {
        if (rtk::SampleSource::is_spec(files[f])) { std::shared_ptr<rtk::SampleSource> ss = rtk::SampleSource::get(files[f], err); if (!ss) return false; *total += 2 * ss->n_bases(); continue; }
        FILE* fp = fopen(files[f].c_str(), "rb"); if (!fp) { *err = "cannot open " + files[f]; return false; }
        unsigned char m[2] = {0, 0}; const size_t n_m = fread(m, 1, 2, fp);
        fseek(fp, 0, SEEK_END); const uint64_t bytes = static_cast<uint64_t>(ftell(fp)); fclose(fp);
        const bool gz = n_m == 2 && m[0] == 0x1f && m[1] == 0x8b;
        char first = n_m ? static_cast<char>(m[0]) : 0;
        if (gz) { gzFile g = gzopen(files[f].c_str(), "rb"); if (g) { if (gzread(g, &first, 1) != 1) first = 0; gzclose(g); } }
        if (first == '>') *fasta_kmers += gz ? 4 * bytes : bytes; else *total += bytes;
    }
    return true;
}
// host memory to be had: what sysconf reports, or what is left under the control group's limit, if there is one (a container's limit is not what sysconf reports)
inline uint64_t count_host_memory() {
    uint64_t avail = static_cast<uint64_t>(sysconf(_SC_AVPHYS_PAGES)) * static_cast<uint64_t>(sysconf(_SC_PAGE_SIZE));
    unsigned long long lim = 0, cur = 0; bool have = false;
    if (FILE* f1 = fopen("/sys/fs/cgroup/memory.max", "r")) { have = fscanf(f1, "%llu", &lim) == 1; fclose(f1); if (have) { if (FILE* f2 = fopen("/sys/fs/cgroup/memory.current", "r")) { if (fscanf(f2, "%llu", &cur) != 1) cur = 0; fclose(f2); } } }
    if (have && lim > cur && lim - cur < avail) avail = lim - cur;
    return avail;
}

// the device side of one attempt: two slots of text (pinned and device, a stream each), the keys of a partition and the sort's other buffer
template <class KM> struct CountPass {
    int k; uint64_t cap, piece_max; // cap: keys there is room for; piece_max: characters per copy
    DevArr<KM> keys, alt; DevArr<unsigned long long> top, n_sel; DevArr<char> chars[2], tmp; PinArr<char> h_chars[2]; Stream st[2]; int slot = 0;
    CountPass(int k_, uint64_t cap_, uint64_t piece_max_) : k(k_), cap(cap_), piece_max(piece_max_) {
        keys.alloc(cap); alt.alloc(cap); top.alloc(1); n_sel.alloc(1);
        for (int i = 0; i < 2; ++i) chars[i].alloc(piece_max);
        for (int i = 0; i < 2; ++i) h_chars[i].alloc(piece_max);
        for (int i = 0; i < 2; ++i) st[i].create();
    }
    void begin_partition() { rtk_check(hipMemset(top.p, 0, 8), "hipMemset"); slot = 0; }
    // one chunk: pinned copy, H2D and the k-mer kernel on the slot's stream (the other slot's work overlaps the next parse)
    void feed(const char* text, size_t n, uint32_t part, uint32_t n_part) {
        for (size_t off = 0; off < n;) {
            const size_t piece = std::min<size_t>(n - off, piece_max);
            rtk_check(hipStreamSynchronize(st[slot]), "hipStreamSynchronize");
            memcpy(h_chars[slot].p, text + off, piece);
            rtk_check(hipMemcpyAsync(chars[slot].p, h_chars[slot].p, piece, hipMemcpyHostToDevice, st[slot]), "hipMemcpyAsync");
            launch("k_index_kmers", k_index_kmers<KM>, dim3(4096), st[slot], chars[slot].p, piece, k, part, n_part, keys.p, top.p, cap);
            slot ^= 1; off += (off + piece < n) ? piece - static_cast<size_t>(k - 1) : piece; // a cut inside a sequence: the next piece starts k - 1 characters back, so that every window is seen once
        }
    }
    uint64_t n_keys() { return read_word(top.p, "hipDeviceSynchronize"); }
    // the n keys sorted (two-word keys: bits [0, 2k) of the 128-bit value); trace: waited for
    rocprim::double_buffer<KM> sort(uint64_t n, const StageClock& clk) {
        rocprim::double_buffer<KM> db(keys.p, alt.p);
        prim(tmp, "rocprim::radix_sort_keys", [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, db, n, 0, 2 * k); });
        if (clk.trace) { rtk_check(hipDeviceSynchronize(), "radix sort"); fprintf(stderr, "rtk_index_count_kmers:   sorted at %.1f s\n", clk.since()); }
        return db;
    }
    // the first key of every run of >= min_count among the n sorted keys, into the other buffer: how many
    uint64_t select_solid(rocprim::double_buffer<KM>& db, uint64_t n, uint32_t min_count) {
        SolidHead<KM> pred; pred.keys = db.current(); pred.n = n; pred.min_count = min_count;
        KeyAt<KM> at; at.keys = db.current();
        auto idx = rocprim::make_counting_iterator<uint64_t>(0);
        auto vals = rocprim::make_transform_iterator(idx, at);
        auto flags = rocprim::make_transform_iterator(idx, pred); // select with a flag iterator: the flag of element i is the predicate on its index
        prim(tmp, "rocprim::select", [&](void* t, size_t& b) { return rocprim::select(t, b, vals, flags, db.alternate(), n_sel.p, n); });
        return read_word(n_sel.p, "hipDeviceSynchronize");
    }
};

// KM: uint64_t (k <= 31) or km2_t (33 <= k <= 63); *solid_out holds n_solid keys of sizeof(KM) bytes. Throws; an I/O error is returned.
template <class KM> int count_kmers(int k, const char* const* files, int n_files, uint32_t min_count, int n_threads, uint64_t** solid_out, uint64_t* n_solid) {
    const std::vector<std::string> fl(files, files + n_files);
    std::string err;
    // passes: the k-mers of one pass (one hash partition of the k-mer space) must fit twice (radix sort) next to what else lives on the device
    uint64_t total_bytes = 0, fasta_kmers = 0;
    if (!count_input_bytes(fl, &total_bytes, &fasta_kmers, &err)) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + err);
    size_t fr = 0, tot = 0; rtk_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
    if (rtk_knob_index_trace()) fprintf(stderr, "rtk_index_count_kmers: inputs sized (%.1f GB), %.1f GB of device memory free\n", (total_bytes + fasta_kmers) / 1e9, fr / 1e9);
    const uint64_t est_kmers = total_bytes / 2 + fasta_kmers + (1u << 20); // FASTQ: half of the bytes are bases (gzip FASTQ: a multiple of it; the capacity test below catches that); FASTA: see count_input_bytes
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
    const StageClock clk;
    { const uint64_t avail = count_host_memory();
      const int kt = rtk_knob_index_keep_text(); keep_text = kt >= 0 ? kt != 0 : (est_kmers + est_kmers / 8 < avail / 2); // (the caller's own tables come on top of it later: half of what is left, no more)
      if (clk.trace) fprintf(stderr, "rtk_index_count_kmers: %.1f GB of host memory to be had, text %s\n", avail / 1e9, keep_text ? "kept across partitions" : "read again for every partition"); }
    for (bool done = false; !done;) {
        done = true; solid.clear(); run_start.clear(); if (!kept_complete) kept.clear(); // (a restart with more partitions keeps the text of the complete first pass)
        CountPass<KM> pass(k, n_part == 1 ? std::min<uint64_t>(cap, est_kmers + est_kmers / 8) : cap, chunk_bytes + chunk_slack);
        for (uint32_t part = 0; part < n_part && done; ++part) {
            pass.begin_partition();
            uint64_t n_sunk = 0, b_sunk = 0;
            if (clk.trace) fprintf(stderr, "rtk_index_count_kmers: partition %u of %u starts at %.1f s (room for %llu k-mers)\n", part + 1, n_part, clk.since(), static_cast<unsigned long long>(pass.cap));
            auto sink = [&](const char* chars, size_t n) {
                if (clk.trace && (++n_sunk & 31u) == 0) fprintf(stderr, "rtk_index_count_kmers:   %llu chunks, %.1f GB of text at %.1f s\n", static_cast<unsigned long long>(n_sunk), b_sunk / 1e9, clk.since());
                b_sunk += n;
                pass.feed(chars, n, part, n_part);
            };
            if (kept_complete) { for (size_t c = 0; c < kept.size(); ++c) sink(kept[c].data(), kept[c].size()); }
            else if (keep_text && n_part > 1) {
                auto sink_keep = [&](const char* chars, size_t n) { kept.push_back(std::string(chars, n)); sink(chars, n); };
                if (!rtk::for_each_sequence_chunk(fl, n_threads, chunk_bytes, sink_keep, &err)) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + err);
                kept_complete = true;
            }
            else if (!rtk::for_each_sequence_chunk(fl, n_threads, chunk_bytes, sink, &err)) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: " + err);
            const uint64_t n_keys = pass.n_keys();
            if (n_keys > pass.cap) { // more k-mers than estimated: more partitions, again
                n_part = static_cast<uint32_t>((n_keys * static_cast<uint64_t>(n_part) + cap - 1) / cap) + 1; done = false; break;
            }
            if (n_keys == 0) continue;
            if (clk.trace) fprintf(stderr, "rtk_index_count_kmers:   %llu k-mers on the device at %.1f s; sorting\n", static_cast<unsigned long long>(n_keys), clk.since());
            rocprim::double_buffer<KM> db = pass.sort(n_keys, clk);
            const uint64_t n_sel = pass.select_solid(db, n_keys, min_count);
            const size_t old = solid.size(); solid.resize(old + n_sel); run_start.push_back(old);
            if (clk.trace) fprintf(stderr, "rtk_index_count_kmers: partition %u of %u: %llu k-mers, %llu solid (at %.1f s%s)\n", part + 1, n_part, static_cast<unsigned long long>(n_keys), static_cast<unsigned long long>(n_sel), clk.since(), kept_complete ? ", text kept in host memory" : "");
            if (n_sel) rtk_check(hipMemcpy(solid.data() + old, db.alternate(), sizeof(KM) * n_sel, hipMemcpyDeviceToHost), "hipMemcpy");
            pass.tmp.release();
        }
    }
    HostOut<KM> out;
    if (!out.alloc(solid.size())) return rtk_fail(RTK_ERR_IO, "rtk_index_count_kmers: out of host memory");
    rtk::merge_sorted_runs<KM>(solid, run_start, k, n_threads, out.p); // the partitions are sorted each and a k-mer lives in one of them
    if (clk.trace) fprintf(stderr, "rtk_index_count_kmers: %zu solid k-mers from %u partition(s) in %.1f s\n", solid.size(), n_part, clk.since());
    *solid_out = reinterpret_cast<uint64_t*>(out.release()); *n_solid = solid.size();
    return RTK_OK;
}
} // namespace
#endif
