// GPU side of the index build (reference: `Ratatosk index`, src/Ratatosk.cpp:1066-1067 Bifrost build + src/Graph.cpp:1561 addCoverage).
// The reference builds its graph with Bifrost on the CPU; the data-parallel steps of an index build are done here on the device, behind the C ABI
// (include/ratatosk_hip.h), for the index tool (csrc/tools/build_index.cpp --gpu). This file holds the entries; every stage -- its rule and bounds, its kernels and
// the device function of the entry -- has a header of its own, and what they share is in rtk_index_common.h:
//   rtk_index_count_kmers   (rtk_index_count.h)     canonical k-mers of the reads seen >= min_count times (k_index_kmers, rocPRIM sort and select)
//   rtk_index_unitigs       (rtk_index_unitigs.h)   the chains of the compacted graph walked, numbered and spelt (k_ut_*)
//   rtk_index_colour_*      (rtk_index_colour.h)    every read k-mer mapped onto its unitig: colour events and coverage (k_col_map); with rtk_index_colour_chunk_q the
//                                                   bases of a chunk whose quality is below a threshold turned into N ahead of the mapping (k_col_mask)
//     ..._end_subsampled    (rtk_index_subsample.h) the events thinned out by coverage and their ids renumbered before they leave the device (k_sub_*)
//     ..._merge             (rtk_index_merge.h)     the ids of read pairs on the same unitigs merged in place before that (k_merge_*)
//   rtk_index_snp_candidates (rtk_index_snps.h)     the candidate search of the SNP annotations: the graph k-mers one substitution away from every window of the
//                                                   searched unitigs (k_snp_*), in passes over partitions of the key space when the views of all
//                                                   windows do not fit; rtk_index_snp_plan: what it would do, from the offsets alone
//   rtk_index_cover_*       (rtk_index_cover.h)     the text of other sequences (the k2 unitigs) walked over the k-mer table: where it crosses an edge recorded as
//                                                   shared by too few colours (k_cover_map); the crossings in the order of the file for the caller's serial walk
//   rtk_index_pair_ids      (rtk_index_pairs.h)     the ids of the read pairs by name: the rank of every record's name hash by first appearance (k_pair_*), in passes
//                                                   over equal ranges of the hash space when sort buffers for all records do not fit; rtk_index_pair_plan: what it would do
// Every step serves one-word k-mers (k <= 31, key type uint64_t) and two-word k-mers (33 <= k <= 63, key type unsigned __int128: the 2k-bit code,
// first base in the most significant bits; in memory the low word first). Own translation unit: rocPRIM's templates.
// An entry is: the checks of its arguments, entry(...) -- the device set, what is thrown turned into the entry's error --, one call into the stage.
#include <memory>
#include <mutex>
#include <string>

#include "rtk_index_common.h"
#include "rtk_index_count.h"
#include "rtk_index_unitigs.h"
#include "rtk_index_colour.h"
#include "rtk_index_subsample.h"
#include "rtk_index_merge.h"
#include "rtk_index_snps.h"
#include "rtk_index_cover.h"
#include "rtk_index_pairs.h"

extern "C" int rtk_index_count_kmers(int device, int k, const char* const* files, int n_files, uint32_t min_count, int n_threads, uint64_t** solid_out, uint64_t* n_solid) {
    if (!files || n_files <= 0 || !solid_out || !n_solid) return rtk_fail(RTK_ERR_ARG, "rtk_index_count_kmers: null argument");
    if (const int rc = check_k_and_device("rtk_index_count_kmers", k, device)) return rc;
    if (min_count < 1) min_count = 1;
    return entry("rtk_index_count_kmers", device, [&]() { return by_key_type(k, [&](auto km) { return count_kmers<decltype(km)>(k, files, n_files, min_count, n_threads, solid_out, n_solid); }); });
}

extern "C" int rtk_index_unitigs(int device, int k, const uint64_t* solid, uint64_t n_solid, char** seq_pool, uint64_t** seq_off, uint64_t** seeds, uint64_t* n_unitigs, uint64_t** left, uint64_t* n_left) {
    if (!solid || !seq_pool || !seq_off || !seeds || !n_unitigs || !left || !n_left) return rtk_fail(RTK_ERR_ARG, "rtk_index_unitigs: null argument");
    if (const int rc = check_k_and_device("rtk_index_unitigs", k, device)) return rc;
    if (n_solid >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_unitigs: more than 2^32 solid k-mers");
    *seq_pool = nullptr; *seq_off = nullptr; *seeds = nullptr; *left = nullptr; *n_unitigs = 0; *n_left = 0;
    return entry("rtk_index_unitigs", device, [&]() { return by_key_type(k, [&](auto km) { // (two words per two-word k-mer, low word first)
        return unitigs<decltype(km)>(k, reinterpret_cast<const decltype(km)*>(solid), n_solid, seq_pool, seq_off, seeds, n_unitigs, left, n_left); }); });
}

extern "C" int rtk_index_colour_begin(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, void** job_out) {
    if (!seq_pool || !seq_off || !job_out || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_begin: null argument");
    if (const int rc = check_k_and_device("rtk_index_colour_begin", k, device)) return rc;
    if (n_unitigs >= 0xFFFFFFFFull) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_colour_begin: more than 2^32 - 1 unitigs");
    *job_out = nullptr;
    return entry("rtk_index_colour_begin", device, [&]() { std::unique_ptr<ColourJob> J(new ColourJob()); J->begin(device, k, seq_pool, seq_off, n_unitigs); *job_out = J.release(); return RTK_OK; });
}

// one chunk of either entry; quals == nullptr: no quality bytes, nothing of the masking step runs
static int colour_chunk(const char* name, void* job, const char* chars, const unsigned char* quals, unsigned char q_min, uint64_t n_chars, const uint64_t* starts, const uint32_t* ids, uint32_t n_reads) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !chars || !starts || !ids) return rtk_fail(RTK_ERR_ARG, std::string(name) + ": null argument");
    if (n_reads == 0 || n_chars == 0) return RTK_OK;
    if (n_chars > J->chunk_cap || n_reads > J->reads_cap) return rtk_fail(RTK_ERR_ARG, std::string(name) + ": chunk larger than 64 MB of characters / 4 M reads");
    std::lock_guard<std::mutex> lk(J->m);
    return entry(name, J->device, [&]() { J->chunk(chars, quals, q_min, n_chars, starts, ids, n_reads); return RTK_OK; });
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
    return entry("rtk_index_colour_end", J->device, [&]() {
        J->compact();
        HostOut<uint64_t> ev, cv;
        if (!J->events_out(J->events.p, J->n_events, ev) || !J->coverage(cv)) return rtk_fail(RTK_ERR_IO, "rtk_index_colour_end: out of host memory");
        *events = ev.release(); *n_events = J->n_events; *cov = cv.release();
        J->trace_end("");
        return RTK_OK;
    });
}

// The coverage of every unitig once all chunks are mapped (and the events sorted, the distinct ones kept); the job stays alive for rtk_index_colour_end or
// rtk_index_colour_end_subsampled: the caller needs the coverage to work out the bins before the events can be thinned.
extern "C" int rtk_index_colour_cov(void* job, uint64_t** cov) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !cov) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_cov: null argument");
    *cov = nullptr;
    std::lock_guard<std::mutex> lk(J->m);
    return entry("rtk_index_colour_cov", J->device, [&]() {
        J->compact();
        HostOut<uint64_t> cv;
        if (!J->coverage(cv)) return rtk_fail(RTK_ERR_IO, "rtk_index_colour_cov: out of host memory");
        *cov = cv.release();
        return RTK_OK;
    });
}

// rtk_index_colour_end with the events thinned out by coverage and renumbered on the device (the rule: rtk_index_subsample.h); only the kept events are copied to the host.
extern "C" int rtk_index_colour_end_subsampled(void* job, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled, uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed,
                                               uint64_t** events, uint64_t* n_events, uint64_t* n_events_before, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    std::unique_ptr<ColourJob> J(static_cast<ColourJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_end_subsampled: null job");
    if (!events || !n_events || !n_events_before || !n_ids_before || !n_ids_after) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_end_subsampled: null argument");
    *events = nullptr; *n_events = 0;
    const SubsampleRule rule = {bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate, seed};
    if (const char* bad = subsample_rule_bad(rule)) return rtk_fail(RTK_ERR_ARG, std::string("rtk_index_colour_end_subsampled: ") + bad);
    return entry("rtk_index_colour_end_subsampled", J->device, [&]() {
        J->compact();
        const StageClock sub;
        const SubsampleResult r = subsample_events_device(J->events.p, J->n_events, J->alt.p, J->n_unitigs, J->n_ids, rule);
        HostOut<uint64_t> ev;
        if (!J->events_out(J->alt.p, r.n_out, ev)) return rtk_fail(RTK_ERR_IO, "rtk_index_colour_end_subsampled: out of host memory");
        *events = ev.release(); *n_events = r.n_out; *n_events_before = J->n_events; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
        char thinned[96]; snprintf(thinned, sizeof(thinned), ", %llu left after subsampling (%.3f s)", static_cast<unsigned long long>(r.n_out), sub.since());
        J->trace_end(thinned);
        return RTK_OK;
    });
}

// Stage entry for tests: the device function behind rtk_index_colour_end_subsampled on events of the caller (host arrays; ascending, distinct, unitigs < n_unitigs);
// events_out has room for n_events words.
extern "C" int rtk_index_subsample_events(int device, const uint64_t* events, uint64_t n_events, uint32_t n_unitigs, const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled,
                                          uint32_t n_bins, uint32_t mcv, double rate, uint64_t seed, uint64_t* events_out, uint64_t* n_out, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    if ((!events && n_events) || (!events_out && n_events) || !n_out || !n_ids_before || !n_ids_after || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: null argument");
    const SubsampleRule rule = {bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, mcv, rate, seed};
    if (const char* bad = subsample_rule_bad(rule)) return rtk_fail(RTK_ERR_ARG, std::string("rtk_index_subsample_events: ") + bad);
    if (const int rc = check_device("rtk_index_subsample_events", device)) return rc;
    uint64_t n_ids = 0;
    if (const int rc = check_host_events("rtk_index_subsample_events", events, n_events, n_unitigs, &n_ids)) return rc;
    for (uint32_t u = 0; u < n_unitigs; ++u) if (bin_of_unitig[u] != 255 && bin_of_unitig[u] >= n_bins) return rtk_fail(RTK_ERR_ARG, "rtk_index_subsample_events: a unitig names a bin >= n_bins");
    return entry("rtk_index_subsample_events", device, [&]() {
        DevArr<uint64_t> d_ev, d_out; d_ev.alloc(n_events); d_out.alloc(n_events);
        if (n_events) rtk_check(hipMemcpy(d_ev.p, events, 8 * n_events, hipMemcpyHostToDevice), "hipMemcpy");
        const SubsampleResult r = subsample_events_device(d_ev.p, n_events, d_out.p, n_unitigs, n_ids, rule);
        *n_out = r.n_out; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
        if (r.n_out) rtk_check(hipMemcpy(events_out, d_out.p, 8 * r.n_out, hipMemcpyDeviceToHost), "hipMemcpy");
        return RTK_OK;
    });
}

// The ids of an open colouring job merged in place (the rule: rtk_index_merge.h): finishes the pending chunks and the last sort-and-unique, merges, and sets the job's
// events and ids, so that rtk_index_colour_end, rtk_index_colour_cov and rtk_index_colour_end_subsampled go on from the merged events. The job stays alive, also on error.
extern "C" int rtk_index_colour_merge(void* job, uint64_t* n_events_before, uint64_t* n_events_after, uint64_t* n_ids_before, uint64_t* n_ids_after) {
    ColourJob* J = static_cast<ColourJob*>(job);
    if (!J || !n_events_before || !n_events_after || !n_ids_before || !n_ids_after) return rtk_fail(RTK_ERR_ARG, "rtk_index_colour_merge: null argument");
    std::lock_guard<std::mutex> lk(J->m);
    return entry("rtk_index_colour_merge", J->device, [&]() {
        J->compact();
        const StageClock clk;
        MergeResult r; const uint64_t before = J->n_events;
        const uint64_t* out = merge_events_device(J->events.p, J->alt.p, before, J->n_unitigs, J->tmp, &r);
        if (before) { J->set_events(out, r.n_out); J->n_ids = r.ids_after; }
        J->merge_classes_above_one = r.classes_above_one; J->merge_largest = r.largest;
        *n_events_before = before; *n_events_after = J->n_events; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
        if (clk.trace) fprintf(stderr, "rtk_index_colour: ids merged on the device: %llu -> %llu ids, %llu -> %llu events (%.3f s)\n", static_cast<unsigned long long>(r.ids_before), static_cast<unsigned long long>(r.ids_after),
                               static_cast<unsigned long long>(before), static_cast<unsigned long long>(J->n_events), clk.since());
        return RTK_OK;
    });
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
    if (const int rc = check_device("rtk_index_merge_events", device)) return rc;
    if (const int rc = check_host_events("rtk_index_merge_events", events, n_events, n_unitigs, nullptr)) return rc;
    *n_out = 0; *n_ids_before = 0; *n_ids_after = 0;
    return entry("rtk_index_merge_events", device, [&]() {
        DevArr<uint64_t> d_a, d_b; DevArr<char> d_tmp; d_a.alloc(n_events); d_b.alloc(n_events);
        if (n_events) rtk_check(hipMemcpy(d_a.p, events, 8 * n_events, hipMemcpyHostToDevice), "hipMemcpy");
        MergeResult r; const uint64_t* out = merge_events_device(d_a.p, d_b.p, n_events, n_unitigs, d_tmp, &r);
        if (r.n_out > n_events) return rtk_fail(RTK_ERR_DEVICE, "rtk_index_merge_events: more events after the merge than before");
        if (r.n_out) rtk_check(hipMemcpy(events_out, out, 8 * r.n_out, hipMemcpyDeviceToHost), "hipMemcpy");
        *n_out = r.n_out; *n_ids_before = r.ids_before; *n_ids_after = r.ids_after;
        return RTK_OK;
    });
}

extern "C" int rtk_index_cover_begin(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* low_bits, void** job_out) {
    if (!seq_pool || !seq_off || !low_bits || !job_out || n_unitigs == 0) return rtk_fail(RTK_ERR_ARG, "rtk_index_cover_begin: null argument");
    if (n_unitigs > RTK_COVER_MAX_UNITIGS) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_cover_begin: more than 2^30 unitigs (a crossing names two unitigs in one word)");
    if (const int rc = check_k_and_device("rtk_index_cover_begin", k, device)) return rc;
    *job_out = nullptr;
    return entry("rtk_index_cover_begin", device, [&]() { std::unique_ptr<CoverJob> J(new CoverJob()); J->begin(device, k, seq_pool, seq_off, n_unitigs, low_bits); *job_out = J.release(); return RTK_OK; });
}

extern "C" int rtk_index_cover_chunk(void* job, const char* chars, uint64_t n_chars, const uint64_t* starts, const uint32_t* seq_numbers, const uint64_t* first_positions, uint32_t n_seqs) {
    CoverJob* J = static_cast<CoverJob*>(job);
    if (!J || !chars || !starts || !seq_numbers || !first_positions) return rtk_fail(RTK_ERR_ARG, "rtk_index_cover_chunk: null argument");
    if (n_seqs == 0 || n_chars == 0) return RTK_OK;
    if (n_chars > RTK_COVER_MAX_CHUNK || n_seqs > RTK_COVER_MAX_CHUNK / 16) return rtk_fail(RTK_ERR_ARG, "rtk_index_cover_chunk: chunk larger than 64 MB of characters / 4 M pieces");
    for (uint32_t r = 0; r < n_seqs; ++r) { // (the kernel finds the piece of a position by bisection over starts, and a position has 32 bits in a crossing)
        if (starts[r] >= n_chars || (r == 0 ? starts[0] != 0 : starts[r] <= starts[r - 1])) return rtk_fail(RTK_ERR_ARG, "rtk_index_cover_chunk: starts begin at 0, ascend and lie inside the chunk");
        if (first_positions[r] + ((r + 1 < n_seqs ? starts[r + 1] : n_chars) - starts[r]) > (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_cover_chunk: a sequence of more than 2^32 characters");
    }
    std::lock_guard<std::mutex> lk(J->m);
    return entry("rtk_index_cover_chunk", J->device, [&]() { J->chunk(chars, n_chars, starts, seq_numbers, first_positions, n_seqs); return RTK_OK; });
}

extern "C" int rtk_index_cover_end(void* job, uint64_t** crossings, uint64_t* n) {
    std::unique_ptr<CoverJob> J(static_cast<CoverJob*>(job));
    if (!J) return rtk_fail(RTK_ERR_ARG, "rtk_index_cover_end: null job");
    if (!crossings || !n) return RTK_OK; // (abandoned job: released)
    *crossings = nullptr; *n = 0;
    return entry("rtk_index_cover_end", J->device, [&]() {
        HostOut<uint64_t> out;
        if (!J->end(out)) return rtk_fail(RTK_ERR_IO, "rtk_index_cover_end: out of host memory");
        *crossings = out.release(); *n = J->n_found;
        J->trace_end();
        return RTK_OK;
    });
}

extern "C" int rtk_index_snp_candidates(int device, int k, const char* seq_pool, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint32_t flags, uint64_t** cand, uint64_t* n_cand) {
    if (!cand || !n_cand || (n_unitigs && (!seq_pool || !seq_off))) return rtk_fail(RTK_ERR_ARG, "rtk_index_snp_candidates: null argument");
    if (const int rc = check_k_and_device("rtk_index_snp_candidates", k, device)) return rc;
    if (n_unitigs >= 0xFFFFFFFFull) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_candidates: more than 2^32 - 1 unitigs");
    *cand = nullptr; *n_cand = 0;
    if (n_unitigs == 0) return RTK_OK;
    return entry("rtk_index_snp_candidates", device, [&]() { return by_key_type(k, [&](auto km) { return snp_candidates<decltype(km)>(k, seq_pool, seq_off, n_unitigs, searched, flags, cand, n_cand); }); });
}

extern "C" int rtk_index_snp_plan(int device, int k, const uint64_t* seq_off, uint64_t n_unitigs, const uint8_t* searched, uint64_t room, uint32_t* passes, uint64_t* need_one_pass, uint64_t* need_min) {
    if (!passes || !need_one_pass || !need_min || (n_unitigs && !seq_off)) return rtk_fail(RTK_ERR_ARG, "rtk_index_snp_plan: null argument");
    if (const int rc = check_k_and_device("rtk_index_snp_plan", k, device)) return rc;
    if (n_unitigs >= 0xFFFFFFFFull) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_snp_plan: more than 2^32 - 1 unitigs");
    *passes = 0; *need_one_pass = 0; *need_min = 0;
    const uint64_t none[1] = {0};
    return entry("rtk_index_snp_plan", device, [&]() { return by_key_type(k, [&](auto km) { return snp_plan<decltype(km)>(k, n_unitigs ? seq_off : none, n_unitigs, searched, room, passes, need_one_pass, need_min); }); });
}

extern "C" int rtk_index_pair_ids(int device, const uint64_t* name_hash, uint64_t n, uint32_t* ids, uint64_t* n_ids) {
    if (!n_ids || (n && (!name_hash || !ids))) return rtk_fail(RTK_ERR_ARG, "rtk_index_pair_ids: null argument");
    if (n >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_pair_ids: 2^32 records or more (an id has 32 bits)");
    if (const int rc = check_device("rtk_index_pair_ids", device)) return rc;
    *n_ids = 0;
    if (n == 0) return RTK_OK;
    return entry("rtk_index_pair_ids", device, [&]() { return pair_ids_device(name_hash, n, ids, n_ids); });
}

extern "C" int rtk_index_pair_plan(int device, uint64_t n, uint64_t room, uint32_t* passes, uint64_t* need_one_pass, uint64_t* need_min) {
    if (!passes || !need_one_pass || !need_min) return rtk_fail(RTK_ERR_ARG, "rtk_index_pair_plan: null argument");
    if (n >= (1ull << 32)) return rtk_fail(RTK_ERR_UNSUPPORTED, "rtk_index_pair_plan: 2^32 records or more (an id has 32 bits)");
    if (const int rc = check_device("rtk_index_pair_plan", device)) return rc;
    *passes = 1; *need_one_pass = 0; *need_min = 0;
    if (n == 0) return RTK_OK; // (nothing is allocated for no records)
    return entry("rtk_index_pair_plan", device, [&]() { return pair_plan_entry(n, room, passes, need_one_pass, need_min); });
}
