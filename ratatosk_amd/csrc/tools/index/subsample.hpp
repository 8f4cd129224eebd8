// rtk_build_index --subsample-colours: the colours thinned out by coverage before they are final (restates the subsampling of addCoverage,
// src/Graph.cpp:2312-2870, with estimateHaplotypeCoverage, src/Graph.cpp:4185-4234; DESIGN.md section 4 [A12]). One rule for the host route here and
// for the device route (csrc/hip/rtk_index_subsample.h rtk_index_colour_end_subsampled), which give the same bytes:
//   H     per-haplotype k-mer coverage from the simple bubbles of the graph; below 10 nothing is subsampled. rate = 5.0 / H.
//   bins  the rounded k-mer coverages of the unitigs, sorted descending, cut at twenty quantiles; bin j (lowest coverage first) is the half-open range
//         [s[p_j], s[p_j+1]) of coverages, an empty one is skipped, unitigs at the maximum fall into none.
//   ids   an id belongs to the first bin that holds a unitig it colours; it is kept when that bin starts below 5, else when u(id) <= rate. Beside that the
//         min_cov_vertices ids of smallest (h(id), id) of every non-branching unitig are kept (all of them when it has no more).
//   The kept ids are renumbered densely from 0, ascending; the colours of every unitig become the new ids of its kept ids. Coverage stays.
// Three deviations from the reference are forced. (1) It draws from std::random_device; this tool is deterministic and hashes the id:
// h(id) = splitmix64 finalizer of id + seed * 0x9E3779B97F4A7C15, u(id) = (h >> 11) * 2^-53 (--subsample-seed, default 1). (2) subsample()
// (src/Common.cpp:495-522) draws positions with replacement and can force fewer than min_cov_vertices ids; exactly that many are forced here, which
// is the purpose stated at src/Graph.cpp:2353. (3) The reference walks `for (double i = 1.0; i > 0.0; i -= 0.05)` and indexes with n * i, so its last
// step depends on accumulated rounding; the boundaries here are the integers p_j = n (20 - j) / 20, p_0 taken as n - 1.
// The phased-read lists of src/Graph.cpp:2605-2642 have no counterpart: there is no phasing input.
#ifndef RTK_TOOLS_INDEX_SUBSAMPLE_HPP
#define RTK_TOOLS_INDEX_SUBSAMPLE_HPP

#include <functional>

#include "colour.hpp"

namespace rtk {

inline uint64_t subsample_hash(uint64_t id, uint64_t seed) {
    uint64_t z = id + seed * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
inline double subsample_unit(uint64_t h) { return static_cast<double>(h >> 11) * (1.0 / 9007199254740992.0); } // exact: 53 bits times 2^-53

// H of the rule: forward orientation of every unitig only, as the reference's loop
template <class KM> static uint64_t haplotype_coverage(const IndexBuild<KM>& s) {
    const int k = s.k; const size_t n = s.U.size();
    struct Or { int64_t u; bool fw; };
    auto succ = [&](size_t u, bool fw, Or out[4]) { // oriented successors of oriented unitig (u, fw)
        int m = 0; const KM endk = fw ? s.tailk[u] : kmer_revcomp(s.headk[u], k);
        for (uint64_t b = 0; b < 4; ++b) { const int64_t w = s.adj[u].u[fw ? 0 : 1][b]; if (w < 0) continue; out[m].u = w; out[m].fw = (((endk << 2) | static_cast<KM>(b)) & s.mask) == s.headk[static_cast<size_t>(w)]; ++m; }
        return m;
    };
    auto degree = [&](size_t u, int d) { int m = 0; for (int b = 0; b < 4; ++b) m += s.adj[u].u[d][b] >= 0; return m; };
    uint64_t tot_cov = 0, nb_km = 0;
    for (size_t u = 0; u < n; ++u) {
        Or v[4]; const int m = succ(u, true, v);
        if (m < 2) continue;
        bool branches = false;
        for (int i = 0; i < m; ++i) branches = branches || degree(static_cast<size_t>(v[i].u), v[i].fw ? 0 : 1) > 1 || degree(static_cast<size_t>(v[i].u), v[i].fw ? 1 : 0) > 1;
        if (branches) continue;
        bool simple = true, have_end = false; Or end; end.u = -1; end.fw = true;
        for (int i = 0; i < m; ++i) { Or w[4]; const int mm = succ(static_cast<size_t>(v[i].u), v[i].fw, w);
            for (int j = 0; j < mm; ++j) { if (!have_end) { end = w[j]; have_end = true; } else simple = simple && w[j].u == end.u && w[j].fw == end.fw; } }
        if (!simple) continue;
        for (int i = 0; i < m; ++i) { nb_km += s.U[static_cast<size_t>(v[i].u)].seq.size() - static_cast<size_t>(k) + 1; tot_cov += s.U[static_cast<size_t>(v[i].u)].cov; }
    }
    return nb_km == 0 ? 0 : tot_cov / nb_km;
}

// what the host works out from coverage and structure; the events and ids are then thinned on the host threads or on the device
struct SubsamplePlan {
    static const uint32_t N_BINS = 20;
    uint64_t hap_cov = 0; double rate = 0.0;
    std::vector<uint8_t> bin_of_unitig, forced_candidate; // bin 0..19 or 255 for none; 1: non-branching
    uint8_t bin_is_sampled[N_BINS]; uint32_t bins = 0, sampled_bins = 0; // non-empty bins, and those of them that start at coverage >= 5
};
struct SubsampleCounts { uint64_t ids_before = 0, ids_after = 0, events_before = 0, events_after = 0; };

template <class KM> static void subsample_plan(const IndexBuild<KM>& s, SubsamplePlan& p) {
    const size_t n = s.U.size(); const uint32_t NB = SubsamplePlan::N_BINS;
    p.hap_cov = haplotype_coverage(s);
    memset(p.bin_is_sampled, 0, sizeof(p.bin_is_sampled));
    if (p.hap_cov < 10 || n == 0) return;
    p.rate = 5.0 / static_cast<double>(p.hap_cov);
    std::vector<uint64_t> kc(n);
    for (size_t u = 0; u < n; ++u) kc[u] = static_cast<uint64_t>(static_cast<long long>(static_cast<double>(s.U[u].cov) / static_cast<double>(s.U[u].seq.size() - s.k + 1) + 0.5)); // (colour_split's kcov)
    std::vector<uint64_t> srt(kc); std::sort(srt.begin(), srt.end(), std::greater<uint64_t>());
    uint64_t lo[NB], hi[NB];
    for (uint32_t j = 0; j < NB; ++j) {
        const size_t pj = j == 0 ? n - 1 : n * (NB - j) / NB, pj1 = n * (NB - j - 1) / NB;
        lo[j] = srt[pj]; hi[j] = srt[pj1];
        if (lo[j] < hi[j]) { ++p.bins; if (lo[j] >= 5) { p.bin_is_sampled[j] = 1; ++p.sampled_bins; } }
    }
    p.bin_of_unitig.assign(n, 255); p.forced_candidate.assign(n, 0);
    for (size_t u = 0; u < n; ++u) {
        for (uint32_t j = 0; j < NB; ++j) if (lo[j] < hi[j] && kc[u] >= lo[j] && kc[u] < hi[j]) { p.bin_of_unitig[u] = static_cast<uint8_t>(j); break; }
        p.forced_candidate[u] = (s.kmcov[u] >> 63) ? 0 : 1;
    }
}

// the rule on the colours of the unitigs, on the host threads (one thread without --fast: the same bytes)
template <class KM> static void subsample_host(IndexBuild<KM>& s, const SubsamplePlan& p, uint64_t seed, SubsampleCounts& c) {
    std::vector<Unitig>& U = s.U; const size_t n = U.size(); const unsigned nt = s.o.fast ? s.n_thr : 1u; const size_t mcv = s.o.min_cov_vertices;
    uint64_t n_ids = 0;
    for (size_t u = 0; u < n; ++u) { c.events_before += U[u].colours.size(); if (!U[u].colours.empty()) n_ids = std::max<uint64_t>(n_ids, static_cast<uint64_t>(U[u].colours.back()) + 1); }
    const uint64_t n_words = (n_ids + 63) / 64;
    std::vector<uint8_t> first_bin(n_ids, 255); // 255: the id colours nothing, 254: only unitigs of no bin
    std::vector<uint64_t> keep(n_words, 0), rank(n_words + 1, 0);
    parallel_for(n, nt, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) {
        const std::vector<uint32_t>& col = U[u].colours; const uint8_t bin = p.bin_of_unitig[u] == 255 ? 254 : p.bin_of_unitig[u];
        for (size_t i = 0; i < col.size(); ++i) { uint8_t* f = &first_bin[col[i]]; uint8_t old = __atomic_load_n(f, __ATOMIC_RELAXED); while (old > bin && !__atomic_compare_exchange_n(f, &old, bin, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} }
        if (!p.forced_candidate[u]) continue;
        auto force = [&](uint32_t id) { __atomic_fetch_or(&keep[id >> 6], 1ULL << (id & 63), __ATOMIC_RELAXED); };
        if (col.size() <= mcv) { for (size_t i = 0; i < col.size(); ++i) force(col[i]); continue; }
        std::vector<std::pair<uint64_t, uint32_t> > hs(col.size());
        for (size_t i = 0; i < col.size(); ++i) hs[i] = std::make_pair(subsample_hash(col[i], seed), col[i]);
        std::partial_sort(hs.begin(), hs.begin() + static_cast<std::ptrdiff_t>(mcv), hs.end());
        for (size_t i = 0; i < mcv; ++i) force(hs[i].second);
    } });
    std::vector<uint64_t> present(nt, 0);
    parallel_for(static_cast<size_t>(n_words), nt, [&](size_t b, size_t e, unsigned t) { for (size_t w = b; w < e; ++w) {
        uint64_t bits = 0;
        for (uint64_t j = 0; j < 64 && 64 * w + j < n_ids; ++j) {
            const uint64_t id = 64 * w + j; const uint8_t fb = first_bin[id];
            if (fb != 255) ++present[t];
            if (fb < SubsamplePlan::N_BINS && (!p.bin_is_sampled[fb] || subsample_unit(subsample_hash(id, seed)) <= p.rate)) bits |= 1ULL << j;
        }
        keep[w] |= bits;
    } });
    for (unsigned t = 0; t < nt; ++t) c.ids_before += present[t];
    for (uint64_t w = 0; w < n_words; ++w) rank[w + 1] = rank[w] + static_cast<uint64_t>(__builtin_popcountll(keep[w]));
    c.ids_after = rank[n_words];
    std::vector<uint64_t> left(nt, 0);
    parallel_for(n, nt, [&](size_t b, size_t e, unsigned t) { for (size_t u = b; u < e; ++u) {
        std::vector<uint32_t>& col = U[u].colours; size_t m = 0;
        for (size_t i = 0; i < col.size(); ++i) { const uint32_t id = col[i]; const uint64_t w = keep[id >> 6], bit = 1ULL << (id & 63);
            if (w & bit) col[m++] = static_cast<uint32_t>(rank[id >> 6] + static_cast<uint64_t>(__builtin_popcountll(w & (bit - 1)))); }
        col.resize(m); left[t] += m;
    } });
    for (unsigned t = 0; t < nt; ++t) c.events_after += left[t];
}

// the step: needs the structural half of the adjacency (successors, branching); the edge bits come after it, on the thinned colours
template <class KM> static bool subsample_colours(IndexBuild<KM>& s) {
    std::shared_ptr<void> hold; hold.swap(s.colour_sink); // (the sink goes when the step returns)
    ColourSink<KM>* sink = static_cast<ColourSink<KM>*>(hold.get());
    SubsamplePlan p; subsample_plan(s, p);
    if (p.hap_cov < 10) {
        fprintf(stderr, "rtk_build_index: subsample: hap_cov=%llu off\n", static_cast<unsigned long long>(p.hap_cov));
        return !(sink && sink->job) || sink->finish_device(); // (the device still holds the events)
    }
    SubsampleCounts c;
    if (sink && sink->job) { if (!sink->finish_device_subsampled(p.bin_of_unitig.data(), p.forced_candidate.data(), p.bin_is_sampled, SubsamplePlan::N_BINS, p.rate, s.o.subsample_seed, &c.events_before, &c.events_after, &c.ids_before, &c.ids_after)) return false; }
    else subsample_host(s, p, s.o.subsample_seed, c);
    fprintf(stderr, "rtk_build_index: subsample: hap_cov=%llu rate=%.6f ids=%llu->%llu events=%llu->%llu bins=%u sampled_bins=%u\n", static_cast<unsigned long long>(p.hap_cov), p.rate,
            static_cast<unsigned long long>(c.ids_before), static_cast<unsigned long long>(c.ids_after), static_cast<unsigned long long>(c.events_before), static_cast<unsigned long long>(c.events_after), p.bins, p.sampled_bins);
    return true;
}

} // namespace rtk

#endif
