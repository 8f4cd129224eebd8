// rtk_build_index --merge-duplicates: short-read pairs that lie on the same unitigs share one colour id (restates the block the reference announces as "Detecting
// and removing duplicated reads", src/Graph.cpp:1630-1705 and 2089-2134: every pair gets a signature, the sum of the hashes of the unitigs its reads map to, and
// pairs of equal signature that meet on a unitig receive the same read id; DESIGN.md section 4 [A13]). One rule for the host route here and for the device route
// (csrc/hip/rtk_index_merge.h rtk_index_colour_merge), which give the same bytes:
//   U(i)   the unitigs of id i (an id without events takes no part); g(u) = subsample_hash(u + 1, 0), the splitmix64 finalizer of u + 1;
//   S(i)   the sum of g(u) over U(i) modulo 2^64; low(i) = min U(i).
//   Ids with equal (S, low) are one class; its leader is its smallest id; the leaders, ascending, are numbered from 0; every id takes its leader's number; the
//   colours of a unitig become the distinct new numbers of its ids, ascending. Coverage, unitigs and the FASTA stay (merged reads still count as coverage,
//   src/Graph.cpp:1721-1765).
// Deviations, all forced. (1) The reference sums per mate, so a unitig under both mates counts twice; the events hold the distinct unitigs of the pair, and those
// are summed. (2) g by the unitig's number (the tool's own order, which plain, --fast and --gpu share) replaces Bifrost's hash of the head k-mer [A9]. (3) The
// reference merges only pairs that chose the same centroid unitig, and which one a pair chooses depends on what other threads have written (src/Graph.cpp:
// 1669-1690); here every pair with an equal key merges: `low` stands in for "meet on a unitig" and keeps a chance collision of the 64-bit sum local, which the
// reference accepts as well. (4) The reference numbers in unitig iteration order from 1; here by leader from 0, as [A12] numbers. (5) -S RATE, the read-level
// draw of the same block (src/Graph.cpp:2117, 2123), is out of scope. With --colour-reads every read keeps its own id (src/Graph.cpp:
// 2115-2118): the step says `merge: off (--colour-reads)` and changes nothing.
// Every table is sized by the events or by the ids that have events, never by the largest id.
#ifndef RTK_TOOLS_INDEX_MERGE_HPP
#define RTK_TOOLS_INDEX_MERGE_HPP

#include "subsample.hpp"

namespace rtk {

struct MergeCounts { uint64_t ids_before = 0, ids_after = 0, events_before = 0, events_after = 0, classes_above_one = 0, largest = 0; };

// v sorted ascending, its values distinct: pieces sorted by the threads, then merged pairwise (the same order with any number of threads)
inline void merge_sort_words(std::vector<uint64_t>& v, unsigned nt) {
    if (nt < 2 || v.size() < (1u << 12)) { std::sort(v.begin(), v.end()); return; }
    std::vector<size_t> cut(nt + 1); for (unsigned t = 0; t <= nt; ++t) cut[t] = v.size() * t / nt;
    parallel_for(nt, nt, [&](size_t b, size_t e, unsigned) { for (size_t t = b; t < e; ++t) std::sort(v.begin() + static_cast<std::ptrdiff_t>(cut[t]), v.begin() + static_cast<std::ptrdiff_t>(cut[t + 1])); });
    for (unsigned w = 1; w < nt; w *= 2) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t + w < nt; t += 2 * w) th.emplace_back([&, t]() { std::inplace_merge(v.begin() + static_cast<std::ptrdiff_t>(cut[t]), v.begin() + static_cast<std::ptrdiff_t>(cut[t + w]), v.begin() + static_cast<std::ptrdiff_t>(cut[std::min(nt, t + 2 * w)])); });
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
    }
}

// the rule on the colours of the unitigs (sorted, each id once), on nt host threads: the same result with any nt
inline void merge_host(std::vector<Unitig>& U, unsigned nt, MergeCounts& c) {
    const size_t n = U.size(); if (nt < 1) nt = 1;
    std::vector<uint64_t> first(n + 1, 0); for (size_t u = 0; u < n; ++u) first[u + 1] = first[u] + U[u].colours.size();
    c.events_before = first[n];
    std::vector<uint64_t> ev(first[n]); // id << 32 | unitig: sorted, an id is one run with its unitigs ascending
    parallel_for(n, nt, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) for (size_t i = 0; i < U[u].colours.size(); ++i) ev[first[u] + i] = (static_cast<uint64_t>(U[u].colours[i]) << 32) | u; });
    merge_sort_words(ev, nt);
    struct Run { uint64_t S; uint32_t low, id, at; }; // at: the place of the id among the ids that have events
    std::vector<Run> runs;
    for (size_t i = 0; i < ev.size();) {
        Run r; r.S = 0; r.id = static_cast<uint32_t>(ev[i] >> 32); r.low = static_cast<uint32_t>(ev[i]); r.at = static_cast<uint32_t>(runs.size());
        for (; i < ev.size() && (ev[i] >> 32) == r.id; ++i) r.S += subsample_hash((ev[i] & 0xFFFFFFFFull) + 1, 0);
        runs.push_back(r);
    }
    std::vector<uint64_t>().swap(ev);
    const size_t R = runs.size(); c.ids_before = R;
    std::vector<uint32_t> ids(R); for (size_t r = 0; r < R; ++r) ids[r] = runs[r].id;
    std::sort(runs.begin(), runs.end(), [](const Run& a, const Run& b) { return a.S != b.S ? a.S < b.S : (a.low != b.low ? a.low < b.low : a.id < b.id); });
    std::vector<uint32_t> leader(R); std::vector<uint64_t> number(R + 1, 0); // leader[at]: the place of the id's leader; number[at]: leaders before this place
    for (size_t j = 0; j < R;) {
        size_t e = j + 1; while (e < R && runs[e].S == runs[j].S && runs[e].low == runs[j].low) ++e;
        for (size_t x = j; x < e; ++x) leader[runs[x].at] = runs[j].at;
        number[runs[j].at + 1] = 1;
        if (e - j > 1) ++c.classes_above_one;
        c.largest = std::max<uint64_t>(c.largest, e - j);
        j = e;
    }
    for (size_t r = 0; r < R; ++r) number[r + 1] += number[r];
    c.ids_after = number[R];
    std::vector<uint64_t> left(nt, 0);
    parallel_for(n, nt, [&](size_t b, size_t e, unsigned t) { for (size_t u = b; u < e; ++u) {
        std::vector<uint32_t>& col = U[u].colours;
        for (size_t i = 0; i < col.size(); ++i) col[i] = static_cast<uint32_t>(number[leader[static_cast<size_t>(std::lower_bound(ids.begin(), ids.end(), col[i]) - ids.begin())]]);
        std::sort(col.begin(), col.end()); col.erase(std::unique(col.begin(), col.end()), col.end());
        left[t] += col.size();
    } });
    for (unsigned t = 0; t < nt; ++t) c.events_after += left[t];
}

inline void merge_line(const MergeCounts& c) {
    fprintf(stderr, "rtk_build_index: merge: ids=%llu->%llu events=%llu->%llu classes_above_one=%llu largest=%llu\n", static_cast<unsigned long long>(c.ids_before), static_cast<unsigned long long>(c.ids_after),
            static_cast<unsigned long long>(c.events_before), static_cast<unsigned long long>(c.events_after), static_cast<unsigned long long>(c.classes_above_one), static_cast<unsigned long long>(c.largest));
}

// the step: right after the colouring, so that subsampling, edge bits, short cycles, SNP annotations and the global / local split all see the merged ids
template <class KM> static bool merge_duplicates(IndexBuild<KM>& s) {
    if (!s.o.colour_files.empty()) { fprintf(stderr, "rtk_build_index: merge: off (--colour-reads)\n"); return true; }
    MergeCounts c;
    ColourSink<KM>* sink = static_cast<ColourSink<KM>*>(s.colour_sink.get());
    if (sink && sink->job && sink->merge_fn) { // the events are on the device and stay there: merged in place
        if (!sink->merge_device(&c.events_before, &c.events_after, &c.ids_before, &c.ids_after, &c.classes_above_one, &c.largest)) return false;
        if (!(s.o.subsample && sink->end_sub_fn)) { const bool ok = sink->finish_device(); s.colour_sink.reset(); if (!ok) return false; } // (else they wait there for the subsampling step)
    }
    else merge_host(s.U, s.o.fast ? s.n_thr : 1u, c);
    merge_line(c);
    return true;
}

} // namespace rtk

#endif
