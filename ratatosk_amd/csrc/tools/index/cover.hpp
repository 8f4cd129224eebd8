// rtk_build_index --cover-edges-from FILE: the low-coverage edges that the sequences of FILE cross get two fresh colour ids on both ends (restates the last block of
// the reference's first-pass addCoverage, "Covering low coverage edges.", src/Graph.cpp:3085-3363; DESIGN.md section 4 [A16]). FILE is the unitig FASTA of the k2
// graph (what --graph-only writes), or any FASTA. One rule for the plain route, --fast and --gpu (csrc/hip/rtk_index_cover.h), which write the same bytes:
//   record  low[u], one byte per unitig, after the edge bits are known: for every edge of u whose shared bit is NOT set (fewer than min_cov_vertices colours in
//           common), bit idx(c) of the base c the successor appends (A, C, G, T = 1, 2, 4, 8) for the forward strand, the same bit << 4 for the reverse strand --
//           the nibbles the other way round than in the `shared` byte (annotate.hpp), as in the reference (src/Graph.cpp:3109, 3126 against UnitigData.hpp:263-273).
//   map     a CROSSING is a position p of a sequence whose windows at p and p + 1 are all A/C/G/T (either case), the k-mer at p is the last k-mer of its unitig u in
//           the direction the text walks it, the k-mer at p + 1 is in the graph (on v; v may be u), and bit (direction, character p + k) of low[u] is set as
//           recorded. In a compacted graph this is what the reference's map / extend / jump walk with its adjacency test finds: a k-mer inside its unitig has one
//           successor, so a mapping can only end at the end of its unitig, at a window that is no k-mer of the graph, or at the end of the text.
//   walk    the crossings in the order of the file, left to right (the reference's order with one thread): if the bit is STILL set, both unitigs get the ids next
//           and next + 1 (two ids whatever min_cov_vertices is), next += 2, the bit is cleared. The other direction of the same edge is another bit on the other
//           unitig: crossed that way, the edge gets two more ids. The first id is one above the largest id that colours a unitig at that point (after merging and
//           subsampling, which number their ids densely from 0: the number of ids they report).
// The added ids join the colours the annotators read (short cycles, SNPs), not the edge bits (the reference does not recompute them), not the coverage; the global /
// local split is made on the read colours alone and the added ids are appended to the local sets afterwards (SharedPairID::add puts a fresh id there).
#ifndef RTK_TOOLS_INDEX_COVER_HPP
#define RTK_TOOLS_INDEX_COVER_HPP

#include "state.hpp"

namespace rtk {

struct CoverCounts { uint64_t recorded = 0, covered = 0, ids_added = 0; };

// the crossings of one sequence appended to `out`, two words each as the device writes them: sequence << 32 | p, u << 33 | v << 3 | direction << 2 | base
template <class KM> static void cover_map_sequence(IndexBuild<KM>& s, const std::vector<uint8_t>& low, const char* seq, size_t len, uint64_t seq_number, std::vector<uint64_t>& out) {
    const int k = s.k; KM fw = 0; int valid = 0;
    bool prev_last = false, prev_rev = false; size_t prev_u = 0; // the window before this one: in the graph and the last k-mer of its unitig in walk direction
    for (size_t i = 0; i < len; ++i) {
        const int b = base2bits(seq[i]);
        if (b < 0) { valid = 0; fw = 0; prev_last = false; continue; }
        fw = ((fw << 2) | static_cast<KM>(b)) & s.mask;
        if (++valid < k) continue;
        const size_t p = i + 1 - static_cast<size_t>(k);
        bool q_can; const KM can = kmer_canonical(fw, k, &q_can);
        const uint64_t* v = s.km.slot(can, false);
        if (!v) { prev_last = false; continue; }
        const size_t u = static_cast<size_t>((*v >> 32) - 1), off = static_cast<size_t>((*v & 0xFFFFFFFFULL) >> 1);
        if (prev_last) {
            const unsigned bit = (1u << b) << (prev_rev ? 4 : 0);
            if (low[prev_u] & bit) { out.push_back((seq_number << 32) | static_cast<uint64_t>(p - 1)); out.push_back((static_cast<uint64_t>(prev_u) << 33) | (static_cast<uint64_t>(u) << 3) | (prev_rev ? 4ULL : 0ULL) | static_cast<uint64_t>(b)); }
        }
        const bool walk_fw = ((*v & 1ULL) != 0) == q_can; // the unitig spells the window as the text does
        prev_u = u; prev_rev = !walk_fw;
        prev_last = walk_fw ? off + static_cast<size_t>(k) == s.U[u].seq.size() : off == 0;
    }
}

// --gpu: the sequences handed to the device in chunks of pieces (a sequence longer than a chunk is cut, a piece starting k characters before the end of the one
// before it, so that every pair of windows lies whole inside exactly one piece); the crossings of all of them come back sorted at the end
template <class KM> struct CoverFeed {
    IndexBuild<KM>& s; void* job = nullptr; HipLib::cover_chunk_fn chunk_fn = nullptr; HipLib::cover_end_fn end_fn = nullptr; bool failed = false;
    std::string chars; std::vector<uint64_t> starts, first; std::vector<uint32_t> seqs; size_t chunk_chars = 48u << 20;
    explicit CoverFeed(IndexBuild<KM>& st) : s(st) { const char* e = getenv("RTK_INDEX_CHUNK"); if (e && strtoull(e, nullptr, 10) >= 1024) chunk_chars = std::min<size_t>(static_cast<size_t>(strtoull(e, nullptr, 10)), 60u << 20); }
    ~CoverFeed() { if (job) end_fn(job, nullptr, nullptr); } // (left early: the job released)
    bool open(const std::vector<uint8_t>& low) {
        HipLib::cover_begin_fn begin_fn = nullptr;
        if (!s.lib.handle || !s.lib.get(begin_fn, "rtk_index_cover_begin") || !s.lib.get(chunk_fn, "rtk_index_cover_chunk") || !s.lib.get(end_fn, "rtk_index_cover_end")) {
            fprintf(stderr, "rtk_build_index: --gpu: %s lacks rtk_index_cover_begin / _chunk / _end: edges covered on the host threads\n", s.lib.path.c_str()); return false; }
        const size_t n_u = s.U.size();
        std::vector<uint64_t> off(n_u + 1, 0); for (size_t u = 0; u < n_u; ++u) off[u + 1] = off[u] + s.U[u].seq.size();
        std::string pool(off[n_u], 'A');
        parallel_for(n_u, s.n_thr, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) memcpy(&pool[off[u]], s.U[u].seq.data(), s.U[u].seq.size()); });
        if (begin_fn(0, s.k, pool.data(), off.data(), n_u, low.data(), &job) != 0) { fprintf(stderr, "rtk_build_index: --gpu: edges covered on the host threads (%s)\n", s.lib.last_error()); job = nullptr; return false; }
        return true;
    }
    void flush() {
        if (seqs.empty()) return;
        if (chunk_fn(job, chars.data(), chars.size(), starts.data(), seqs.data(), first.data(), static_cast<uint32_t>(seqs.size())) != 0) failed = true;
        chars.clear(); starts.clear(); first.clear(); seqs.clear();
    }
    void add(const char* seq, size_t len, uint64_t seq_number) {
        const size_t k = static_cast<size_t>(s.k), piece = chunk_chars - 1;
        if (len < k + 1) return; // (no pair of windows)
        for (size_t a = 0;;) {
            const size_t e = std::min(len, a + piece);
            if (chars.size() + (e - a) + 1 > chunk_chars || seqs.size() >= (2u << 20)) flush();
            starts.push_back(chars.size()); first.push_back(a); seqs.push_back(static_cast<uint32_t>(seq_number));
            chars.append(seq + a, e - a); chars.push_back('\n');
            if (e == len) break;
            a = e - k;
        }
    }
    bool finish(std::vector<uint64_t>& crossings) {
        flush();
        uint64_t* list = nullptr; uint64_t n = 0; void* j = job; job = nullptr;
        if (end_fn(j, &list, &n) != 0 || failed) { fprintf(stderr, "rtk_build_index: --gpu: covering the edges on the device failed (%s)\n", s.lib.last_error()); if (list) s.lib.free(list); return false; }
        crossings.assign(list, list + 2 * n); s.lib.free(list);
        return true;
    }
};

// The step: after edge_bits, before the annotators. The added ids are appended to the colours (and noted in s.cover_ids for the split).
template <class KM> static bool cover_edges(IndexBuild<KM>& s) {
    const size_t n = s.U.size(); CoverCounts c;
    // record
    std::vector<uint8_t> low(n, 0);
    for (size_t u = 0; u < n; ++u) for (int d = 0; d < 2; ++d) for (unsigned b = 0; b < 4; ++b) {
        if (s.adj[u].u[d][b] < 0) continue;
        const uint64_t shared_bit = d == 0 ? ((1ULL << b) << 4) : (1ULL << b);
        if (!(s.shared[u] & shared_bit)) { low[u] = static_cast<uint8_t>(low[u] | (d == 0 ? (1u << b) : ((1u << b) << 4))); ++c.recorded; }
    }
    uint64_t next = 0; // one above the largest id that colours a unitig
    for (size_t u = 0; u < n; ++u) if (!s.U[u].colours.empty()) next = std::max<uint64_t>(next, static_cast<uint64_t>(s.U[u].colours.back()) + 1);
    s.cover_ids.assign(n, std::vector<uint32_t>());
    // walk: the crossings in order; false: the ids ran out
    auto walk = [&](const std::vector<uint64_t>& x) {
        for (size_t i = 0; i + 1 < x.size(); i += 2) {
            const uint64_t w1 = x[i + 1]; const size_t u = static_cast<size_t>(w1 >> 33), v = static_cast<size_t>((w1 >> 3) & 0x3FFFFFFFULL);
            const unsigned bit = (1u << (w1 & 3ULL)) << ((w1 & 4ULL) ? 4 : 0);
            if (!(low[u] & bit)) continue;
            if (next + 2 > 0xFFFFFFFFULL) return false;
            for (int j = 0; j < 2; ++j, ++next) { s.cover_ids[u].push_back(static_cast<uint32_t>(next)); if (v != u) s.cover_ids[v].push_back(static_cast<uint32_t>(next)); }
            low[u] = static_cast<uint8_t>(low[u] & ~bit); ++c.covered; c.ids_added += 2;
        }
        return true;
    };
    std::unique_ptr<CoverFeed<KM> > feed;
    if (s.o.gpu && n > 0) { feed.reset(new CoverFeed<KM>(s)); if (!feed->open(low)) feed.reset(); }
    // map: the records of the files in their order, numbered as they come; batches of about 64 MB mapped (--fast: by the threads, a range of records each) and walked
    struct Batch { std::vector<std::string> seq; std::vector<uint64_t> number; size_t bytes = 0; } batch;
    bool ok = true; uint64_t seq_number = 0, long_enough = 0;
    auto run_batch = [&]() {
        if (batch.seq.empty()) return;
        if (feed) { for (size_t r = 0; r < batch.seq.size(); ++r) feed->add(batch.seq[r].data(), batch.seq[r].size(), batch.number[r]); }
        else {
            const unsigned nt = s.o.fast ? s.n_thr : 1u;
            std::vector<std::vector<uint64_t> > found(nt);
            parallel_for(batch.seq.size(), nt, [&](size_t b, size_t e, unsigned t) { for (size_t r = b; r < e; ++r) cover_map_sequence(s, low, batch.seq[r].data(), batch.seq[r].size(), batch.number[r], found[t]); });
            for (unsigned t = 0; t < nt && ok; ++t) ok = walk(found[t]); // (the ranges are in the order of the records; the bits are only read while mapping)
        }
        batch.seq.clear(); batch.number.clear(); batch.bytes = 0;
    };
    std::string name, seq, qual;
    for (size_t f = 0; f < s.o.cover_files.size() && ok; ++f) {
        FastxReader fr; if (!fr.open(s.o.cover_files[f], s.o.fast ? static_cast<int>(s.n_thr < 8 ? s.n_thr : 8) : 0)) { fprintf(stderr, "rtk_build_index: --cover-edges-from: cannot open %s\n", s.o.cover_files[f].c_str()); return false; }
        while (ok && fr.next(name, seq, qual)) {
            if (seq_number >= 0xFFFFFFFFULL || seq.size() >= 0xFFFFFFFFULL) { fprintf(stderr, "rtk_build_index: --cover-edges-from: more than 2^32 - 1 sequences, or a sequence that long\n"); return false; }
            if (seq.size() >= static_cast<size_t>(s.k)) ++long_enough;
            batch.bytes += seq.size(); batch.number.push_back(seq_number++); batch.seq.push_back(std::string()); batch.seq.back().swap(seq);
            if (batch.bytes >= (64u << 20)) run_batch();
        }
        if (fr.failed()) { fprintf(stderr, "rtk_build_index: --cover-edges-from: %s ends in a damaged or cut-short gzip stream\n", s.o.cover_files[f].c_str()); return false; }
    }
    if (ok) run_batch();
    if (ok && feed) { std::vector<uint64_t> crossings; if (!feed->finish(crossings)) return false; ok = walk(crossings); }
    if (!ok) { fprintf(stderr, "rtk_build_index: --cover-edges-from: more than 2^32 colour ids\n"); return false; }
    if (long_enough == 0) fprintf(stderr, "rtk_build_index: --cover-edges-from: no sequence of %d characters in the file%s given: nothing covered\n", s.k, s.o.cover_files.size() > 1 ? "s" : "");
    // the ids join the colours the annotators read: larger than every read id, ascending as handed out
    parallel_for(n, s.o.fast ? s.n_thr : 1u, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) s.U[u].colours.insert(s.U[u].colours.end(), s.cover_ids[u].begin(), s.cover_ids[u].end()); });
    if (s.knobs.trace) fprintf(stderr, "rtk_build_index: cover: edges_recorded=%llu edges_covered=%llu ids_added=%llu\n", static_cast<unsigned long long>(c.recorded), static_cast<unsigned long long>(c.covered), static_cast<unsigned long long>(c.ids_added));
    return true;
}

} // namespace rtk

#endif
