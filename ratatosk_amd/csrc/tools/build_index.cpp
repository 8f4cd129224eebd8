// rtk_build_index: minimal, deterministic producer of the two index files `Ratatosk correct -1` consumes:
//   PREFIX.index.k31.fasta.gz   unitigs of the compacted de Bruijn graph (one FASTA record per unitig)
//   PREFIX.index.k31.rtsk       per-unitig data records (format: ../common/rtsk_io.hpp)
//
// This is NOT the reference's `index` step (src/Graph.cpp:1561-3366 `addCoverage`, Bifrost `build`):
// that step is out of the hot-path scope and cannot be built here (Bifrost is
// absent). It only has to emit the reference's *file formats* with semantically equivalent content so
// the correction path has inputs:
//   * unitigs        = maximal non-branching paths over canonical k-mers seen >= --min-count times
//   * colours        = ids of the short-read pairs having >= 1 k-mer on the unitig (sorted u32)
//   * kmCov          = number of read k-mers mapped on the unitig (unphased coverage, bits 31..61)
//   * branching bit  = >1 predecessors or >1 successors            (reference: src/Graph.cpp:1997)
//   * edge bits      = neighbour shares >= min_cov_vertices colours (reference: src/Graph.cpp:1999-2017)
//   * merged ids     (--merge-duplicates only) = read pairs on the same unitigs share one colour id, as src/Graph.cpp:1630-1705, 2089-2134 do (index/merge.hpp)
//   * subsampling    (--subsample-colours only) = the colours thinned by coverage as src/Graph.cpp:2312-2870 does (index/subsample.hpp)
//   * global/local   = simplified form of the colour compaction of src/Graph.cpp:2874-2985
//   * short cycles   = restatement of detectShortCycles (src/Graph.cpp:4660-4735), so that fixRepeats has inputs
//   * SNP annotations (--snps only) = restatement of detectSNPs (src/Graph.cpp:484-720) with the breadth-first bubble walk of
//     isValidSNPcandidate (src/GraphTraversal.cpp:1057-1147); haplotype ids stay empty (no phasing input).
//   * graph reuse    (--graph-only / --graph-from) = the graph of one build's unitig FASTA taken as the graph of another, of any k: the reference builds its k1 graph
//     from the text of the k2 unitigs and reads the k2 graph back for the second pass (src/Ratatosk.cpp:1092-1101, 1194); DESIGN.md section 4 [A15]
//   covered edges  (--cover-edges-from only) = the edges that too few colours share get two fresh ids on both ends where a k2 unitig walks over them, as the last
//     block of addCoverage does (src/Graph.cpp:3085-3363; index/cover.hpp; DESIGN.md section 4 [A16])
// The build is a list of steps over one state (tools/index/state.hpp): run<KM>() below names them in order.
#include <zlib.h>

#include <fstream>
#include <sstream>

#include "../common/kmer_count.hpp"
#include "../common/rtsk_io.hpp"
#include "index/annotate.hpp"
#include "index/colour.hpp"
#include "index/cover.hpp"
#include "index/merge.hpp"
#include "index/subsample.hpp"
#include "index/unitigs.hpp"

using namespace rtk;

// --dump-input: what a `sample:` source stands for, as a file (tests compare the index built from either)
static int dump_input(const IndexOptions& o) {
    FILE* fo = fopen(o.dump_input.c_str(), "wb"); if (!fo) { fprintf(stderr, "rtk_build_index: cannot write %s\n", o.dump_input.c_str()); return 1; }
    std::string name, seq, qual;
    for (size_t f = 0; f < o.in_files.size(); ++f) { FastxReader fr; if (!fr.open(o.in_files[f])) { fprintf(stderr, "rtk_build_index: cannot open %s\n", o.in_files[f].c_str()); return 1; }
        while (fr.next(name, seq, qual)) fprintf(fo, "@%s\n%s\n+\n%s\n", name.c_str(), seq.c_str(), qual.empty() ? std::string(seq.size(), 'I').c_str() : qual.c_str()); }
    fclose(fo); return 0;
}

// ---- pass 1: the solid k-mers, sorted (unitig construction is independent of table layout): counted on the host threads (common/kmer_count.hpp), or
// with --gpu on the device (csrc/hip/rtk_index.hip, through the C ABI of libratatosk_hip.so next to this executable) ----
template <class KM> static bool count_kmers(IndexBuild<KM>& s) {
    const IndexOptions& o = s.o;
    // the graph of the reads (-s, k-mers seen >= --min-count times), or with --graph-from the graph of a unitig file: every k-mer of its text, once
    // (a compacted graph survives its own FASTA: the unitigs depend on the k-mer set alone). The same route either way.
    const bool from_graph = !o.graph_files.empty();
    const std::vector<std::string>& files = o.graph_inputs(); const unsigned min_count = o.graph_min_count();
    if (s.knobs.trace) { fprintf(stderr, "rtk_build_index: graph from %s", from_graph ? "--graph-from" : "the reads of -s"); for (size_t f = 0; f < files.size(); ++f) fprintf(stderr, " %s", files[f].c_str());
        fprintf(stderr, from_graph ? " (every k-mer of the text is a vertex)\n" : " (k-mers seen >= %u times)\n", min_count); }
    auto nothing_there = [&]() { // a graph file without a window of k bases: no graph to colour, nothing written
        if (!from_graph || !s.solid.empty()) return false;
        std::string names; for (size_t f = 0; f < files.size(); ++f) names += (f ? ", " : "") + files[f];
        fprintf(stderr, "rtk_build_index: no k-mer of length %d in %s\n", s.k, names.c_str()); return true;
    };
    if (!o.gpu) {
        size_t bad_file = 0;
        const int bad = count_kmers_host<KM>(files, s.k, min_count, s.n_thr, s.solid, &bad_file);
        if (bad && from_graph) fprintf(stderr, bad == 2 ? "rtk_build_index: %s ends in a damaged or cut-short gzip stream\n" : "rtk_build_index: cannot open %s\n", files[bad_file].c_str());
        else if (bad) fprintf(stderr, bad == 2 ? "rtk_build_index: an input file ends in a damaged or cut-short gzip stream\n" : "rtk_build_index: cannot open an input file\n");
        return !bad && !nothing_there();
    }
    if (!s.lib.open("rtk_build_index")) return false;
    if (!s.lib.count_kmers || !s.lib.last_error || !s.lib.free) { fprintf(stderr, "rtk_build_index: --gpu: %s lacks the index entry points\n", s.lib.path.c_str()); return false; }
    std::vector<const char*> fp; for (size_t f = 0; f < files.size(); ++f) fp.push_back(files[f].c_str());
    uint64_t* sk = nullptr; uint64_t ns = 0;
    if (s.lib.count_kmers(0, s.k, fp.data(), static_cast<int>(fp.size()), min_count, static_cast<int>(s.n_thr), &sk, &ns) != 0) { fprintf(stderr, "rtk_build_index: --gpu: %s\n", s.lib.last_error()); return false; }
    s.solid.resize(ns);
    if (ns) memcpy(s.solid.data(), sk, sizeof(KM) * ns); // (two-word k-mers: two words each, low word first)
    s.lib.free(sk);
    return !nothing_there();
}

// The unitig FASTA only needs the sequences: with --fast it is compressed on threads of its own while the colours, annotations and records are worked out.
// Groups of unitigs of >= 32 MB of text are gzip MEMBERS of their own (level 6; a concatenation of members is an ordinary gzip file: zlib's gzread, Bifrost's
// reader, reads through them): compressed side by side here and inflated side by side by the loader (common/mgzip.hpp). The same bytes with any number of threads.
static bool gzip_member(const std::vector<Unitig>& U, size_t u0, size_t u1, std::string& out) {
    std::string text; char name[32];
    for (size_t u = u0; u < u1; ++u) { const int nn = snprintf(name, sizeof(name), ">%zu\n", u); text.append(name, static_cast<size_t>(nn)); text += U[u].seq; text.push_back('\n'); }
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    out.resize(deflateBound(&zs, static_cast<uLong>(text.size())) + 64);
    zs.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(text.data())); zs.avail_in = static_cast<uInt>(text.size());
    zs.next_out = reinterpret_cast<Bytef*>(&out[0]); zs.avail_out = static_cast<uInt>(out.size());
    const int rc = deflate(&zs, Z_FINISH); out.resize(out.size() - zs.avail_out); deflateEnd(&zs);
    return rc == Z_STREAM_END;
}
template <class KM> static void write_fasta(IndexBuild<KM>& s) {
    const std::vector<Unitig>& U = s.U; std::atomic<int>& fasta_rc = s.fasta_rc;
    std::vector<size_t> cut(1, 0);
    { size_t bytes = 0; for (size_t u = 0; u < U.size(); ++u) { bytes += U[u].seq.size() + 12; if (bytes >= s.knobs.fasta_member_bytes) { cut.push_back(u + 1); bytes = 0; } } if (cut.back() != U.size() || cut.size() == 1) cut.push_back(U.size()); }
    FILE* fp = fopen(s.o.out_file(".fasta.gz").c_str(), "wb");
    if (!fp) { fasta_rc = 1; return; }
    const size_t n_groups = cut.size() - 1, nt = s.o.fast ? std::min<size_t>(std::max<size_t>(1, s.n_thr / 4), 16) : 1;
    for (size_t g0 = 0; g0 < n_groups && !fasta_rc; g0 += nt) {
        const size_t g1 = std::min(n_groups, g0 + nt);
        std::vector<std::string> out(g1 - g0); std::vector<int> ok(g1 - g0, 0);
        std::vector<std::thread> th;
        for (size_t g = g0 + 1; g < g1; ++g) th.emplace_back([&, g]() { ok[g - g0] = gzip_member(U, cut[g], cut[g + 1], out[g - g0]) ? 1 : 0; });
        ok[0] = gzip_member(U, cut[g0], cut[g0 + 1], out[0]) ? 1 : 0;
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
        for (size_t g = g0; g < g1; ++g) if (!ok[g - g0] || fwrite(out[g - g0].data(), 1, out[g - g0].size(), fp) != out[g - g0].size()) fasta_rc = 1;
    }
    if (fclose(fp) != 0) fasta_rc = 1;
}
template <class KM> static void start_fasta_writer(IndexBuild<KM>& s) { if (s.o.fast) s.fasta_thread = std::thread([&s]() { write_fasta(s); }); }
template <class KM> static bool finish_fasta_writer(IndexBuild<KM>& s) { // (without --fast the file is written here)
    if (s.o.fast) s.fasta_thread.join(); else write_fasta(s);
    if (s.fasta_rc) fprintf(stderr, "rtk_build_index: cannot write fasta.gz\n");
    return !s.fasta_rc;
}

// records are encoded (Roaring containers of the colour sets) by ranges of unitigs on all threads and written in order: the same bytes
template <class KM> static bool write_rtsk(IndexBuild<KM>& s) {
    std::ofstream out(s.o.out_file(".rtsk").c_str(), std::ios::binary);
    const size_t n = s.U.size(); const unsigned n_w = s.o.fast ? s.n_thr : 1u; const size_t per = (n + n_w - 1) / n_w;
    std::vector<std::string> part(n_w);
    parallel_for(n, n_w, [&](size_t b, size_t e, unsigned) {
        std::ostringstream os(std::ios::binary);
        for (size_t u = b; u < e; ++u) {
            RtskRecord r;
            disk_kmer_from_string(s.U[u].seq.c_str(), s.k, r.head);
            r.kmcov = s.kmcov[u]; r.shared = s.shared[u];
            r.global_ids = s.global_ids[u]; r.local_ids = s.local_ids[u]; r.ambiguity_ids = s.ambiguity[u]; r.cycles = s.cycles[u];
            rtsk_write_record(os, r);
        }
        part[per ? b / per : 0] = os.str();
    });
    for (unsigned t = 0; t < n_w; ++t) out.write(part[t].data(), static_cast<std::streamsize>(part[t].size()));
    if (!out.good()) fprintf(stderr, "rtk_build_index: cannot write the .rtsk file\n");
    return out.good();
}

template <class KM> static int run(const IndexOptions& o) {
    IndexBuild<KM> s(o);
    if (!count_kmers(s)) return 1;
    s.lap("k-mers counted");
    fill_table(s);
    s.lap("k-mer table filled");
    build_unitigs(s);
    s.lap("unitigs built");
    if (o.graph_only) { // the unitig FASTA of the full build, and no .rtsk (an earlier one at that path is not touched)
        start_fasta_writer(s);
        if (!finish_fasta_writer(s)) return 1;
        s.lap("files written");
        return 0;
    }
    start_fasta_writer(s);
    if (!colour_and_cover(s)) return 1;
    s.lap("colours and coverage done");
    if (o.merge) { if (!merge_duplicates(s)) return 1; s.lap("duplicates merged"); }
    adjacency_structure(s);
    if (o.subsample) { if (!subsample_colours(s)) return 1; s.lap("colours subsampled"); }
    edge_bits(s);
    s.lap("adjacency and edge bits done");
    const bool cover = !o.cover_files.empty();
    if (cover) { if (!cover_edges(s)) return 1; s.lap("low-coverage edges covered"); }
    if (o.detect_cycles) { short_cycles(s); s.lap("short cycles done"); }
    if (o.detect_snps) { snp_annotations(s); s.lap("SNP annotations done"); }
    colour_split(s);
    s.lap("global / local colour sets done");
    if (!finish_fasta_writer(s) || !write_rtsk(s)) return 1;
    s.lap("files written");
    return 0;
}

int main(int argc, char** argv) {
    IndexOptions o;
    if (const int rc = parse_options(argc, argv, o)) return rc;
    if (!o.dump_input.empty()) return dump_input(o);
    return o.k <= 31 ? run<uint64_t>(o) : run<u128>(o);
}
