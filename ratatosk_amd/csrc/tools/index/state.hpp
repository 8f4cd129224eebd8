// rtk_build_index: the options, the knobs and the state that the steps of the build hand to each other (tools/build_index.cpp lists the steps).
#ifndef RTK_TOOLS_INDEX_STATE_HPP
#define RTK_TOOLS_INDEX_STATE_HPP

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../common/fastx.hpp"
#include "../../common/hip_lib.hpp"
#include "../../common/kmer.hpp"

namespace rtk {

struct IndexOptions {
    std::vector<std::string> in_files;
    std::string prefix = "out";
    int k = 31;
    unsigned min_count = 2;
    size_t min_cov_vertices = 2;
    double global_cov_factor = 3.0, min_color_sharing = 0.5;
    bool detect_cycles = true, detect_snps = false;
    bool fast = false, gpu = false; // --fast: the same files from thread-parallel counting-table build / compaction / adjacency / cycle search; --gpu: --fast with counting, unitigs and colours on the device (any odd k <= 63)
    std::string dump_input; // --dump-input FILE: the inputs (sample: sources included) written out as one FASTQ file, nothing else done
    bool subsample = false; uint64_t subsample_seed = 1; // --subsample-colours [--subsample-seed N]: the colours thinned out by coverage (tools/index/subsample.hpp)
    bool merge = false; // --merge-duplicates: read pairs on the same unitigs share one colour id (tools/index/merge.hpp)
    std::vector<std::string> colour_files; // pass-2 index (`Ratatosk index -2`): colours = ids of these (pass-1 corrected long) reads, one id per read
    // --colour-min-conf M / --colour-max-qual Q / --colour-min-len N (only with --colour-reads; tools/index/colour_filter.hpp has the rule): min_conf < 0 = not given
    double colour_min_conf = -1.0; int colour_max_qual = 40; uint64_t colour_min_len = 0;
    // --graph-from FILE: the graph is every k-mer of the text of these FASTA files (the unitig file of an earlier build, of any k), each once; -s then only colours and covers
    std::vector<std::string> graph_files;
    // --cover-edges-from FILE: the edges that fewer than min_cov_vertices colours share get two fresh ids on both ends wherever a sequence of these FASTA files (the unitigs of the k2 graph) walks over them (tools/index/cover.hpp)
    std::vector<std::string> cover_files;
    bool pair_by_name = false; // --pair-by-name: the id of a short read is the rank of its name by first appearance over all -s files, so that mates in separate files share it (tools/index/colour.hpp; DESIGN.md section 4 [A18])
    bool graph_only = false; // --graph-only: count, table, unitigs, the unitig FASTA written, nothing else
    // what the graph is counted from, and how often a k-mer must be seen there
    const std::vector<std::string>& graph_inputs() const { return graph_files.empty() ? in_files : graph_files; }
    unsigned graph_min_count() const { return graph_files.empty() ? min_count : 1u; }
    std::string out_file(const char* ext) const { return prefix + ".index.k" + std::to_string(k) + ext; }
};

// 0, or the exit status (2: the message or the usage text is on stderr)
inline int parse_options(int argc, char** argv, IndexOptions& o) {
    bool seed_given = false, min_count_given = false; const char* filter_given = nullptr;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* n) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "rtk_build_index: missing value for %s\n", n); exit(2); } return argv[++i]; };
        if (a == "-s") o.in_files.push_back(need("-s"));
        else if (a == "-o") o.prefix = need("-o");
        else if (a == "-k") o.k = atoi(need("-k"));
        else if (a == "--min-count") { o.min_count = static_cast<unsigned>(atoi(need("--min-count"))); min_count_given = true; }
        else if (a == "--graph-from") o.graph_files.push_back(need("--graph-from"));
        else if (a == "--graph-only") o.graph_only = true;
        else if (a == "--cover-edges-from") o.cover_files.push_back(need("--cover-edges-from"));
        else if (a == "--global-cov-factor") o.global_cov_factor = atof(need("--global-cov-factor"));
        else if (a == "--no-short-cycles") o.detect_cycles = false;
        else if (a == "--snps") o.detect_snps = true;
        else if (a == "--fast") o.fast = true;
        else if (a == "--gpu") { o.fast = true; o.gpu = true; }
        else if (a == "--colour-reads") o.colour_files.push_back(need("--colour-reads"));
        else if (a == "--subsample-colours") o.subsample = true;
        else if (a == "--merge-duplicates") o.merge = true;
        else if (a == "--pair-by-name") o.pair_by_name = true;
        else if (a == "--subsample-seed") { const char* v = need("--subsample-seed"); char* end = nullptr; o.subsample_seed = strtoull(v, &end, 10); seed_given = true;
            if (*v < '0' || *v > '9' || *end) { fprintf(stderr, "rtk_build_index: --subsample-seed takes an unsigned number, not '%s'\n", v); return 2; } }
        else if (a == "--colour-min-conf") { const char* v = need("--colour-min-conf"); char* end = nullptr; o.colour_min_conf = strtod(v, &end); filter_given = "--colour-min-conf";
            if (end == v || *end || !(o.colour_min_conf >= 0.0 && o.colour_min_conf <= 1.0)) { fprintf(stderr, "rtk_build_index: --colour-min-conf takes a number in [0, 1], not '%s'\n", v); return 2; } }
        else if (a == "--colour-max-qual") { const char* v = need("--colour-max-qual"); char* end = nullptr; const long q = strtol(v, &end, 10); filter_given = "--colour-max-qual";
            if (end == v || *end || q < 1 || q > 93) { fprintf(stderr, "rtk_build_index: --colour-max-qual takes a number in 1 .. 93, not '%s'\n", v); return 2; } o.colour_max_qual = static_cast<int>(q); }
        else if (a == "--colour-min-len") { const char* v = need("--colour-min-len"); char* end = nullptr; o.colour_min_len = strtoull(v, &end, 10); filter_given = "--colour-min-len";
            if (*v < '0' || *v > '9' || *end) { fprintf(stderr, "rtk_build_index: --colour-min-len takes an unsigned number, not '%s'\n", v); return 2; } }
        else if (a == "--dump-input") o.dump_input = need("--dump-input");
        else { fprintf(stderr, "rtk_build_index: unknown option %s\n", a.c_str()); return 2; }
    }
    if (o.graph_only) { // the graph and nothing else: whatever colours, annotates or takes the graph from elsewhere clashes with it
        const char* clash = o.detect_snps ? "--snps" : !o.colour_files.empty() ? "--colour-reads" : filter_given ? filter_given : o.merge ? "--merge-duplicates" : (o.subsample || seed_given) ? "--subsample-colours" : o.pair_by_name ? "--pair-by-name" : !o.graph_files.empty() ? "--graph-from" : !o.cover_files.empty() ? "--cover-edges-from" : nullptr;
        if (clash) { fprintf(stderr, "rtk_build_index: --graph-only writes the unitig FASTA and stops: %s does not go with it\n", clash); return 2; }
    }
    if (o.pair_by_name && !o.colour_files.empty()) { fprintf(stderr, "rtk_build_index: --pair-by-name next to --colour-reads: the long reads colour, one id each, and there is nothing to pair\n"); return 2; }
    for (size_t f = 0; o.pair_by_name && f < o.in_files.size(); ++f) if (SampleSource::is_spec(o.in_files[f])) {
        fprintf(stderr, "rtk_build_index: --pair-by-name with the source %s: the pairs of a sample: source are numbered by construction, and its names repeat from source to source\n", o.in_files[f].c_str()); return 2; }
    if (!o.cover_files.empty() && !o.colour_files.empty()) { fprintf(stderr, "rtk_build_index: --cover-edges-from next to --colour-reads: the low-coverage edges are covered in a first-pass index only (the reference skips the step when the long reads colour)\n"); return 2; }
    for (size_t f = 0; f < o.cover_files.size(); ++f) { FILE* fp = fopen(o.cover_files[f].c_str(), "rb"); if (!fp) { fprintf(stderr, "rtk_build_index: --cover-edges-from: cannot open %s\n", o.cover_files[f].c_str()); return 2; } fclose(fp); }
    if (!o.graph_files.empty() && min_count_given) { fprintf(stderr, "rtk_build_index: --min-count next to --graph-from: every k-mer of a graph file is a vertex (the reads of -s only colour), so there is nothing it could count\n"); return 2; }
    if (!o.graph_files.empty() && o.in_files.empty() && o.colour_files.empty()) { fprintf(stderr, "rtk_build_index: --graph-from needs reads that colour the graph: -s or --colour-reads\n"); return 2; }
    if (seed_given && !o.subsample) { fprintf(stderr, "rtk_build_index: --subsample-seed without --subsample-colours\n"); return 2; }
    if (filter_given && o.colour_files.empty()) { fprintf(stderr, "rtk_build_index: %s without --colour-reads\n", filter_given); return 2; }
    const bool graph_given = !o.graph_files.empty() && !o.colour_files.empty(); // (the one case without -s: the graph from a file, the colours from --colour-reads)
    if ((o.in_files.empty() && !graph_given) || o.k < 3 || o.k > RTK_MAX_K || !(o.k & 1)) { fprintf(stderr, "usage: rtk_build_index -s reads.fq [-s ...] -o PREFIX [-k 31 (odd, <=63)] [--min-count 2] [--global-cov-factor 3.0] [--no-short-cycles] [--snps] [--fast | --gpu (k <= 63: same files, threads / the device for the heavy steps)] [--dump-input FILE] [--subsample-colours [--subsample-seed 1 (only with --subsample-colours)]: colours subsampled by coverage as the reference's index step does by default] [--merge-duplicates: read pairs that lie on the same unitigs share one colour id, as the reference's index step merges duplicated reads (no effect with --colour-reads)] [--colour-reads corrected_long_reads.fq: second-pass index, the graph comes from -s, colours and coverage from these reads [--colour-min-conf M (0 .. 1): a base of these reads whose quality is below that of confidence M colours nothing, as the reference's second-pass index does with -M (0: the '!' bases); needs FASTQ] [--colour-max-qual 40: the quality that stands for confidence 1 (-Q)] [--colour-min-len N: a read of fewer than N bases colours nothing (-C); these three only with --colour-reads]] [--graph-only: the unitig FASTA (PREFIX.index.kK.fasta.gz, the bytes of the full build) and nothing else, no .rtsk; not with --snps, --colour-reads, --merge-duplicates, --subsample-colours, --graph-from] [--graph-from unitigs.fasta.gz (may be repeated; FASTA as -s reads it): the graph is every all-A/C/G/T window of length k of these records, each once, whatever the k the file was written with (a k above the file's own: the windows of that length inside its unitigs); -s then only colours and covers, and is not needed next to --colour-reads; not with --min-count] [--cover-edges-from k2_unitigs.fasta.gz (may be repeated; FASTA, plain or gzip, of any k): every edge whose two unitigs share fewer than 2 colours gets two fresh colour ids on both unitigs wherever a sequence of the file walks over it, in the order of the file, as the reference's first-pass index covers its low-coverage edges from the k2 unitigs; the annotations see the ids, the edge bits and the coverage stay; not with --colour-reads, --graph-only] [--pair-by-name: the colour id of a short read is the rank of its NAME (the header up to the first blank, without a trailing /1 or /2) by first appearance over all -s files in the order given, as the reference numbers its pairs, so that mates share one id wherever their records lie (-s R1.fastq -s R2.fastq); without it the id is the number of name changes before the read, which pairs the mates of an interleaved file only; an interleaved file gets the same ids either way; not with --colour-reads, --graph-only, sample: sources]\n"); return 2; }
    return 0;
}

// the environment knobs of the tool (listed at the end of hip/rtk_knobs.h), read once
struct IndexKnobs {
    bool trace = getenv("RTK_INDEX_TRACE") != nullptr;                 // the laps and the step counts on stderr
    bool host_unitigs = getenv("RTK_INDEX_HOST_UNITIGS") != nullptr;   // --gpu: the chains on the host threads
    bool host_colours = getenv("RTK_INDEX_HOST_COLOURS") != nullptr;   // --gpu: the colours on the host threads
    bool snps_device = true;                                           // RTK_INDEX_SNPS=device|host: --gpu --snps finds its candidates on the device (unset: device) or on the host threads; ignored without --gpu
    unsigned threads = 0;                                              // RTK_INDEX_THREADS (0: by the machine)
    size_t fasta_member_bytes = 32u << 20;                             // RTK_FASTA_MEMBER_BYTES (tests: many small members)
    IndexKnobs() {
        if (const char* e = getenv("RTK_INDEX_THREADS")) if (atoi(e) > 0) threads = static_cast<unsigned>(atoi(e));
        if (const char* e = getenv("RTK_INDEX_SNPS")) { if (!strcmp(e, "host")) snps_device = false; else if (!strcmp(e, "device")) snps_device = true; }
        if (const char* e = getenv("RTK_FASTA_MEMBER_BYTES")) fasta_member_bytes = static_cast<size_t>(strtoull(e, nullptr, 10));
    }
};

// open-addressing table from canonical k-mers (one- or two-word codes) to a 64-bit value; the all-ones key is no k-mer (odd k <= 63) and marks a free slot
template <class KM> struct KTable {
    const KM EMPTY = ~static_cast<KM>(0);
    std::vector<KM> keys; std::vector<uint64_t> vals;
    size_t n = 0, mask = 0;
    explicit KTable(size_t cap_pow2 = 1 << 20) { reset(cap_pow2); }
    void reset(size_t cap_pow2) { keys.assign(cap_pow2, EMPTY); vals.assign(cap_pow2, 0); mask = cap_pow2 - 1; n = 0; }
    void grow() {
        std::vector<KM> ok; std::vector<uint64_t> ov; ok.swap(keys); ov.swap(vals);
        keys.assign(ok.size() * 2, EMPTY); vals.assign(ok.size() * 2, 0); mask = keys.size() - 1; n = 0;
        for (size_t i = 0; i < ok.size(); ++i) if (ok[i] != EMPTY) *slot(ok[i], true) = ov[i];
    }
    uint64_t* slot(KM key, bool insert) {
        if (insert && (n + 1) * 10 > keys.size() * 6) grow();
        size_t i = hash_km(key) & mask;
        while (true) {
            if (keys[i] == key) return &vals[i];
            if (keys[i] == EMPTY) { if (!insert) return nullptr; keys[i] = key; ++n; return &vals[i]; }
            i = (i + 1) & mask;
        }
    }
};

template <class F> static void parallel_for(size_t n, unsigned n_thr, F f) { // f(begin, end, thread)
    if (n_thr < 1) n_thr = 1;
    std::vector<std::thread> th; const size_t per = (n + n_thr - 1) / n_thr;
    for (unsigned t = 0; t < n_thr; ++t) { const size_t b = std::min(n, per * t), e = std::min(n, per * (t + 1)); if (b < e) th.emplace_back([=]() { f(b, e, t); }); }
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
}

struct Unitig { std::string seq; std::vector<uint32_t> colours; uint64_t cov = 0; };
struct Nb { int64_t u[2][4]; }; // [dir 0 = fw successors, 1 = successors of the reverse strand][base] -> unitig id or -1

inline size_t shared_count(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
    size_t i = 0, j = 0, c = 0;
    while (i < a.size() && j < b.size()) { if (a[i] < b[j]) ++i; else if (b[j] < a[i]) ++j; else { ++c; ++i; ++j; } }
    return c;
}

template <class KM> struct IndexBuild { // KM: uint64_t for k <= 31, u128 for k in 33..63
    const IndexOptions& o; const IndexKnobs knobs; HipLib lib; // (lib: loaded with --gpu only)
    const int k; const KM mask; unsigned n_thr;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    std::vector<KM> solid;          // the canonical k-mers seen >= --min-count times, sorted
    KTable<KM> km;                  // canonical solid k-mer -> 0 (unvisited) or (unitig+1)<<32 | offset<<1 | fw_flag
    std::vector<Unitig> U;
    std::vector<KM> headk, tailk;   // per unitig (from the adjacency step on): first and last k-mer,
    std::vector<Nb> adj; std::vector<uint64_t> kmcov, shared; // neighbours, coverage + branching bit, edge bits (+ 0x100: in a short cycle)
    std::vector<std::string> cycles;
    std::vector<std::vector<uint32_t> > ambiguity, global_ids, local_ids;
    std::vector<std::vector<uint32_t> > cover_ids; // --cover-edges-from: the ids the covering step added, per unitig (also the last of its colours: colour_split leaves that many out and puts them into the local set)
    std::shared_ptr<void> colour_sink; // --gpu --subsample-colours / --merge-duplicates: the ColourSink whose job still holds the events on the device
    std::thread fasta_thread; std::atomic<int> fasta_rc; // --fast: the unitig FASTA is compressed beside the other steps
    explicit IndexBuild(const IndexOptions& opt) : o(opt), k(opt.k), mask(km_mask<KM>(opt.k)), km(16), fasta_rc(0) {
        n_thr = std::thread::hardware_concurrency(); if (n_thr == 0) n_thr = 1; if (n_thr > (o.fast ? 128u : 32u)) n_thr = o.fast ? 128u : 32u; // (--fast: the steps are random accesses into GB-sized tables: latency-bound, SMT threads help)
        if (knobs.threads) n_thr = knobs.threads;
    }
    ~IndexBuild() { if (fasta_thread.joinable()) fasta_thread.join(); } // (whoever leaves early leaves through here: the writer reads U)
    void lap(const char* what) const { if (knobs.trace) fprintf(stderr, "rtk_build_index: [%8.2f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), what); }
    // the oriented neighbours of an oriented k-mer that are in the graph
    bool in_graph(KM oriented) { return km.slot(kmer_canonical(oriented, k), false) != nullptr; }
    int succs(KM x, KM out[4]) { int n = 0; for (uint64_t b = 0; b < 4; ++b) { const KM y = ((x << 2) | static_cast<KM>(b)) & mask; if (in_graph(y)) out[n++] = y; } return n; }
    int preds(KM x, KM out[4]) { int n = 0; for (uint64_t b = 0; b < 4; ++b) { const KM y = (x >> 2) | (static_cast<KM>(b) << (2 * (k - 1))); if (in_graph(y)) out[n++] = y; } return n; }
};

} // namespace rtk

#endif
