// rtk_chunks_step: the two host steps of the device side's k-mer count (hip/rtk_index_count.h) on inputs given by hand -- the threaded readers that hand the
// sequences of the read files out in chunks (common/sequence_chunks.hpp) and the threaded merge of the sorted partitions (common/sorted_runs.hpp). Host code only.
//   rtk_chunks_step chunks FILES... --threads T --chunk-bytes B [--reader]
//       stdout: every sequence the sink was handed, one per line (the order is free across chunks, file order within a chunk). --reader: the sequences as
//       FastxReader gives them, one after the other, in place of the chunked readers (what the tests compare with).
//   rtk_chunks_step merge --k K --threads T < runs.txt
//       runs.txt: a line "run" opens a run (there may be none, or empty ones); every other line is one key of the open run, a 2K-bit code in hexadecimal,
//       ascending and distinct within the run. stdout: the merged keys, one per line, in the same form.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "../common/sequence_chunks.hpp"
#include "../common/sorted_runs.hpp"

using namespace rtk;

static int usage() {
    fprintf(stderr, "usage: rtk_chunks_step chunks FILES... --threads T --chunk-bytes B [--reader]\n       rtk_chunks_step merge --k K(odd, 3 .. 63) --threads T < runs.txt (\"run\" lines and hexadecimal keys)\n");
    return 2;
}

static int chunks(const std::vector<std::string>& files, int threads, uint64_t chunk_bytes, bool reader) {
    if (reader) {
        for (size_t f = 0; f < files.size(); ++f) {
            FastxReader rd; if (!rd.open(files[f], 1)) { fprintf(stderr, "rtk_chunks_step: cannot open %s\n", files[f].c_str()); return 1; }
            std::string name, seq, qual;
            while (rd.next(name, seq, qual)) { fwrite(seq.data(), 1, seq.size(), stdout); fputc('\n', stdout); }
            if (rd.failed()) { fprintf(stderr, "rtk_chunks_step: %s ends in a damaged or cut-short gzip stream\n", files[f].c_str()); return 1; }
        }
        return 0;
    }
    std::string err;
    if (!for_each_sequence_chunk(files, threads, chunk_bytes, [](const char* chars, size_t n) { fwrite(chars, 1, n, stdout); }, &err)) { fprintf(stderr, "rtk_chunks_step: %s\n", err.c_str()); return 1; }
    return 0;
}

template <class KM> static bool parse_key(const std::string& s, int k, KM* out) {
    if (s.empty() || s.size() > 32) return false;
    unsigned __int128 v = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        const char c = s[i]; const int d = c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : (c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1));
        if (d < 0) return false;
        v = (v << 4) | static_cast<unsigned __int128>(d);
    }
    if (v >> (2 * k)) return false;
    *out = static_cast<KM>(v); return true;
}

template <class KM> static int merge(int k, int threads) {
    std::vector<KM> solid; std::vector<size_t> run_start; std::string line;
    while (std::getline(std::cin, line)) {
        if (line == "run") { run_start.push_back(solid.size()); continue; }
        KM v = 0;
        if (run_start.empty() || !parse_key<KM>(line, k, &v)) { fprintf(stderr, "rtk_chunks_step: '%s' is no key of 2 * %d bits inside a run\n", line.c_str(), k); return 2; }
        if (solid.size() > run_start.back() && solid.back() >= v) { fprintf(stderr, "rtk_chunks_step: the keys of a run are not ascending and distinct\n"); return 2; }
        solid.push_back(v);
    }
    std::vector<KM> out(solid.size() ? solid.size() : 1);
    merge_sorted_runs<KM>(solid, run_start, k, threads, out.data());
    for (size_t i = 0; i < solid.size(); ++i) {
        const unsigned __int128 v = out[i]; const uint64_t hi = static_cast<uint64_t>(v >> 64), lo = static_cast<uint64_t>(v);
        if (hi) printf("%llx%016llx\n", static_cast<unsigned long long>(hi), static_cast<unsigned long long>(lo)); else printf("%llx\n", static_cast<unsigned long long>(lo));
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    std::vector<std::string> files; int threads = 0, k = 0; uint64_t chunk_bytes = 0; bool reader = false;
    for (int i = 2; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--reader") reader = true;
        else if (a == "--threads" && i + 1 < argc) threads = atoi(argv[++i]);
        else if (a == "--chunk-bytes" && i + 1 < argc) chunk_bytes = strtoull(argv[++i], nullptr, 10);
        else if (a == "--k" && i + 1 < argc) k = atoi(argv[++i]);
        else if (a.compare(0, 2, "--") == 0) return usage();
        else files.push_back(a);
    }
    if (threads < 1) return usage();
    if (mode == "chunks") { if (files.empty() || chunk_bytes < 1 || k) return usage(); return chunks(files, threads, chunk_bytes, reader); }
    if (mode == "merge") { if (!files.empty() || chunk_bytes || reader || k < 3 || k > 63 || !(k & 1)) return usage(); return k <= 31 ? merge<uint64_t>(k, threads) : merge<unsigned __int128>(k, threads); }
    return usage();
}
