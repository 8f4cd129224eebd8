// rtk_qv: the k-mer QV of reads against the k-mers of the short reads ([A17]; no counterpart in the reference: the measure is Merqury's).
// Of the start positions of a read whose K characters are all A/C/G/T (`windows`), how many spell a canonical K-mer of the set (`found`). The set is the K-mers
// seen at least --min-count times in the -s files, or every K-mer of the records of -g (the unitig file of an index). From the share found follow the per-base
// error rate 1 - (found / windows)^(1/K) and its Phred value: one row per -l file in OUT.qv.tsv, with --per-read one row per read in OUT.qv.reads.tsv.
//   plain    k-mers counted (common/kmer_count.hpp) and reads tested on the host threads (no GPU, no library): bisection in the sorted set
//   --gpu    the count from rtk_index_count_kmers, the test through rtk_qv_begin / _chunk / _end of libratatosk_hip.so next to this executable
// Both write the same bytes: the rows are computed by one function from the same integers.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../common/fastx.hpp"
#include "../common/hip_lib.hpp"
#include "../common/kmer.hpp"
#include "../common/kmer_count.hpp"

using namespace rtk;

// pieces in the chunk layout of rtk_qv_chunk: separated by '\n'; piece p belongs to read read_of[p] of its task
struct Sub { std::string chars; std::vector<uint64_t> starts; std::vector<uint32_t> read_of; };
// reads of one -l file, in input order: mostly one Sub; a read longer than a chunk is a task of its own with one Sub per piece
struct Task { size_t id = 0, file = 0; std::vector<Sub> subs; std::string names; std::vector<uint64_t> name_off, lens; size_t n() const { return lens.size(); } };
struct Totals { unsigned long long reads = 0, bases = 0, windows = 0, found = 0; };

// error_rate and qv of a row, as text (both routes, from the same integers)
static void row_figures(unsigned long long windows, unsigned long long found, int k, std::string& error_rate, std::string& qv) {
    if (windows == 0) { error_rate = "nan"; qv = "nan"; return; }
    if (found == windows) { error_rate = "0"; qv = "inf"; return; }
    const double e = 1.0 - pow(static_cast<double>(found) / static_cast<double>(windows), 1.0 / k);
    char b[64]; snprintf(b, sizeof(b), "%.6g", e); error_rate = b;
    snprintf(b, sizeof(b), "%.2f", -10.0 * log10(e) + 0.0); qv = b; // (+ 0.0: an error rate of 1 is QV 0.00, not -0.00)
}

static int usage() {
    fprintf(stderr, "usage: rtk_qv (-s short_reads.fq [-s ...] [--min-count 2] | -g graph.fasta[.gz]) -l reads.fq [-l ...] -k K (odd, <= 31) -o OUT [--gpu] [--per-read] [-v]\n"
                    "  writes OUT.qv.tsv: per -l file the start positions whose K characters are all A/C/G/T (windows), those whose K-mer occurs at least --min-count times in\n"
                    "  the -s reads -- or at all in the records of -g -- (found), error_rate = 1 - (found / windows)^(1/K) and qv = -10 log10(error_rate);\n"
                    "  --per-read: OUT.qv.reads.tsv as well, one row per read\n");
    return 2;
}

int main(int argc, char** argv) {
    std::vector<std::string> in_short, in_graph, in_long;
    std::string prefix; int k = 31; long long min_count = -1; bool gpu = false, verbose = false, per_read = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* n) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "rtk_qv: missing value for %s\n", n); exit(2); } return argv[++i]; };
        auto add = [&](std::vector<std::string>& v, const char* fn) { std::vector<std::string> l = expand_input_list(fn); if (l.empty()) l.push_back(fn); v.insert(v.end(), l.begin(), l.end()); }; // (a text file lists one path per line; an empty file is a file without reads)
        if (a == "-s") add(in_short, need("-s"));
        else if (a == "-g") add(in_graph, need("-g"));
        else if (a == "-l") add(in_long, need("-l"));
        else if (a == "-o") prefix = need("-o");
        else if (a == "-k") k = atoi(need("-k"));
        else if (a == "--min-count") { const char* v = need("--min-count"); char* end = nullptr; min_count = strtoll(v, &end, 10); if (end == v || *end || min_count < 1 || min_count > 0xFFFFFFFFll) { fprintf(stderr, "rtk_qv: --min-count takes a number >= 1, not '%s'\n", v); return 2; } }
        else if (a == "--gpu") gpu = true;
        else if (a == "--per-read") per_read = true;
        else if (a == "-v") verbose = true;
        else { fprintf(stderr, "rtk_qv: unknown option %s\n", a.c_str()); return usage(); }
    }
    if (!in_short.empty() && !in_graph.empty()) { fprintf(stderr, "rtk_qv: -s and -g exclude each other: the set is counted from the short reads or taken from the unitigs of an index\n"); return usage(); }
    if (!in_graph.empty() && min_count >= 0) { fprintf(stderr, "rtk_qv: --min-count belongs to -s: every K-mer of the records of -g is in the set\n"); return usage(); }
    if (in_short.empty() && in_graph.empty()) { fprintf(stderr, "rtk_qv: no k-mer set: give -s or -g\n"); return usage(); }
    if (in_long.empty()) { fprintf(stderr, "rtk_qv: no reads: give -l\n"); return usage(); }
    if (prefix.empty()) { fprintf(stderr, "rtk_qv: no output prefix: give -o\n"); return usage(); }
    if (k < 3 || k > 31 || !(k & 1)) { fprintf(stderr, "rtk_qv: K must be odd and <= 31 (one-word k-mers)\n"); return usage(); }
    const std::vector<std::string>& in_set = in_graph.empty() ? in_short : in_graph;
    const unsigned set_min = in_graph.empty() ? static_cast<unsigned>(min_count < 0 ? 2 : min_count) : 1u;
    for (int g = 0; g < 2; ++g) { const std::vector<std::string>& v = g == 0 ? in_set : in_long; // (before any counting)
        for (size_t f = 0; f < v.size(); ++f) if (!SampleSource::is_spec(v[f]) && access(v[f].c_str(), R_OK) != 0) { fprintf(stderr, "rtk_qv: cannot open %s\n", v[f].c_str()); return 1; } }
    const std::string fn_out = prefix + ".qv.tsv", fn_reads = prefix + ".qv.reads.tsv";
    const bool trace = getenv("RTK_INDEX_TRACE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (trace || verbose) fprintf(stderr, "rtk_qv: [%8.2f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), what); };
    unsigned n_thr = std::thread::hardware_concurrency(); if (n_thr == 0) n_thr = 1; if (n_thr > 32u) n_thr = 32u;
    { const char* e = getenv("RTK_INDEX_THREADS"); if (e && atoi(e) > 0) n_thr = static_cast<unsigned>(atoi(e)); }
    size_t chunk_chars = 48u << 20; // characters of -l text per chunk (RTK_INDEX_CHUNK: tests force several small chunks and reads cut into pieces)
    { const char* e = getenv("RTK_INDEX_CHUNK"); if (e && strtoull(e, nullptr, 10) >= 1024) chunk_chars = std::min<size_t>(strtoull(e, nullptr, 10), 60u << 20); }
    const size_t chunk_reads = 2u << 20, max_piece = chunk_chars - 1; // (a piece and its separator fill a chunk at the most)

    HipLib lib; HipLib::qv_begin_fn g_begin = nullptr; HipLib::qv_chunk_fn g_chunk = nullptr; HipLib::qv_end_fn g_end = nullptr;
    if (gpu) {
        if (!lib.open("rtk_qv")) return 1;
        if (!lib.count_kmers || !lib.get(g_begin, "rtk_qv_begin") || !lib.get(g_chunk, "rtk_qv_chunk") || !lib.get(g_end, "rtk_qv_end") || !lib.last_error || !lib.free) { fprintf(stderr, "rtk_qv: --gpu: %s lacks the qv entry points\n", lib.path.c_str()); return 1; }
    }

    // ---- the set
    std::vector<uint64_t> solid;
    if (!gpu) {
        size_t f = 0; const int bad = count_kmers_host<uint64_t>(in_set, k, set_min, n_thr, solid, &f);
        if (bad) { fprintf(stderr, bad == 2 ? "rtk_qv: %s ends in a damaged or cut-short gzip stream\n" : "rtk_qv: cannot open %s\n", in_set[f].c_str()); return 1; }
    } else {
        std::vector<const char*> fp; for (size_t f = 0; f < in_set.size(); ++f) fp.push_back(in_set[f].c_str());
        uint64_t* sk = nullptr; uint64_t ns = 0;
        if (lib.count_kmers(0, k, fp.data(), static_cast<int>(fp.size()), set_min, static_cast<int>(n_thr), &sk, &ns) != 0) { fprintf(stderr, "rtk_qv: --gpu: %s\n", lib.last_error()); return 1; }
        solid.assign(sk, sk + ns); lib.free(sk);
    }
    lap("count");
    if (trace || verbose) fprintf(stderr, "rtk_qv: %zu %d-mers in the set (%s, count >= %u)\n", solid.size(), k, in_graph.empty() ? "-s" : "-g", set_min);
    void* job = nullptr;
    if (gpu) {
        if (g_begin(0, k, solid.data(), solid.size(), &job) != 0) { fprintf(stderr, "rtk_qv: --gpu: %s\n", lib.last_error()); return 1; }
        std::vector<uint64_t>().swap(solid); // (the table lives on the device)
    }
    lap("table");

    // ---- the reads: one dispatcher thread reads the -l files in order and lays chunks out, the threads test them (--gpu: on the device, two calls side by side; else
    // on the host), and the per-read rows are written in input order
    FILE* fr_out = nullptr;
    if (per_read) { fr_out = fopen(fn_reads.c_str(), "wb"); if (!fr_out) { fprintf(stderr, "rtk_qv: cannot write %s\n", fn_reads.c_str()); if (job) g_end(job, nullptr, nullptr); return 1; } fputs("file_index\tname\tlength\twindows\tfound\n", fr_out); }
    else unlink(fn_reads.c_str()); // (a file of an earlier run is not this run's result)
    std::mutex mq, m_out, m_err; std::condition_variable cv_put, cv_get, cv_out; std::deque<std::unique_ptr<Task> > q; bool done = false; std::atomic<bool> stop(false);
    std::string first_err; auto fail = [&](const std::string& msg) { { std::lock_guard<std::mutex> lk(m_err); if (first_err.empty()) first_err = msg; } stop = true; { std::lock_guard<std::mutex> lk(mq); } cv_put.notify_all(); cv_get.notify_all(); { std::lock_guard<std::mutex> lk(m_out); } cv_out.notify_all(); };
    std::vector<Totals> totals(in_long.size());
    size_t next_to_write = 0; std::vector<std::pair<size_t, std::string> > waiting; // formatted blocks that wait for the ones before them
    const size_t ahead = 2 * static_cast<size_t>(n_thr) + 4;
    std::thread dispatcher([&]() {
        size_t id = 0;
        auto put = [&](std::unique_ptr<Task>& t) { t->id = id++; std::unique_lock<std::mutex> lk(mq); cv_put.wait(lk, [&]() { return q.size() < ahead || stop.load(); }); if (stop) return; q.push_back(std::move(t)); cv_get.notify_one(); };
        for (size_t f = 0; f < in_long.size() && !stop; ++f) {
            FastxReader fr; std::string name, seq, qual;
            if (!fr.open(in_long[f], static_cast<int>(std::min(n_thr, 16u)))) { fail("cannot open " + in_long[f]); break; }
            std::unique_ptr<Task> t;
            auto fresh = [&]() { t.reset(new Task()); t->file = f; };
            auto add_read = [&]() { t->name_off.push_back(t->names.size()); t->names += name; t->lens.push_back(seq.size()); };
            fresh();
            while (!stop && fr.next(name, seq, qual)) {
                if (seq.size() > max_piece) { // cut with an overlap of k - 1: every window lies whole in exactly one piece
                    if (t->n()) { put(t); fresh(); }
                    add_read();
                    for (size_t a = 0;; a += max_piece - static_cast<size_t>(k - 1)) {
                        t->subs.emplace_back(); Sub& s = t->subs.back();
                        s.starts.push_back(0); s.read_of.push_back(0); s.chars.assign(seq, a, max_piece); s.chars.push_back('\n');
                        if (a + max_piece >= seq.size()) break;
                    }
                    put(t); fresh();
                    continue;
                }
                if (t->n() && (t->subs[0].chars.size() + seq.size() + 1 > chunk_chars || t->n() >= chunk_reads)) { put(t); fresh(); }
                if (t->subs.empty()) t->subs.emplace_back();
                Sub& s = t->subs[0];
                s.starts.push_back(s.chars.size()); s.read_of.push_back(static_cast<uint32_t>(t->n())); s.chars += seq; s.chars.push_back('\n');
                add_read();
            }
            if (!stop && fr.failed()) fail(in_long[f] + " ends in a damaged or cut-short gzip stream");
            if (!stop && t->n()) put(t);
        }
        { std::lock_guard<std::mutex> lk(mq); done = true; } cv_get.notify_all();
    });
    auto worker = [&]() {
        std::string block; std::vector<uint32_t> pw, pf; std::vector<unsigned long long> rw, rf;
        for (;;) {
            std::unique_ptr<Task> t;
            { std::unique_lock<std::mutex> lk(mq); cv_get.wait(lk, [&]() { return !q.empty() || done || stop.load(); }); if (stop || q.empty()) return; t = std::move(q.front()); q.pop_front(); }
            cv_put.notify_one();
            { std::unique_lock<std::mutex> lk(m_out); cv_out.wait(lk, [&]() { return t->id < next_to_write + ahead || stop.load(); }); if (stop) return; } // bounded run-ahead of the writer
            const size_t n = t->n(); rw.assign(n, 0); rf.assign(n, 0);
            for (size_t u = 0; u < t->subs.size(); ++u) {
                const Sub& s = t->subs[u]; const size_t np = s.starts.size();
                pw.assign(np, 0); pf.assign(np, 0);
                if (gpu) { if (g_chunk(job, s.chars.data(), s.chars.size(), s.starts.data(), static_cast<uint32_t>(np), pw.data(), pf.data()) != 0) { fail(std::string("--gpu: ") + lib.last_error()); return; } }
                else for (size_t p = 0; p < np; ++p) { const size_t e = (p + 1 < np ? s.starts[p + 1] : s.chars.size()) - 1; // (without the separator)
                    uint32_t w = 0, fd = 0;
                    for_each_canonical_kmer<uint64_t>(s.chars.data() + s.starts[p], e - s.starts[p], k, kmer_mask(k), [&](uint64_t c, size_t) { ++w; if (std::binary_search(solid.begin(), solid.end(), c)) ++fd; });
                    pw[p] = w; pf[p] = fd; }
                for (size_t p = 0; p < np; ++p) { rw[s.read_of[p]] += pw[p]; rf[s.read_of[p]] += pf[p]; }
            }
            Totals add; add.reads = n; block.clear(); t->name_off.push_back(t->names.size());
            for (size_t r = 0; r < n; ++r) {
                add.bases += t->lens[r]; add.windows += rw[r]; add.found += rf[r];
                if (per_read) { block += std::to_string(t->file); block += '\t'; block.append(t->names, t->name_off[r], t->name_off[r + 1] - t->name_off[r]); block += '\t'; block += std::to_string(t->lens[r]); block += '\t';
                    block += std::to_string(rw[r]); block += '\t'; block += std::to_string(rf[r]); block += '\n'; }
            }
            std::unique_lock<std::mutex> lk(m_out); // blocks leave in task order: whoever holds the next one writes it and those that waited for it
            Totals& T = totals[t->file]; T.reads += add.reads; T.bases += add.bases; T.windows += add.windows; T.found += add.found;
            waiting.emplace_back(t->id, std::string()); waiting.back().second.swap(block);
            for (bool more = true; more;) { more = false;
                for (size_t w = 0; w < waiting.size(); ++w) if (waiting[w].first == next_to_write) {
                    const std::string& blk = waiting[w].second;
                    if (fr_out && !blk.empty() && fwrite(blk.data(), 1, blk.size(), fr_out) != blk.size()) { lk.unlock(); fail("write error on " + fn_reads); return; }
                    waiting.erase(waiting.begin() + static_cast<std::ptrdiff_t>(w)); ++next_to_write; more = true; break;
                } }
            lk.unlock(); cv_out.notify_all();
        }
    };
    { std::vector<std::thread> th; for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(worker); for (size_t t = 0; t < th.size(); ++t) th[t].join(); }
    { std::lock_guard<std::mutex> lk(mq); } cv_put.notify_all();
    dispatcher.join();
    bool failed = false;
    if (!first_err.empty()) { fprintf(stderr, "rtk_qv: %s\n", first_err.c_str()); failed = true; }
    else if (!waiting.empty()) { fprintf(stderr, "rtk_qv: output incomplete\n"); failed = true; }
    uint64_t dev_windows = 0, dev_found = 0;
    if (job && g_end(job, &dev_windows, &dev_found) != 0) { fprintf(stderr, "rtk_qv: --gpu: %s\n", lib.last_error()); failed = true; }
    if (fr_out && fclose(fr_out) != 0) { fprintf(stderr, "rtk_qv: write error on %s\n", fn_reads.c_str()); failed = true; }
    if (!failed && gpu) { // the device's own totals against the sums of the pieces
        unsigned long long w = 0, fd = 0; for (size_t f = 0; f < totals.size(); ++f) { w += totals[f].windows; fd += totals[f].found; }
        if (w != dev_windows || fd != dev_found) { fprintf(stderr, "rtk_qv: --gpu: the pieces add up to %llu windows / %llu found, the device counted %llu / %llu\n", w, fd, static_cast<unsigned long long>(dev_windows), static_cast<unsigned long long>(dev_found)); failed = true; }
    }
    if (failed) { unlink(fn_out.c_str()); unlink(fn_reads.c_str()); return 1; } // a failing run leaves no output file
    lap("filter");
    std::string table = "file\treads\tbases\twindows\tfound\tmissing\terror_rate\tqv\n", er, qv;
    for (size_t f = 0; f < in_long.size(); ++f) {
        const Totals& T = totals[f]; row_figures(T.windows, T.found, k, er, qv);
        table += in_long[f]; table += '\t'; table += std::to_string(T.reads); table += '\t'; table += std::to_string(T.bases); table += '\t'; table += std::to_string(T.windows); table += '\t';
        table += std::to_string(T.found); table += '\t'; table += std::to_string(T.windows - T.found); table += '\t'; table += er; table += '\t'; table += qv; table += '\n';
    }
    FILE* fo = fopen(fn_out.c_str(), "wb");
    if (!fo || fwrite(table.data(), 1, table.size(), fo) != table.size() || fclose(fo) != 0) { fprintf(stderr, "rtk_qv: cannot write %s\n", fn_out.c_str()); unlink(fn_out.c_str()); unlink(fn_reads.c_str()); return 1; }
    fputs(table.c_str(), stderr);
    return 0;
}
