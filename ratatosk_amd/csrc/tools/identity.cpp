// rtk_identity: the identity of reads to their simulated truth ([A19]; no counterpart in the reference: the project's own tool, like rtk_qv).
// -t is what rtk_simulate --lr-truth writes: per read the record of -r it was drawn from, the 0-based start, the length and the strand. The truth of a read is
// that stretch of the upper-cased reference, reverse-complemented on '-' (A<->T, C<->G, any other byte as it is); its figure is the unit-cost global (NW) edit
// distance of read and truth, exact, bytes equal iff identical after upper-casing. One row per -l file in OUT.identity.tsv: error_rate = distance / truth_bases,
// identity = 1 - error_rate, further = the aligned reads that are further from their truth than the read of that name in the nearest earlier -l file that has
// one (several of a name in that file: the closest); with --per-read one row per aligned read in OUT.identity.reads.tsv.
//   plain    the distances on the host threads (common/edit_distance.hpp; no GPU, no library)
//   --gpu    through rtk_identity_begin / _chunk / _end of libratatosk_hip.so next to this executable: the reference lives on the device, the stretches are cut there
// Both write the same bytes: the rows are printed by one function from the same integers.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../common/edit_distance.hpp"
#include "../common/fastx.hpp"
#include "../common/hip_lib.hpp"

using namespace rtk;

static const size_t kMaxLen = 262144; // the longest read or truth stretch the tool takes: it sizes the device's per-wave work areas (rtk_identity_begin)

struct Truth { uint32_t rec; uint64_t start; uint32_t len; bool rev; };
// aligned reads of one -l file, in input order, in the chunk layout of rtk_identity_chunk
struct Task { size_t id = 0, file = 0; std::string chars, names; std::vector<uint64_t> starts, name_off, t_start; std::vector<uint32_t> lens, truth, rec, t_len; std::vector<unsigned char> rev; size_t n() const { return lens.size(); } };
struct Totals { unsigned long long reads = 0, aligned = 0, not_in_truth = 0, read_bases = 0, truth_bases = 0, distance = 0; };

static inline char upper(char c) { return (c >= 'a' && c <= 'z') ? static_cast<char>(c - 32) : c; }
static inline char complement(char c) { return c == 'A' ? 'T' : (c == 'T' ? 'A' : (c == 'C' ? 'G' : (c == 'G' ? 'C' : c))); }

// one row of the table, as text (both routes, from the same integers); further < 0: the first file
static std::string table_row(const std::string& file, const Totals& T, long long further) {
    char er[64], id[64];
    if (T.truth_bases == 0) { snprintf(er, sizeof(er), "nan"); snprintf(id, sizeof(id), "nan"); }
    else { const double e = static_cast<double>(T.distance) / static_cast<double>(T.truth_bases); snprintf(er, sizeof(er), "%.6g", e); snprintf(id, sizeof(id), "%.6f", 1.0 - e); }
    return file + '\t' + std::to_string(T.reads) + '\t' + std::to_string(T.aligned) + '\t' + std::to_string(T.not_in_truth) + '\t' + std::to_string(T.read_bases) + '\t' + std::to_string(T.truth_bases) + '\t' +
           std::to_string(T.distance) + '\t' + er + '\t' + id + '\t' + (further < 0 ? std::string("-") : std::to_string(further)) + '\n';
}

static int usage() {
    fprintf(stderr, "usage: rtk_identity -r REF.fa[.gz] -t TRUTH.tsv -l reads.fq [-l ...] -o OUT [--gpu] [--per-read] [-v]\n"
                    "  -t: the file rtk_simulate --lr-truth writes (read name, record number of -r, 0-based start, length, strand + / -)\n"
                    "  writes OUT.identity.tsv: per -l file the reads found in -t (aligned), their unit-cost global edit distance to their truth stretches (distance),\n"
                    "  error_rate = distance / truth_bases, identity = 1 - error_rate, and further = the reads that are further from the truth than in the nearest earlier -l file;\n"
                    "  --per-read: OUT.identity.reads.tsv as well, one row per aligned read\n");
    return 2;
}

int main(int argc, char** argv) {
    std::vector<std::string> in_long; std::string fn_ref, fn_truth, prefix; bool gpu = false, verbose = false, per_read = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* n) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "rtk_identity: missing value for %s\n", n); exit(2); } return argv[++i]; };
        if (a == "-l") { const char* fn = need("-l"); std::vector<std::string> l = expand_input_list(fn); if (l.empty()) l.push_back(fn); in_long.insert(in_long.end(), l.begin(), l.end()); } // (a text file lists one path per line; an empty file is a file without reads)
        else if (a == "-r") fn_ref = need("-r");
        else if (a == "-t") fn_truth = need("-t");
        else if (a == "-o") prefix = need("-o");
        else if (a == "--gpu") gpu = true;
        else if (a == "--per-read") per_read = true;
        else if (a == "-v") verbose = true;
        else { fprintf(stderr, "rtk_identity: unknown option %s\n", a.c_str()); return usage(); }
    }
    if (fn_ref.empty()) { fprintf(stderr, "rtk_identity: no reference: give -r\n"); return usage(); }
    if (fn_truth.empty()) { fprintf(stderr, "rtk_identity: no truth: give -t\n"); return usage(); }
    if (in_long.empty()) { fprintf(stderr, "rtk_identity: no reads: give -l\n"); return usage(); }
    if (prefix.empty()) { fprintf(stderr, "rtk_identity: no output prefix: give -o\n"); return usage(); }
    { std::vector<std::string> v = in_long; v.push_back(fn_ref); v.push_back(fn_truth); // (before anything is read)
      for (size_t f = 0; f < v.size(); ++f) if (access(v[f].c_str(), R_OK) != 0) { fprintf(stderr, "rtk_identity: cannot open %s\n", v[f].c_str()); return 1; } }
    const std::string fn_out = prefix + ".identity.tsv", fn_reads = prefix + ".identity.reads.tsv";
    const bool trace = getenv("RTK_INDEX_TRACE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (trace || verbose) fprintf(stderr, "rtk_identity: [%8.2f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), what); };
    unsigned n_thr = std::thread::hardware_concurrency(); if (n_thr == 0) n_thr = 1; if (n_thr > 32u) n_thr = 32u;
    { const char* e = getenv("RTK_INDEX_THREADS"); if (e && atoi(e) > 0) n_thr = static_cast<unsigned>(atoi(e)); }
    // characters of -l text per chunk (RTK_INDEX_CHUNK: tests force several small chunks; a chunk holds whole reads, one at the least). The host threads share the
    // work chunk by chunk, so the plain route's chunks are small; a chunk of the device is a launch, whose waves take its pairs heaviest first
    size_t chunk_chars = gpu ? (48u << 20) : (2u << 20);
    { const char* e = getenv("RTK_INDEX_CHUNK"); if (e && strtoull(e, nullptr, 10) >= 1024) chunk_chars = std::min<size_t>(strtoull(e, nullptr, 10), 60u << 20); }
    const size_t chunk_reads = 2u << 20;

    HipLib lib; HipLib::identity_begin_fn g_begin = nullptr; HipLib::identity_chunk_fn g_chunk = nullptr; HipLib::identity_end_fn g_end = nullptr;
    if (gpu) {
        if (!lib.open("rtk_identity")) return 1;
        if (!lib.get(g_begin, "rtk_identity_begin") || !lib.get(g_chunk, "rtk_identity_chunk") || !lib.get(g_end, "rtk_identity_end") || !lib.last_error) { fprintf(stderr, "rtk_identity: --gpu: %s lacks the identity entry points\n", lib.path.c_str()); return 1; }
    }

    // ---- the reference: records in file order, upper-cased, back to back
    std::string ref; std::vector<uint64_t> rec_off(1, 0);
    {
        FastxReader fr; std::string name, seq, qual;
        if (!fr.open(fn_ref, static_cast<int>(std::min(n_thr, 16u)))) { fprintf(stderr, "rtk_identity: cannot open %s\n", fn_ref.c_str()); return 1; }
        while (fr.next(name, seq, qual)) { for (size_t i = 0; i < seq.size(); ++i) seq[i] = upper(seq[i]); ref += seq; rec_off.push_back(ref.size()); }
        if (fr.failed()) { fprintf(stderr, "rtk_identity: %s ends in a damaged or cut-short gzip stream\n", fn_ref.c_str()); return 1; }
    }
    const size_t n_rec = rec_off.size() - 1;
    lap("reference");

    // ---- the truth: five tab-separated columns per line
    std::vector<Truth> truth; std::unordered_map<std::string, uint32_t> by_name;
    {
        FILE* f = fopen(fn_truth.c_str(), "rb");
        if (!f) { fprintf(stderr, "rtk_identity: cannot open %s\n", fn_truth.c_str()); return 1; }
        std::string line; char buf[1 << 16]; unsigned long long ln = 0; bool eof = false;
        auto bad = [&](const std::string& why) { fprintf(stderr, "rtk_identity: %s line %llu: %s\n", fn_truth.c_str(), ln, why.c_str()); fclose(f); return 1; };
        auto number = [](const std::string& s, unsigned long long& v) { if (s.empty() || s.size() > 18) return false; v = 0; for (size_t i = 0; i < s.size(); ++i) { if (s[i] < '0' || s[i] > '9') return false; v = 10 * v + static_cast<unsigned long long>(s[i] - '0'); } return true; };
        while (!eof) {
            line.clear();
            for (;;) { if (!fgets(buf, sizeof(buf), f)) { eof = true; break; } line += buf; if (!line.empty() && line[line.size() - 1] == '\n') break; }
            if (eof && line.empty()) break;
            ++ln;
            while (!line.empty() && (line[line.size() - 1] == '\n' || line[line.size() - 1] == '\r')) line.erase(line.size() - 1);
            if (line.empty()) continue;
            std::vector<std::string> col; { size_t a = 0; for (;;) { const size_t b = line.find('\t', a); col.push_back(line.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; } }
            unsigned long long rec = 0, start = 0, len = 0;
            if (col.size() != 5 || col[0].empty() || !number(col[1], rec) || !number(col[2], start) || !number(col[3], len) || (col[4] != "+" && col[4] != "-"))
                return bad("malformed: expected name, record number, 0-based start, length and strand (+ or -), tab-separated");
            if (rec >= n_rec) return bad("record " + col[1] + " is not in " + fn_ref + " (" + std::to_string(n_rec) + " records)");
            const uint64_t rl = rec_off[rec + 1] - rec_off[rec];
            if (start > rl || len > rl - start) return bad("the stretch " + col[2] + " + " + col[3] + " lies outside record " + col[1] + " (" + std::to_string(rl) + " characters)");
            if (len > kMaxLen) return bad("the stretch of " + col[3] + " characters is longer than the limit of " + std::to_string(kMaxLen));
            if (!by_name.emplace(col[0], static_cast<uint32_t>(truth.size())).second) return bad("the name " + col[0] + " is listed twice");
            Truth t; t.rec = static_cast<uint32_t>(rec); t.start = start; t.len = static_cast<uint32_t>(len); t.rev = col[4] == "-"; truth.push_back(t);
        }
        fclose(f);
    }
    lap("truth");
    if (trace || verbose) fprintf(stderr, "rtk_identity: %zu reference characters in %zu records, %zu reads in the truth\n", ref.size(), n_rec, truth.size());

    void* job = nullptr;
    if (gpu) {
        if (g_begin(0, ref.data(), ref.size(), rec_off.data(), static_cast<uint32_t>(n_rec), static_cast<uint32_t>(kMaxLen), &job) != 0) { fprintf(stderr, "rtk_identity: --gpu: %s\n", lib.last_error()); return 1; }
        std::string().swap(ref); // (the reference lives on the device)
        lap("reference on the device");
    }

    // ---- the reads: one dispatcher thread reads the -l files in order and lays chunks out, the threads align them (--gpu: on the device, two calls side by side; else
    // on the host), and the per-read rows are written in input order
    FILE* fr_out = nullptr;
    if (per_read) { fr_out = fopen(fn_reads.c_str(), "wb"); if (!fr_out) { fprintf(stderr, "rtk_identity: cannot write %s\n", fn_reads.c_str()); if (job) g_end(job, nullptr, nullptr); return 1; } fputs("file_index\tname\tlength\ttruth_length\tdistance\n", fr_out); }
    else unlink(fn_reads.c_str()); // (a file of an earlier run is not this run's result)
    std::mutex mq, m_out, m_err; std::condition_variable cv_put, cv_get, cv_out; std::deque<std::unique_ptr<Task> > q; bool done = false; std::atomic<bool> stop(false);
    std::string first_err; auto fail = [&](const std::string& msg) { { std::lock_guard<std::mutex> lk(m_err); if (first_err.empty()) first_err = msg; } stop = true; { std::lock_guard<std::mutex> lk(mq); } cv_put.notify_all(); cv_get.notify_all(); { std::lock_guard<std::mutex> lk(m_out); } cv_out.notify_all(); };
    std::vector<Totals> totals(in_long.size());
    std::vector<std::vector<std::pair<uint32_t, int32_t> > > seen(in_long.size()); // per file: (entry of the truth, distance) of every aligned read
    size_t next_to_write = 0; std::vector<std::pair<size_t, std::string> > waiting; // formatted blocks that wait for the ones before them
    const size_t ahead = 2 * static_cast<size_t>(n_thr) + 4;
    std::thread dispatcher([&]() {
        size_t id = 0;
        auto put = [&](std::unique_ptr<Task>& t) { t->id = id++; std::unique_lock<std::mutex> lk(mq); cv_put.wait(lk, [&]() { return q.size() < ahead || stop.load(); }); if (stop) return; q.push_back(std::move(t)); cv_get.notify_one(); };
        for (size_t f = 0; f < in_long.size() && !stop; ++f) {
            FastxReader fr; std::string name, seq, qual;
            if (!fr.open(in_long[f], static_cast<int>(std::min(n_thr, 16u)))) { fail("cannot open " + in_long[f]); break; }
            std::unique_ptr<Task> t; unsigned long long reads = 0, missing = 0;
            auto fresh = [&]() { t.reset(new Task()); t->file = f; };
            fresh();
            while (!stop && fr.next(name, seq, qual)) {
                ++reads;
                const auto it = by_name.find(name);
                if (it == by_name.end()) { ++missing; continue; }
                if (seq.size() > kMaxLen) { fail("read " + name + " of " + in_long[f] + " has " + std::to_string(seq.size()) + " characters, more than the limit of " + std::to_string(kMaxLen)); break; }
                if (t->n() && (t->chars.size() + seq.size() + 1 > chunk_chars || t->n() >= chunk_reads)) { put(t); fresh(); }
                const Truth& T = truth[it->second];
                for (size_t i = 0; i < seq.size(); ++i) seq[i] = upper(seq[i]);
                t->starts.push_back(t->chars.size()); t->chars += seq; t->chars.push_back('\n');
                t->name_off.push_back(t->names.size()); t->names += name; t->lens.push_back(static_cast<uint32_t>(seq.size()));
                t->truth.push_back(it->second); t->rec.push_back(T.rec); t->t_start.push_back(T.start); t->t_len.push_back(T.len); t->rev.push_back(T.rev ? 1 : 0);
            }
            if (!stop && fr.failed()) fail(in_long[f] + " ends in a damaged or cut-short gzip stream");
            if (!stop && t->n()) put(t);
            { std::lock_guard<std::mutex> lk(m_out); totals[f].reads += reads; totals[f].not_in_truth += missing; }
        }
        { std::lock_guard<std::mutex> lk(mq); done = true; } cv_get.notify_all();
    });
    auto worker = [&]() {
        std::string block, stretch; std::vector<int32_t> dist; EditDistance ed;
        for (;;) {
            std::unique_ptr<Task> t;
            { std::unique_lock<std::mutex> lk(mq); cv_get.wait(lk, [&]() { return !q.empty() || done || stop.load(); }); if (stop || q.empty()) return; t = std::move(q.front()); q.pop_front(); }
            cv_put.notify_one();
            { std::unique_lock<std::mutex> lk(m_out); cv_out.wait(lk, [&]() { return t->id < next_to_write + ahead || stop.load(); }); if (stop) return; } // bounded run-ahead of the writer
            const size_t n = t->n(); dist.assign(n, 0);
            if (gpu) { if (g_chunk(job, t->chars.data(), t->chars.size(), t->starts.data(), static_cast<uint32_t>(n), t->rec.data(), t->t_start.data(), t->t_len.data(), t->rev.data(), dist.data()) != 0) { fail(std::string("--gpu: ") + lib.last_error()); return; } }
            else for (size_t r = 0; r < n; ++r) {
                const char* src = ref.data() + rec_off[t->rec[r]] + t->t_start[r]; const size_t tl = t->t_len[r];
                if (t->rev[r]) { stretch.resize(tl); for (size_t i = 0; i < tl; ++i) stretch[i] = complement(src[tl - 1 - i]); src = stretch.data(); }
                dist[r] = static_cast<int32_t>(ed(t->chars.data() + t->starts[r], t->lens[r], src, tl));
            }
            Totals add; add.aligned = n; block.clear(); t->name_off.push_back(t->names.size());
            for (size_t r = 0; r < n; ++r) {
                add.read_bases += t->lens[r]; add.truth_bases += t->t_len[r]; add.distance += static_cast<unsigned long long>(dist[r]);
                if (per_read) { block += std::to_string(t->file); block += '\t'; block.append(t->names, t->name_off[r], t->name_off[r + 1] - t->name_off[r]); block += '\t'; block += std::to_string(t->lens[r]); block += '\t';
                    block += std::to_string(t->t_len[r]); block += '\t'; block += std::to_string(dist[r]); block += '\n'; }
            }
            std::unique_lock<std::mutex> lk(m_out); // blocks leave in task order: whoever holds the next one writes it and those that waited for it
            Totals& T = totals[t->file]; T.aligned += add.aligned; T.read_bases += add.read_bases; T.truth_bases += add.truth_bases; T.distance += add.distance;
            for (size_t r = 0; r < n; ++r) seen[t->file].emplace_back(t->truth[r], dist[r]);
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
    if (!first_err.empty()) { fprintf(stderr, "rtk_identity: %s\n", first_err.c_str()); failed = true; }
    else if (!waiting.empty()) { fprintf(stderr, "rtk_identity: output incomplete\n"); failed = true; }
    uint64_t dev_pairs = 0, dev_sum = 0;
    if (job && g_end(job, &dev_pairs, &dev_sum) != 0) { fprintf(stderr, "rtk_identity: --gpu: %s\n", lib.last_error()); failed = true; }
    if (fr_out && fclose(fr_out) != 0) { fprintf(stderr, "rtk_identity: write error on %s\n", fn_reads.c_str()); failed = true; }
    if (!failed && gpu) { // the device's own totals against the sums of the chunks
        unsigned long long p = 0, s = 0; for (size_t f = 0; f < totals.size(); ++f) { p += totals[f].aligned; s += totals[f].distance; }
        if (p != dev_pairs || s != dev_sum) { fprintf(stderr, "rtk_identity: --gpu: the chunks add up to %llu pairs / distance %llu, the device counted %llu / %llu\n", p, s, static_cast<unsigned long long>(dev_pairs), static_cast<unsigned long long>(dev_sum)); failed = true; }
    }
    if (failed) { unlink(fn_out.c_str()); unlink(fn_reads.c_str()); return 1; } // a failing run leaves no output file
    lap("distances");
    // further: against the nearest earlier file that aligned a read of that name (the closest read of the name there)
    std::string table = "file\treads\taligned\tnot_in_truth\tread_bases\ttruth_bases\tdistance\terror_rate\tidentity\tfurther\n";
    std::vector<int32_t> nearest(truth.size(), -1); // distance of the name in the nearest earlier file, -1: none yet
    for (size_t f = 0; f < in_long.size(); ++f) {
        long long further = f == 0 ? -1 : 0;
        for (size_t i = 0; f > 0 && i < seen[f].size(); ++i) { const int32_t was = nearest[seen[f][i].first]; if (was >= 0 && seen[f][i].second > was) ++further; }
        for (size_t i = 0; i < seen[f].size(); ++i) nearest[seen[f][i].first] = -1; // this file replaces what earlier ones said about its names ...
        for (size_t i = 0; i < seen[f].size(); ++i) { int32_t& d = nearest[seen[f][i].first]; if (d < 0 || seen[f][i].second < d) d = seen[f][i].second; } // ... with its closest read of each
        table += table_row(in_long[f], totals[f], further);
    }
    FILE* fo = fopen(fn_out.c_str(), "wb");
    if (!fo || fwrite(table.data(), 1, table.size(), fo) != table.size() || fclose(fo) != 0) { fprintf(stderr, "rtk_identity: cannot write %s\n", fn_out.c_str()); unlink(fn_out.c_str()); unlink(fn_reads.c_str()); return 1; }
    fputs(table.c_str(), stderr);
    return 0;
}
