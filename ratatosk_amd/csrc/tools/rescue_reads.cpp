// rtk_rescue_reads: the rescue of unmapped short reads before the index build (`Ratatosk correct -u`; reference: retrieveMissingReads,
// src/Graph.cpp:3857-4131, called at src/Ratatosk.cpp:1040-1056). Scans the reads of the -u files and keeps those with at least 31 start positions
// (min_nb_km_unmapped = small_k, src/Common.hpp:156: 31 whatever -k says) whose k-mer is seen at least twice in the long reads (-l) and not at least
// twice in the mapped short reads (-s); the kept reads go to OUT_extra_sr.fasta (">NAME\nSEQ\n", upper-cased, input order), which joins the short reads
// of the index builds. Exact sets where the reference has Bloom filters: DESIGN.md section 4, [A11].
//   plain    k-mers counted and reads tested on the host threads (no GPU, no library): bisection in the two sorted sets
//   --gpu    both counts from rtk_index_count_kmers, the filter through rtk_rescue_begin / _chunk / _end of libratatosk_hip.so next to this executable
// Both write the same bytes. No read kept, or no long-read k-mer seen twice: exit status 0 and no file (src/Graph.cpp:4124-4128).
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
#include <vector>

#include "../common/fastx.hpp"
#include "../common/hip_lib.hpp"
#include "../common/kmer.hpp"
#include "../common/kmer_count.hpp"

using namespace rtk;

static const uint32_t MIN_POSITIONS = 31; // min_nb_km_unmapped (src/Common.hpp:156)

// a batch of -u reads in the chunk layout of rtk_rescue_chunk: sequences separated by '\n'
struct Batch { std::string chars, names; std::vector<uint64_t> starts, name_off; std::vector<unsigned char> keep; size_t n() const { return starts.size(); } };

static bool in_sorted(const std::vector<uint64_t>& a, uint64_t x) { return std::binary_search(a.begin(), a.end(), x); }

// the restated rule on the host: start positions whose k characters are all A/C/G/T and spell a k-mer of lr that is not in sr
static uint32_t qualifying_positions(const char* s, size_t len, int k, const std::vector<uint64_t>& lr, const std::vector<uint64_t>& sr) {
    uint32_t n = 0;
    for_each_canonical_kmer<uint64_t>(s, len, k, kmer_mask(k), [&](uint64_t c, size_t) { if (in_sorted(lr, c) && !in_sorted(sr, c)) ++n; });
    return n;
}

int main(int argc, char** argv) {
    std::vector<std::string> in_short, in_long, in_unmapped;
    std::string prefix; int k = 31; bool gpu = false, verbose = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* n) -> const char* { if (i + 1 >= argc) { fprintf(stderr, "rtk_rescue_reads: missing value for %s\n", n); exit(2); } return argv[++i]; };
        auto add = [&](std::vector<std::string>& v, const char* fn) { const std::vector<std::string> l = expand_input_list(fn); v.insert(v.end(), l.begin(), l.end()); }; // (a text file lists one path per line)
        if (a == "-s") add(in_short, need("-s"));
        else if (a == "-l") add(in_long, need("-l"));
        else if (a == "-u") add(in_unmapped, need("-u"));
        else if (a == "-o") prefix = need("-o");
        else if (a == "-k") k = atoi(need("-k"));
        else if (a == "--gpu") gpu = true;
        else if (a == "-v") verbose = true;
        else { fprintf(stderr, "rtk_rescue_reads: unknown option %s\n", a.c_str()); return 2; }
    }
    if (in_short.empty() || in_long.empty() || in_unmapped.empty() || prefix.empty() || k < 3 || k > 31 || !(k & 1)) {
        fprintf(stderr, "usage: rtk_rescue_reads -s mapped_short_reads.fq [-s ...] -l long_reads.fq [-l ...] -u unmapped_short_reads.fq [-u ...] -o PREFIX [-k 31 (odd, <= 31)] [--gpu] [-v]\n"
                        "  writes PREFIX_extra_sr.fasta: the -u reads with at least 31 positions whose k-mer occurs twice in the long reads and not twice in the -s reads\n");
        return 2;
    }
    for (int g = 0; g < 3; ++g) { const std::vector<std::string>& v = g == 0 ? in_short : (g == 1 ? in_long : in_unmapped); // (before any counting: a missing file is an argument error)
        for (size_t f = 0; f < v.size(); ++f) if (!SampleSource::is_spec(v[f]) && access(v[f].c_str(), R_OK) != 0) { fprintf(stderr, "rtk_rescue_reads: cannot open %s\n", v[f].c_str()); return 1; } }
    const std::string fn_out = prefix + "_extra_sr.fasta";
    const bool trace = getenv("RTK_INDEX_TRACE") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (trace) fprintf(stderr, "rtk_rescue_reads: [%8.2f s] %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(), what); };
    unsigned n_thr = std::thread::hardware_concurrency(); if (n_thr == 0) n_thr = 1; if (n_thr > 32u) n_thr = 32u;
    { const char* e = getenv("RTK_INDEX_THREADS"); if (e && atoi(e) > 0) n_thr = static_cast<unsigned>(atoi(e)); }
    size_t chunk_chars = 48u << 20; // characters of -u text per batch (RTK_INDEX_CHUNK: tests force several small batches)
    { const char* e = getenv("RTK_INDEX_CHUNK"); if (e && strtoull(e, nullptr, 10) >= 1024) chunk_chars = std::min<size_t>(strtoull(e, nullptr, 10), 60u << 20); }
    const size_t chunk_reads = 2u << 20;

    HipLib lib; HipLib::rescue_begin_fn g_begin = nullptr; HipLib::rescue_chunk_fn g_chunk = nullptr; HipLib::rescue_end_fn g_end = nullptr;
    if (gpu) {
        if (!lib.open("rtk_rescue_reads")) return 1;
        if (!lib.count_kmers || !lib.get(g_begin, "rtk_rescue_begin") || !lib.get(g_chunk, "rtk_rescue_chunk") || !lib.get(g_end, "rtk_rescue_end") || !lib.last_error || !lib.free) { fprintf(stderr, "rtk_rescue_reads: --gpu: %s lacks the rescue entry points\n", lib.path.c_str()); return 1; }
    }

    // ---- the two k-mer sets: seen at least twice in the -s reads (bf_non_uniq, src/Graph.cpp:3733, 3830), in the long reads (the Bifrost build with its singleton filter, :3884)
    std::vector<uint64_t> sr, lr;
    auto count = [&](const std::vector<std::string>& files, std::vector<uint64_t>& out) -> bool {
        if (!gpu) {
            size_t f = 0; const int bad = count_kmers_host<uint64_t>(files, k, 2, n_thr, out, &f);
            if (bad) fprintf(stderr, bad == 2 ? "rtk_rescue_reads: %s ends in a damaged or cut-short gzip stream\n" : "rtk_rescue_reads: cannot open %s\n", files[f].c_str());
            return !bad;
        }
        std::vector<const char*> fp; for (size_t f = 0; f < files.size(); ++f) fp.push_back(files[f].c_str());
        uint64_t* sk = nullptr; uint64_t ns = 0;
        if (lib.count_kmers(0, k, fp.data(), static_cast<int>(fp.size()), 2, static_cast<int>(n_thr), &sk, &ns) != 0) { fprintf(stderr, "rtk_rescue_reads: --gpu: %s\n", lib.last_error()); return false; }
        out.assign(sk, sk + ns); lib.free(sk); return true;
    };
    if (verbose) fprintf(stderr, "Ratatosk::retrieveMissingReads(): Creating index of short reads\n");
    if (!count(in_short, sr)) return 1;
    lap("count SR");
    if (verbose) fprintf(stderr, "Ratatosk::retrieveMissingReads(): Creating index of long reads\n");
    if (!count(in_long, lr)) return 1;
    lap("count LR");
    if (trace) fprintf(stderr, "rtk_rescue_reads: %zu %d-mers seen twice in the long reads, %zu in the short reads\n", lr.size(), k, sr.size());
    unlink(fn_out.c_str()); // (a file of an earlier run is not this run's result)
    if (lr.empty()) { // nb_km_lr == 0 (src/Graph.cpp:3890): nothing can qualify
        if (verbose) fprintf(stderr, "Ratatosk::retrieveMissingReads(): Added 0 short reads to dataset.\n");
        fprintf(stderr, "rtk_rescue_reads: 0 reads kept (no long-read %d-mer is seen twice)\n", k);
        return 0;
    }
    void* job = nullptr;
    if (gpu) {
        if (g_begin(0, k, lr.data(), lr.size(), sr.data(), sr.size(), MIN_POSITIONS, &job) != 0) { fprintf(stderr, "rtk_rescue_reads: --gpu: %s\n", lib.last_error()); return 1; }
        std::vector<uint64_t>().swap(lr); std::vector<uint64_t>().swap(sr); // (the table lives on the device)
    }
    lap("build D");

    // ---- the scan. A file that can be reached at any offset (plain, blocked gzip) is cut into byte ranges that the threads parse independently (rtk::PlainChunks);
    // everything else (ordinary gzip, sampled sources, FASTQ on more than four lines) is read by the one dispatcher thread. Either way a batch has a number, the
    // threads test their batches (--gpu: on the device, two calls side by side; else on the host) and format the kept reads, and blocks are written in batch order.
    if (verbose) fprintf(stderr, "Ratatosk::retrieveMissingReads(): Querying full short read set for missing reads\n");
    FILE* fo = fopen(fn_out.c_str(), "wb");
    if (!fo) { fprintf(stderr, "rtk_rescue_reads: cannot write %s\n", fn_out.c_str()); if (job) g_end(job, nullptr, nullptr); return 1; }
    struct Task { size_t id = 0; const PlainChunks* pc = nullptr; size_t chunk = 0; std::unique_ptr<Batch> ready; };
    std::mutex mq, m_out, m_err; std::condition_variable cv_put, cv_get, cv_out; std::deque<Task> q; bool done = false; std::atomic<bool> stop(false);
    std::string first_err; auto fail = [&](const std::string& msg) { { std::lock_guard<std::mutex> lk(m_err); if (first_err.empty()) first_err = msg; } stop = true; { std::lock_guard<std::mutex> lk(mq); } cv_put.notify_all(); cv_get.notify_all(); { std::lock_guard<std::mutex> lk(m_out); } cv_out.notify_all(); };
    std::vector<std::unique_ptr<PlainChunks> > pcs; // (alive until the threads are done)
    size_t next_to_write = 0; std::vector<std::pair<size_t, std::string> > waiting; // formatted blocks that wait for the ones before them
    std::atomic<unsigned long long> n_in(0), n_kept(0);
    const size_t ahead = 2 * static_cast<size_t>(n_thr) + 4;
    const bool serial = getenv("RTK_SERIAL_READER") != nullptr;
    std::thread dispatcher([&]() {
        size_t id = 0;
        auto put = [&](Task&& t) { std::unique_lock<std::mutex> lk(mq); cv_put.wait(lk, [&]() { return q.size() < ahead || stop.load(); }); if (stop) return; q.push_back(std::move(t)); cv_get.notify_one(); };
        for (size_t f = 0; f < in_unmapped.size() && !stop; ++f) {
            if (!serial && PlainChunks::is_plain(in_unmapped[f])) {
                pcs.emplace_back(new PlainChunks());
                if (!pcs.back()->open(in_unmapped[f], chunk_chars)) { fail("cannot open " + in_unmapped[f]); break; } // (a range of that many BYTES of FASTA/FASTQ text holds fewer characters of sequence)
                for (size_t c = 0; c < pcs.back()->n_chunks() && !stop; ++c) { Task t; t.id = id++; t.pc = pcs.back().get(); t.chunk = c; put(std::move(t)); }
                continue;
            }
            FastxReader fr; std::string name, seq, qual; std::unique_ptr<Batch> b(new Batch());
            if (!fr.open(in_unmapped[f], static_cast<int>(std::min(n_thr, 16u)))) { fail("cannot open " + in_unmapped[f]); break; }
            auto push = [&]() { Task t; t.id = id++; t.ready = std::move(b); put(std::move(t)); b.reset(new Batch()); };
            while (!stop && fr.next(name, seq, qual)) {
                if (seq.size() + 1 > chunk_chars) { fail("a read of " + in_unmapped[f] + " is longer than a batch (" + std::to_string(chunk_chars) + " characters)"); break; }
                if (b->chars.size() + seq.size() + 1 > chunk_chars || b->n() >= chunk_reads) push();
                b->starts.push_back(b->chars.size()); b->chars += seq; b->chars.push_back('\n');
                b->name_off.push_back(b->names.size()); b->names += name;
            }
            if (!stop && fr.failed()) fail(in_unmapped[f] + " ends in a damaged or cut-short gzip stream");
            if (!stop && b->n()) push();
        }
        { std::lock_guard<std::mutex> lk(mq); done = true; } cv_get.notify_all();
    });
    auto worker = [&]() {
        std::string block;
        for (;;) {
            Task t;
            { std::unique_lock<std::mutex> lk(mq); cv_get.wait(lk, [&]() { return !q.empty() || done || stop.load(); }); if (stop || q.empty()) return; t = std::move(q.front()); q.pop_front(); }
            cv_put.notify_one();
            { std::unique_lock<std::mutex> lk(m_out); cv_out.wait(lk, [&]() { return t.id < next_to_write + ahead || stop.load(); }); if (stop) return; } // bounded run-ahead of the writer
            std::unique_ptr<Batch> b = std::move(t.ready);
            if (!b) { // a byte range of a plain file
                PackedReads pr(false);
                if (!t.pc->parse_chunk(t.chunk, pr)) { fail(pr.malformed() ? "a -u file starts as 4-line FASTQ but holds a record laid out differently; RTK_SERIAL_READER=1 reads such a file on one thread" : "read error on a -u file"); return; }
                b.reset(new Batch()); b->chars.reserve(pr.n_bases() + pr.size());
                for (size_t r = 0; r < pr.size(); ++r) { b->starts.push_back(b->chars.size()); b->chars.append(pr.seq(r), pr.seq_len(r)); b->chars.push_back('\n'); b->name_off.push_back(b->names.size()); b->names.append(pr.name(r), pr.name_len(r)); }
                if (b->chars.size() > (60u << 20) || b->n() > (4u << 20) - 1) { fail("a byte range of a -u file holds more than a batch (a read of tens of megabases?)"); return; }
            }
            const size_t n = b->n(); b->keep.assign(n ? n : 1, 0); b->name_off.push_back(b->names.size());
            if (n && gpu) { if (g_chunk(job, b->chars.data(), b->chars.size(), b->starts.data(), static_cast<uint32_t>(n), b->keep.data()) != 0) { fail(std::string("--gpu: ") + lib.last_error()); return; } }
            else for (size_t r = 0; r < n; ++r) { const size_t e = (r + 1 < n ? b->starts[r + 1] : b->chars.size()) - 1; // (without the separator)
                b->keep[r] = qualifying_positions(b->chars.data() + b->starts[r], e - b->starts[r], k, lr, sr) >= MIN_POSITIONS ? 1 : 0; }
            block.clear(); unsigned long long kept = 0;
            for (size_t r = 0; r < n; ++r) if (b->keep[r]) {
                const size_t s0 = b->starts[r], e = (r + 1 < n ? b->starts[r + 1] : b->chars.size()) - 1;
                block += '>'; block.append(b->names, b->name_off[r], b->name_off[r + 1] - b->name_off[r]); block += '\n';
                const size_t at = block.size(); block.append(b->chars, s0, e - s0);
                for (size_t i = at; i < block.size(); ++i) block[i] = static_cast<char>(toupper(static_cast<unsigned char>(block[i])));
                block += '\n'; ++kept;
            }
            n_in += n; n_kept += kept;
            std::unique_lock<std::mutex> lk(m_out); // blocks leave in batch order: whoever holds the next one writes it and those that waited for it
            waiting.emplace_back(t.id, std::string()); waiting.back().second.swap(block);
            for (bool more = true; more;) { more = false;
                for (size_t w = 0; w < waiting.size(); ++w) if (waiting[w].first == next_to_write) {
                    const std::string& blk = waiting[w].second;
                    if (!blk.empty() && fwrite(blk.data(), 1, blk.size(), fo) != blk.size()) { lk.unlock(); fail("write error on " + fn_out); return; }
                    waiting.erase(waiting.begin() + static_cast<std::ptrdiff_t>(w)); ++next_to_write; more = true; break;
                } }
            lk.unlock(); cv_out.notify_all();
        }
    };
    { std::vector<std::thread> th; for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(worker); for (size_t t = 0; t < th.size(); ++t) th[t].join(); }
    { std::lock_guard<std::mutex> lk(mq); } cv_put.notify_all();
    dispatcher.join();
    bool failed = false;
    if (!first_err.empty()) { fprintf(stderr, "rtk_rescue_reads: %s\n", first_err.c_str()); failed = true; }
    else if (!waiting.empty()) { fprintf(stderr, "rtk_rescue_reads: output incomplete\n"); failed = true; }
    uint64_t n_probed = 0, n_hits = 0;
    if (job && g_end(job, &n_probed, &n_hits) != 0) { fprintf(stderr, "rtk_rescue_reads: --gpu: %s\n", lib.last_error()); failed = true; }
    if (fclose(fo) != 0) { fprintf(stderr, "rtk_rescue_reads: write error on %s\n", fn_out.c_str()); failed = true; }
    if (failed) { unlink(fn_out.c_str()); return 1; } // a failing step leaves no output file
    lap("filter");
    if (trace && gpu) fprintf(stderr, "rtk_rescue_reads: %llu positions probed, %llu hits\n", static_cast<unsigned long long>(n_probed), static_cast<unsigned long long>(n_hits));
    const unsigned long long kept_all = n_kept.load(), in_all = n_in.load();
    if (trace) fprintf(stderr, "rtk_rescue_reads: reads in %llu / kept %llu\n", in_all, kept_all);
    if (verbose) fprintf(stderr, "Ratatosk::retrieveMissingReads(): Added %llu short reads to dataset.\n", kept_all);
    if (kept_all == 0) unlink(fn_out.c_str()); // src/Graph.cpp:4124-4128
    fprintf(stderr, "rtk_rescue_reads: %llu reads kept of %llu%s\n", kept_all, in_all, kept_all ? (" -> " + fn_out).c_str() : " (no file)");
    return 0;
}
