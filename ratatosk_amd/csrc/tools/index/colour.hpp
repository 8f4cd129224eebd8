// rtk_build_index, pass 2: colours (ids of the read pairs, or of the reads with --colour-reads) and coverage of every unitig. Three read sources
// number the reads and hand (sequence, id) to one sink, which looks the k-mers up on the host threads or feeds the device job.
#ifndef RTK_TOOLS_INDEX_COLOUR_HPP
#define RTK_TOOLS_INDEX_COLOUR_HPP

#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>

#include "../../common/name_hash.hpp"
#include "colour_filter.hpp"
#include "state.hpp"

namespace rtk {

// mates share a name up to a trailing /1 or /2: the length of the name without it
inline size_t pair_name_len(const char* p, size_t n) { return (n > 2 && p[n - 2] == '/' && (p[n - 1] == '1' || p[n - 1] == '2')) ? n - 2 : n; }

// --gpu: the reads are handed to the device chunk by chunk (csrc/hip/rtk_index_colour.h rtk_index_colour_*: the k-mer table of the unitigs in HBM, one lane per
// read position); this tool keeps what is its own -- reading, and the numbering of the reads. Every thread fills a chunk of its own.
// With a confidence threshold (q_min != 0; tools/index/colour_filter.hpp) the quality bytes travel beside the characters and the device masks (fn_q); a library without
// that entry gets characters masked here.
struct Feed {
    std::string chars, quals; std::vector<uint64_t> starts; std::vector<uint32_t> ids; void* job; HipLib::col_chunk_fn fn; std::atomic<int>* failed;
    HipLib::col_chunk_q_fn fn_q = nullptr; unsigned char q_min = 0;
    void flush() {
        if (ids.empty()) return;
        const int rc = q_min && fn_q ? fn_q(job, chars.data(), reinterpret_cast<const unsigned char*>(quals.data()), q_min, chars.size(), starts.data(), ids.data(), static_cast<uint32_t>(ids.size()))
                                     : fn(job, chars.data(), chars.size(), starts.data(), ids.data(), static_cast<uint32_t>(ids.size()));
        if (rc != 0) *failed = 1;
        chars.clear(); quals.clear(); starts.clear(); ids.clear();
    }
    void add(const char* seq, const char* qual, size_t len, uint32_t id) {
        if (len + 1 > (60u << 20)) { *failed = 1; return; } // (a read longer than a chunk)
        if (chars.size() + len + 1 > (60u << 20) || ids.size() >= (2u << 20) || (chars.size() >= (24u << 20))) flush();
        starts.push_back(chars.size()); ids.push_back(id);
        if (q_min && !fn_q) { const size_t at = chars.size(); chars.resize(at + len); colour_mask_bases(seq, qual, len, q_min, &chars[at]); }
        else chars.append(seq, len);
        chars.push_back('\n');
        if (q_min && fn_q) { quals.append(qual, len); quals.push_back('\n'); } // (the byte beside a separator is not looked at)
    }
};

template <class KM> struct ColourSink {
    IndexBuild<KM>& s; std::vector<Unitig>& U; const size_t n_u;
    void* job = nullptr; std::atomic<int> failed; HipLib::col_chunk_fn chunk_fn = nullptr; HipLib::col_end_fn end_fn = nullptr; std::vector<Feed> feeds;
    HipLib::col_cov_fn cov_fn = nullptr; HipLib::col_end_sub_fn end_sub_fn = nullptr; bool open_job = false; // --subsample-colours: the job stays open (open_job) between the coverage and the thinned events
    HipLib::col_merge_fn merge_fn = nullptr; HipLib::col_merge_classes_fn merge_classes_fn = nullptr; // --merge-duplicates (pairs only): the events merged in place in the open job
    std::vector<std::vector<uint64_t> > cov; std::vector<std::vector<std::pair<uint32_t, uint32_t> > > ev; // host: per thread, k-mers per unitig and (unitig, id) events
    // --colour-reads with --colour-min-conf / --colour-min-len (tools/index/colour_filter.hpp): q_min = 0 and min_len = 0 when not given
    const unsigned char q_min; const uint64_t min_len; HipLib::col_chunk_q_fn chunk_q_fn = nullptr;
    struct PerThread { std::string masked; uint64_t too_short = 0; char pad[64]; }; std::vector<PerThread> per_thread; // a host thread's masked copy of its read; the reads its length rule left out

    explicit ColourSink(IndexBuild<KM>& st) : s(st), U(st.U), n_u(st.U.size()), failed(0), feeds(st.n_thr), cov(st.n_thr), ev(st.n_thr),
                                              q_min(st.o.colour_min_conf >= 0.0 ? colour_q_min(st.o.colour_min_conf, st.o.colour_max_qual) : static_cast<unsigned char>(0)), min_len(st.o.colour_min_len), per_thread(st.n_thr) {
        HipLib::col_begin_fn begin_fn = nullptr;
        if (s.o.gpu && s.lib.get(begin_fn, "rtk_index_colour_begin") && s.lib.get(chunk_fn, "rtk_index_colour_chunk") && s.lib.get(end_fn, "rtk_index_colour_end") && !s.knobs.host_colours && n_u > 0) {
            if (s.o.merge && s.o.colour_files.empty() && !(s.lib.get(merge_fn, "rtk_index_colour_merge") && s.lib.get(merge_classes_fn, "rtk_index_colour_merge_classes"))) { // (the events are then fetched at once and every later step runs on the host threads)
                merge_fn = nullptr; merge_classes_fn = nullptr; fprintf(stderr, "rtk_build_index: --gpu: %s lacks rtk_index_colour_merge / rtk_index_colour_merge_classes: ids merged on the host threads\n", s.lib.path.c_str()); }
            const bool host_merge = s.o.merge && s.o.colour_files.empty() && !merge_fn;
            if (s.o.subsample && host_merge) { cov_fn = nullptr; end_sub_fn = nullptr; }
            else if (s.o.subsample && !(s.lib.get(cov_fn, "rtk_index_colour_cov") && s.lib.get(end_sub_fn, "rtk_index_colour_end_subsampled"))) { // (the events are then fetched the old way, rtk_index_colour_end)
                cov_fn = nullptr; end_sub_fn = nullptr; fprintf(stderr, "rtk_build_index: --gpu: %s lacks rtk_index_colour_cov / rtk_index_colour_end_subsampled: colours subsampled on the host threads\n", s.lib.path.c_str()); }
            if (q_min && !s.lib.get(chunk_q_fn, "rtk_index_colour_chunk_q")) { // (the look-ups stay on the device)
                chunk_q_fn = nullptr; fprintf(stderr, "rtk_build_index: --gpu: %s lacks rtk_index_colour_chunk_q: bases masked on the host threads\n", s.lib.path.c_str()); }
            std::vector<uint64_t> off(n_u + 1, 0); for (size_t u = 0; u < n_u; ++u) off[u + 1] = off[u] + s.U[u].seq.size();
            std::string pool(off[n_u], 'A');
            parallel_for(n_u, s.n_thr, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) memcpy(&pool[off[u]], s.U[u].seq.data(), s.U[u].seq.size()); });
            if (begin_fn(0, s.k, pool.data(), off.data(), n_u, &job) != 0) { fprintf(stderr, "rtk_build_index: --gpu: colours on the host threads (%s)\n", s.lib.last_error()); job = nullptr; }
            open_job = job != nullptr;
        }
        for (unsigned t = 0; t < s.n_thr; ++t) { feeds[t].job = job; feeds[t].fn = chunk_fn; feeds[t].failed = &failed; feeds[t].fn_q = chunk_q_fn; feeds[t].q_min = q_min; if (!job) cov[t].assign(n_u, 0); }
    }
    ~ColourSink() { if (open_job) end_fn(job, nullptr, nullptr, nullptr); } // (left early: the job released)
    // one read, from thread t of the source: its k-mers looked up (the table is only read), or the read handed to the device
    // (qual: len quality bytes, or null; the sources see to it that a read has them when there is a confidence threshold)
    void read(unsigned t, const char* seq, const char* qual, size_t len, uint32_t id) {
        if (len < min_len) { ++per_thread[t].too_short; return; } // (the read keeps its id: the source has numbered it)
        if (job) { feeds[t].add(seq, qual, len, id); return; }
        if (q_min) { std::string& m = per_thread[t].masked; m.resize(len); colour_mask_bases(seq, qual, len, q_min, &m[0]); seq = m.data(); }
        std::vector<uint64_t>& c = cov[t]; std::vector<std::pair<uint32_t, uint32_t> >& e = ev[t];
        for_each_canonical_kmer<KM>(seq, len, s.k, s.mask, [&](KM km, size_t) {
            const uint64_t* v = s.km.slot(km, false);
            if (v) { const uint32_t u = static_cast<uint32_t>((*v >> 32) - 1); ++c[u]; if (e.empty() || e.back().first != u || e.back().second != id) e.push_back(std::make_pair(u, id)); }
        });
    }
    // sorted events unitig << 32 | id into the colours of the unitigs
    void take_events(const uint64_t* evs, uint64_t n_ev) {
        parallel_for(n_u, s.n_thr, [&](size_t b, size_t e, unsigned) {
            if (b >= e) return;
            const uint64_t* p = std::lower_bound(evs, evs + n_ev, static_cast<uint64_t>(b) << 32);
            for (size_t u = b; u < e; ++u) { const uint64_t* q = p; while (q < evs + n_ev && (*q >> 32) == u) ++q; U[u].colours.resize(static_cast<size_t>(q - p)); for (size_t i = 0; p + i < q; ++i) U[u].colours[i] = static_cast<uint32_t>(p[i] & 0xFFFFFFFFull); p = q; }
        });
    }
    uint64_t too_short() const { uint64_t n = 0; for (size_t t = 0; t < per_thread.size(); ++t) n += per_thread[t].too_short; return n; }
    void take_cov(const uint64_t* cv) { parallel_for(n_u, s.n_thr, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) U[u].cov = cv[u]; }); }
    // --gpu: the distinct (unitig, id) events in sorted order and the coverages, back from the device
    bool finish_device() {
        if (!job) return true;
        for (unsigned t = 0; t < s.n_thr; ++t) feeds[t].flush();
        uint64_t* evs = nullptr; uint64_t* cv = nullptr; uint64_t n_ev = 0;
        open_job = false;
        if (end_fn(job, &evs, &n_ev, &cv) != 0 || failed) { fprintf(stderr, "rtk_build_index: --gpu: colouring on the device failed (%s)\n", s.lib.last_error()); return false; }
        take_cov(cv); take_events(evs, n_ev);
        s.lib.free(evs); s.lib.free(cv);
        return true;
    }
    // --gpu --subsample-colours, first half: the reads are all fed, the coverages come back; the events stay on the device
    bool cov_device() {
        if (!job) return true;
        for (unsigned t = 0; t < s.n_thr; ++t) feeds[t].flush();
        uint64_t* cv = nullptr;
        if (cov_fn(job, &cv) != 0 || failed) { fprintf(stderr, "rtk_build_index: --gpu: colouring on the device failed (%s)\n", s.lib.last_error()); return false; }
        take_cov(cv); s.lib.free(cv);
        return true;
    }
    // --gpu --merge-duplicates: the reads are all fed; the events merged in place on the device (tools/index/merge.hpp has the rule), the job stays open
    bool merge_device(uint64_t* ev_before, uint64_t* ev_after, uint64_t* ids_before, uint64_t* ids_after, uint64_t* classes_above_one, uint64_t* largest) {
        for (unsigned t = 0; t < s.n_thr; ++t) feeds[t].flush();
        if (failed || merge_fn(job, ev_before, ev_after, ids_before, ids_after) != 0 || merge_classes_fn(job, classes_above_one, largest) != 0) {
            fprintf(stderr, "rtk_build_index: --gpu: merging the ids on the device failed (%s)\n", s.lib.last_error()); return false; }
        return true;
    }
    // second half: the events thinned and renumbered on the device (tools/index/subsample.hpp has the rule), only the kept ones copied back
    bool finish_device_subsampled(const uint8_t* bin_of_unitig, const uint8_t* forced_candidate, const uint8_t* bin_is_sampled, uint32_t n_bins, double rate, uint64_t seed,
                                  uint64_t* ev_before, uint64_t* ev_after, uint64_t* ids_before, uint64_t* ids_after) {
        uint64_t* evs = nullptr; uint64_t n_ev = 0;
        open_job = false;
        if (end_sub_fn(job, bin_of_unitig, forced_candidate, bin_is_sampled, n_bins, static_cast<uint32_t>(s.o.min_cov_vertices), rate, seed, &evs, &n_ev, ev_before, ids_before, ids_after) != 0) {
            fprintf(stderr, "rtk_build_index: --gpu: subsampling on the device failed (%s)\n", s.lib.last_error()); return false; }
        *ev_after = n_ev;
        take_events(evs, n_ev); s.lib.free(evs);
        return true;
    }
    // the threads' counts and events into the unitigs; the colours sorted, each id once
    void finish_host() {
        if (job) return;
        for (unsigned t = 0; t < s.n_thr; ++t) {
            for (size_t u = 0; u < n_u; ++u) U[u].cov += cov[t][u];
            for (size_t e = 0; e < ev[t].size(); ++e) U[ev[t][e].first].colours.push_back(ev[t][e].second);
            std::vector<uint64_t>().swap(cov[t]); std::vector<std::pair<uint32_t, uint32_t> >().swap(ev[t]);
        }
        parallel_for(U.size(), s.o.fast ? s.n_thr : 1u, [&](size_t b, size_t e, unsigned) { for (size_t i = b; i < e; ++i) { std::sort(U[i].colours.begin(), U[i].colours.end()); U[i].colours.erase(std::unique(U[i].colours.begin(), U[i].colours.end()), U[i].colours.end()); } });
    }
};

// a colouring record without a quality string of its own length under --colour-min-conf: the one message of all routes
inline void colour_no_quality(const std::string& file) { fprintf(stderr, "rtk_build_index: --colour-min-conf: %s holds a record without a quality string of its own length (FASTQ input is needed)\n", file.c_str()); }

// ---- --pair-by-name (DESIGN.md section 4 [A18]): the id of a record is the rank of its NAME by first appearance over the whole colouring input -- the -s files in
// the order given, records in file order --, as the reference's name_hmap hands ids out (src/Graph.cpp:1595-1608, 1800-1804): mates in separate files share one id.
// Every record counts, so an interleaved file gets the ids of the name-change rule. A name sweep ahead of the colouring notes the hash of every record's name
// (common/name_hash.hpp) under the record's ordinal; pair_ids() turns the hashes into ids (--gpu: rtk_index_pair_ids, csrc/hip/rtk_index_pairs.h; else pair_ids_host);
// the mapping sweep of the source then feeds record r with ids[r]. Sink, events and every later step see ids as before.
struct PairNames {
    std::vector<uint64_t> hash; // [ordinal]
    std::vector<uint32_t> ids;  // [ordinal]
    uint64_t n_ids = 0;
    size_t chunk_bytes = 32u << 20; // source 3: bytes per range (RTK_INDEX_CHUNK: tests, many ranges)
    std::vector<std::vector<uint64_t> > range_first; // source 3, per file: the ordinal of the first record of every range, and past the last
    PairNames() { const char* e = getenv("RTK_INDEX_CHUNK"); if (e && strtoull(e, nullptr, 10) >= 1024) chunk_bytes = static_cast<size_t>(strtoull(e, nullptr, 10)); }
};

// ids[r] = the number of distinct hashes whose first record precedes the first record of hash[r]. The records go into 256 buckets by the top byte of the hash, in
// ordinal order; a bucket is sorted by (hash, ordinal) on a thread, the first of a run is its leader; the ids are the ranks of the leaders.
inline void pair_ids_host(const std::vector<uint64_t>& hash, unsigned n_thr, std::vector<uint32_t>& ids, uint64_t* n_ids) {
    const size_t n = hash.size();
    std::vector<size_t> start(257, 0);
    for (size_t i = 0; i < n; ++i) ++start[(hash[i] >> 56) + 1];
    for (size_t b = 0; b < 256; ++b) start[b + 1] += start[b];
    std::vector<std::pair<uint64_t, uint32_t> > rec(n); std::vector<uint32_t> leader(n);
    { std::vector<size_t> at(start.begin(), start.end() - 1); for (size_t i = 0; i < n; ++i) rec[at[hash[i] >> 56]++] = std::make_pair(hash[i], static_cast<uint32_t>(i)); }
    parallel_for(256, n_thr, [&](size_t b, size_t e, unsigned) {
        for (size_t bk = b; bk < e; ++bk) {
            std::sort(rec.begin() + start[bk], rec.begin() + start[bk + 1]);
            uint32_t head = 0;
            for (size_t i = start[bk]; i < start[bk + 1]; ++i) { if (i == start[bk] || rec[i].first != rec[i - 1].first) head = rec[i].second; leader[rec[i].second] = head; }
        }
    });
    uint32_t next = 0; ids.assign(n, 0);
    for (size_t j = 0; j < n; ++j) ids[j] = leader[j] == j ? next++ : ids[leader[j]]; // (leader[j] <= j)
    *n_ids = next;
}

template <class KM> static bool pair_ids(IndexBuild<KM>& s, PairNames& pn, const char** where) {
    const size_t n = pn.hash.size(); *where = "host threads";
    if (n >= (1ull << 32)) { fprintf(stderr, "rtk_build_index: --pair-by-name: 2^32 records or more (an id has 32 bits)\n"); return false; }
    if (s.o.gpu && n) { // a library without the entry, or a device without the room: said, and paired here
        HipLib::pair_ids_fn fn = nullptr; pn.ids.assign(n, 0);
        if (!s.lib.handle || !s.lib.get(fn, "rtk_index_pair_ids")) fprintf(stderr, "rtk_build_index: --gpu: %s lacks rtk_index_pair_ids: read names paired on the host threads\n", s.lib.path.c_str());
        else if (fn(0, pn.hash.data(), n, pn.ids.data(), &pn.n_ids) == 0) { *where = "device"; return true; }
        else fprintf(stderr, "rtk_build_index: --gpu: read names paired on the host threads (%s)\n", s.lib.last_error());
    }
    pair_ids_host(pn.hash, s.n_thr, pn.ids, &pn.n_ids);
    return true;
}

// the name sweep of source 1: the input read once more, for the names only
template <class KM> static bool pair_names_from_reader(IndexBuild<KM>& s, const std::vector<std::string>& col_in, PairNames& pn) {
    std::string name, seq, qual;
    for (size_t f = 0; f < col_in.size(); ++f) {
        FastxReader fr; if (!fr.open(col_in[f], s.o.fast ? static_cast<int>(s.n_thr < 8 ? s.n_thr : 8) : 0)) { fprintf(stderr, "rtk_build_index: cannot open %s\n", col_in[f].c_str()); return false; }
        while (fr.next(name, seq, qual)) pn.hash.push_back(name_hash(name.data(), pair_name_len(name.data(), name.size())));
        if (fr.failed()) { fprintf(stderr, "rtk_build_index: %s ends in a damaged or cut-short gzip stream\n", col_in[f].c_str()); return false; }
    }
    return true;
}
// the name sweep of source 3 (it takes the place of the counting sweep): every range parsed by a thread keeps the hashes of its records; the running sums of the
// ranges' record counts stitch them together and give every range the ordinal of its first record
template <class KM> static bool pair_names_from_plain_ranges(IndexBuild<KM>& s, const std::vector<std::string>& col_in, PairNames& pn) {
    pn.range_first.assign(col_in.size(), std::vector<uint64_t>());
    for (size_t f = 0; f < col_in.size(); ++f) {
        PlainChunks pc; if (!pc.open(col_in[f], pn.chunk_bytes)) { fprintf(stderr, "rtk_build_index: cannot open %s\n", col_in[f].c_str()); return false; }
        const size_t nc = pc.n_chunks();
        std::vector<std::vector<uint64_t> > h(nc); std::atomic<int> bad(0); std::atomic<size_t> nx(0); std::vector<std::thread> th;
        for (unsigned t = 0; t < s.n_thr; ++t) th.emplace_back([&]() {
            for (;;) { const size_t i = nx.fetch_add(1); if (i >= nc) break;
                PackedReads r(false); if (!pc.parse_chunk(i, r)) { bad = 1; break; }
                h[i].resize(r.size());
                for (size_t x = 0; x < r.size(); ++x) h[i][x] = name_hash(r.name(x), pair_name_len(r.name(x), r.name_len(x)));
            } });
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
        if (bad) return false;
        std::vector<uint64_t>& first = pn.range_first[f]; first.assign(nc + 1, pn.hash.size());
        for (size_t i = 0; i < nc; ++i) { first[i] = pn.hash.size(); pn.hash.insert(pn.hash.end(), h[i].begin(), h[i].end()); std::vector<uint64_t>().swap(h[i]); }
        first[nc] = pn.hash.size();
    }
    return true;
}
// the line a user of split files must see: how the names paired up; and the warning when they did not
inline void pair_summary(const PairNames& pn, bool several_files) {
    std::vector<uint32_t> per(pn.n_ids, 0); uint64_t one = 0, two = 0, more = 0;
    for (size_t r = 0; r < pn.ids.size(); ++r) ++per[pn.ids[r]];
    for (size_t i = 0; i < per.size(); ++i) { if (per[i] == 1) ++one; else if (per[i] == 2) ++two; else ++more; }
    fprintf(stderr, "rtk_build_index: --pair-by-name: %llu records, %llu names: %llu with one record, %llu with two, %llu with more\n", static_cast<unsigned long long>(pn.ids.size()),
            static_cast<unsigned long long>(pn.n_ids), static_cast<unsigned long long>(one), static_cast<unsigned long long>(two), static_cast<unsigned long long>(more));
    if (several_files && !pn.ids.empty() && two == 0 && more == 0)
        fprintf(stderr, "rtk_build_index: --pair-by-name: warning: no name has two records: the mates do not seem to share their names (a name is the header up to the first blank, without a trailing /1 or /2), every read is coloured on its own\n");
}

// Source 1, any input: one reader parses the records and numbers them (a pair keeps one id: the id is the number of name changes before the read;
// every read its own id with --colour-reads; pn != nullptr, --pair-by-name: record r gets pn->ids[r]), worker threads take pieces of about 1 MB from a bounded queue.
template <class KM> static bool colour_from_reader(IndexBuild<KM>& s, ColourSink<KM>& sink, const std::vector<std::string>& col_in, bool by_read, const PairNames* pn) {
    struct Chunk { std::vector<std::string> seq, qual; std::vector<uint32_t> id; size_t bytes = 0; }; // (qual: filled with a confidence threshold only)
    const bool with_qual = sink.q_min != 0;
    std::mutex mq; std::condition_variable cv_put, cv_get; std::deque<std::unique_ptr<Chunk> > q; bool done = false, ok = true;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < s.n_thr; ++t) th.emplace_back([&, t]() {
        while (true) {
            std::unique_ptr<Chunk> c;
            { std::unique_lock<std::mutex> lk(mq); cv_get.wait(lk, [&]() { return !q.empty() || done; }); if (q.empty()) return; c = std::move(q.front()); q.pop_front(); }
            cv_put.notify_one();
            for (size_t r = 0; r < c->seq.size(); ++r) sink.read(t, c->seq[r].data(), with_qual ? c->qual[r].data() : nullptr, c->seq[r].size(), c->id[r]);
        }
    });
    std::string name, seq, qual, prev_name;
    uint32_t pair_id = 0; bool first = true; size_t ordinal = 0;
    std::unique_ptr<Chunk> cur(new Chunk());
    auto flush = [&]() { if (cur->seq.empty()) return; { std::unique_lock<std::mutex> lk(mq); cv_put.wait(lk, [&]() { return q.size() < 4u * s.n_thr; }); q.push_back(std::move(cur)); } cv_get.notify_one(); cur.reset(new Chunk()); };
    for (size_t f = 0; f < col_in.size() && ok; ++f) {
        FastxReader fr; if (!fr.open(col_in[f], s.o.fast ? static_cast<int>(s.n_thr < 8 ? s.n_thr : 8) : 0)) { fprintf(stderr, "rtk_build_index: cannot open %s\n", col_in[f].c_str()); ok = false; break; }
        while (fr.next(name, seq, qual)) {
            for (size_t x = 0; x < seq.size(); ++x) seq[x] = static_cast<char>(seq[x] & 0xDF);
            name.erase(pair_name_len(name.data(), name.size()));
            if (pn) { if (ordinal >= pn->ids.size()) { fprintf(stderr, "rtk_build_index: --pair-by-name: %s holds more records than the name sweep saw\n", col_in[f].c_str()); ok = false; break; } pair_id = pn->ids[ordinal++]; }
            else if (first) { first = false; prev_name = name; }
            else if (by_read || name != prev_name) { ++pair_id; prev_name = name; }
            if (with_qual) { if (qual.size() != seq.size()) { colour_no_quality(col_in[f]); ok = false; break; } cur->qual.push_back(std::string()); cur->qual.back().swap(qual); }
            cur->bytes += seq.size(); cur->seq.push_back(std::string()); cur->seq.back().swap(seq); cur->id.push_back(pair_id);
            if (cur->bytes >= (1u << 20)) flush();
        }
        if (ok && fr.failed()) { fprintf(stderr, "rtk_build_index: %s ends in a damaged or cut-short gzip stream\n", col_in[f].c_str()); ok = false; }
    }
    flush();
    { std::lock_guard<std::mutex> lk(mq); done = true; }
    cv_get.notify_all();
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
    return ok;
}

// Source 2, --fast on `sample:` specs: reads sampled from a reference on the fly (common/sample_source.hpp): pair p of a source has the id (pairs of the
// sources before it) + p (the number of name changes before it: mates share the name "s<p>"); ranges of pairs generated by all threads
template <class KM> static bool colour_from_samples(IndexBuild<KM>& s, ColourSink<KM>& sink, const std::vector<std::string>& col_in) {
    uint64_t id_base = 0;
    for (size_t f = 0; f < col_in.size(); ++f) {
        std::string err; std::shared_ptr<SampleSource> ss = SampleSource::get(col_in[f], &err);
        if (!ss) { fprintf(stderr, "rtk_build_index: %s\n", err.c_str()); return false; }
        if (id_base + ss->n_pairs() > 0xFFFFFFFFull) { fprintf(stderr, "rtk_build_index: more than 2^32 read pairs\n"); return false; }
        const uint64_t per = 1 << 14, n_ch = (ss->n_pairs() + per - 1) / per; const uint32_t L = ss->read_len();
        std::atomic<uint64_t> nx(0);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < s.n_thr; ++t) th.emplace_back([&, t]() {
            std::string m(2 * static_cast<size_t>(L), 'A');
            for (;;) { const uint64_t c = nx.fetch_add(1); if (c >= n_ch) break;
                const uint64_t p0 = c * per, p1 = std::min<uint64_t>(ss->n_pairs(), p0 + per);
                for (uint64_t p = p0; p < p1; ++p) { ss->pair(p, &m[0], &m[L]); for (int mate = 0; mate < 2; ++mate) sink.read(t, m.data() + mate * L, nullptr, L, static_cast<uint32_t>(id_base + p)); }
            } });
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
        id_base += ss->n_pairs();
    }
    return true;
}

// Source 3, --fast on plain files: byte ranges of the files parsed and looked up by all threads. The id of a read is the number of name changes
// before it (every read with --colour-reads), so a first sweep over the ranges counts the changes inside each and notes its first and last
// name; the running sums give every range the id of its first read; the second sweep maps the reads. pn != nullptr (--pair-by-name): the name sweep
// (pair_names_from_plain_ranges, over the same ranges) has taken the place of the first sweep, and record x of range i gets pn->ids[range_first[i] + x].
template <class KM> static bool colour_from_plain_ranges(IndexBuild<KM>& s, ColourSink<KM>& sink, const std::vector<std::string>& col_in, bool by_read, const PairNames* pn) {
    struct RangeInfo { uint32_t changes = 0; uint64_t n_reads = 0; std::string first, last; };
    uint32_t next_id = 0; bool have_prev = false; std::string prev_last;
    for (size_t f = 0; f < col_in.size(); ++f) {
        PlainChunks pc; if (!pc.open(col_in[f], pn ? pn->chunk_bytes : 32u << 20)) { fprintf(stderr, "rtk_build_index: cannot open %s\n", col_in[f].c_str()); return false; }
        const size_t nc = pc.n_chunks();
        if (pn && pn->range_first[f].size() != nc + 1) { fprintf(stderr, "rtk_build_index: --pair-by-name: %s is not the file the name sweep saw\n", col_in[f].c_str()); return false; }
        std::vector<RangeInfo> info(nc); std::vector<uint32_t> id0(nc, 0); // id0: id of the first read of every range
        std::atomic<int> bad(0), no_quality(0); const bool with_qual = sink.q_min != 0;
        // sweep(map the reads, or only count): every range parsed by a thread; the names walked, the changes counted from id0 of the range
        auto sweep = [&](bool map) {
            std::atomic<size_t> nx(0); std::vector<std::thread> th;
            for (unsigned t = 0; t < s.n_thr; ++t) th.emplace_back([&, t]() {
                for (;;) { const size_t i = nx.fetch_add(1); if (i >= nc) break;
                    PackedReads r(with_qual); if (!pc.parse_chunk(i, r)) { bad = 1; break; }
                    RangeInfo& ri = info[i]; uint32_t id = id0[i]; const char* pp = nullptr; size_t pl = 0;
                    if (pn && pn->range_first[f][i + 1] - pn->range_first[f][i] != r.size()) { bad = 1; break; } // (the file changed under the two sweeps)
                    for (size_t x = 0; x < r.size(); ++x) {
                        const char* p = r.name(x); const size_t n = pair_name_len(p, r.name_len(x));
                        if (pn) id = pn->ids[pn->range_first[f][i] + x];
                        else if (x != 0 && (by_read || n != pl || memcmp(p, pp, n) != 0)) ++id;
                        pp = p; pl = n;
                        if (with_qual && !r.qual(x)) { no_quality = 1; bad = 1; break; }
                        if (map) sink.read(t, r.seq(x), with_qual ? r.qual(x) : nullptr, r.seq_len(x), id);
                        else if (x == 0) ri.first.assign(p, n);
                    }
                    if (!map) { ri.n_reads = r.size(); ri.changes = id - id0[i]; if (r.size()) ri.last.assign(pp, pl); }
                } });
            for (size_t t = 0; t < th.size(); ++t) th[t].join();
        };
        if (!pn) sweep(false);
        if (no_quality) colour_no_quality(col_in[f]);
        if (bad) return false;
        for (size_t i = 0; i < nc && !pn; ++i) {
            if (info[i].n_reads == 0) { id0[i] = next_id; continue; }
            if (have_prev && (by_read || info[i].first != prev_last)) ++next_id;
            id0[i] = next_id; next_id += info[i].changes; have_prev = true; prev_last = info[i].last;
        }
        sweep(true);
        if (bad) return false;
    }
    return true;
}

template <class KM> static bool colour_and_cover(IndexBuild<KM>& s) {
    // second-pass index: the reads that colour the graph are the (pass-1 corrected) long reads, every read its own id
    // (addCoverage(dbg, opt_pass2, ..., long_read_correct = true), src/Ratatosk.cpp:1218)
    const bool by_read = !s.o.colour_files.empty();
    const std::vector<std::string>& col_in = by_read ? s.o.colour_files : s.o.in_files;
    bool all_sampled = s.o.fast && !by_read && !col_in.empty(), all_plain = s.o.fast;
    for (size_t f = 0; f < col_in.size(); ++f) { all_sampled = all_sampled && SampleSource::is_spec(col_in[f]); all_plain = all_plain && PlainChunks::is_plain(col_in[f]); }
    // --pair-by-name (never next to --colour-reads or a sample: source): the name sweep and the ids ahead of the mapping sweep, and ahead of the sink, so that the
    // lap holds the option's own work and not the set-up of the colour job
    std::unique_ptr<PairNames> pn;
    if (s.o.pair_by_name) {
        pn.reset(new PairNames());
        const auto t0 = std::chrono::steady_clock::now(); auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        if (!(all_plain ? pair_names_from_plain_ranges(s, col_in, *pn) : pair_names_from_reader(s, col_in, *pn))) return false;
        const double t_sweep = since(); const char* where = "";
        if (!pair_ids(s, *pn, &where)) return false;
        if (s.knobs.trace) fprintf(stderr, "rtk_build_index: read names: sweep %.3f s (%s), ids %.3f s (%s)\n", t_sweep, all_plain ? "byte ranges on all threads" : "one reader", since() - t_sweep, where);
        if (s.knobs.trace || col_in.size() >= 2) pair_summary(*pn, col_in.size() >= 2);
        std::vector<uint64_t>().swap(pn->hash);
        s.lap("read names paired");
    }
    std::shared_ptr<ColourSink<KM> > sink_p = std::make_shared<ColourSink<KM> >(s); ColourSink<KM>& sink = *sink_p;
    const bool ok = all_sampled ? colour_from_samples(s, sink, col_in) : (all_plain ? colour_from_plain_ranges(s, sink, col_in, by_read, pn.get()) : colour_from_reader(s, sink, col_in, by_read, pn.get()));
    if (s.knobs.trace && (sink.q_min || sink.min_len)) { // (the same line on every route)
        fprintf(stderr, "rtk_build_index: colour filter:");
        if (sink.q_min) fprintf(stderr, " bases of the colouring reads with a quality byte below %u masked%s", static_cast<unsigned>(sink.q_min), sink.min_len ? ";" : "");
        if (sink.min_len) fprintf(stderr, " %llu colouring reads shorter than %llu left out", static_cast<unsigned long long>(sink.too_short()), static_cast<unsigned long long>(sink.min_len));
        fprintf(stderr, "\n");
    }
    const bool sub_there = s.o.subsample && sink.job && sink.end_sub_fn, merge_there = sink.job && sink.merge_fn;
    if (sub_there || merge_there) { // the events wait on the device for the merging or the subsampling step
        if ((sub_there && !sink.cov_device()) || !ok) return false;
        s.colour_sink = sink_p;
        return true;
    }
    if (!sink.finish_device() || !ok) return false;
    sink.finish_host();
    return true;
}

} // namespace rtk

#endif
