// rtk_build_index: what is worked out per unitig once colours and coverage are known -- adjacency, branching and edge bits, short cycles,
// SNP annotations (--snps), the global / local colour split.
#ifndef RTK_TOOLS_INDEX_ANNOTATE_HPP
#define RTK_TOOLS_INDEX_ANNOTATE_HPP

#include <memory>
#include <queue>
#include <set>

#include "state.hpp"

namespace rtk {

// ---- adjacency and branching (structure: the sequences and the k-mer table alone), then the edge bits (the colours) ----
template <class KM> static void adjacency_structure(IndexBuild<KM>& s) {
    const int k = s.k; const size_t n = s.U.size(); const std::vector<Unitig>& U = s.U;
    s.adj.resize(n); s.headk.resize(n); s.tailk.resize(n); s.kmcov.assign(n, 0); s.shared.assign(n, 0); s.cycles.assign(n, std::string()); s.ambiguity.assign(n, std::vector<uint32_t>()); // (what the later steps fill per unitig)
    parallel_for(n, s.o.fast ? s.n_thr : 1u, [&](size_t b0, size_t e0, unsigned) { for (size_t u = b0; u < e0; ++u) { // (unitigs are independent: the table is only read)
        const std::string& q = U[u].seq;
        km_encode<KM>(q.c_str() + q.size() - k, k, s.tailk[u]);
        km_encode<KM>(q.c_str(), k, s.headk[u]);
        const KM ends[2] = { s.tailk[u], kmer_revcomp(s.headk[u], k) }; // last k-mer in walk direction fw / rev
        int deg[2] = {0, 0};
        for (int d = 0; d < 2; ++d) for (uint64_t b = 0; b < 4; ++b) {
            s.adj[u].u[d][b] = -1;
            const KM y = ((ends[d] << 2) | static_cast<KM>(b)) & s.mask;
            const uint64_t* v = s.km.slot(kmer_canonical(y, k), false);
            if (!v) continue;
            s.adj[u].u[d][b] = static_cast<int64_t>((*v >> 32) - 1);
            ++deg[d];
        }
        const uint64_t cov = std::min<uint64_t>(U[u].cov, 0x7fffffffULL);
        s.kmcov[u] = (cov << 31) | ((deg[0] > 1 || deg[1] > 1) ? (1ULL << 63) : 0ULL);
    } });
}
template <class KM> static void edge_bits(IndexBuild<KM>& s) {
    const size_t n = s.U.size(); const std::vector<Unitig>& U = s.U;
    parallel_for(n, s.o.fast ? s.n_thr : 1u, [&](size_t b0, size_t e0, unsigned) { for (size_t u = b0; u < e0; ++u)
        for (int d = 0; d < 2; ++d) for (uint64_t b = 0; b < 4; ++b) {
            const int64_t w = s.adj[u].u[d][b];
            if (w >= 0 && shared_count(U[u].colours, U[static_cast<size_t>(w)].colours) >= s.o.min_cov_vertices) s.shared[u] |= (d == 0) ? ((1ULL << b) << 4) : (1ULL << b); // idx(A,C,G,T)=1,2,4,8 (src/Common.hpp:260,358)
        }
    });
}

// ---- short cycles (restatement of detectShortCycles, src/Graph.cpp:4660-4735): for every unitig U in forward direction, breadth
// first over paths U -> X1 .. Xm -> U whose interior spans fewer than k + 1 k-mers, following only edges carrying an edge bit and
// unitigs sharing >= min_cov colours with U; a cycle counts when its interior unitigs are distinct and U's colours intersected
// with theirs keep >= min_cov ids. Stored per unitig as the entering bases of X1..Xm (Path::getMiddleCompactedPath), NUL-terminated.
template <class KM> static void short_cycles(IndexBuild<KM>& s) {
    const int k = s.k; const size_t n = s.U.size(); const std::vector<Unitig>& U = s.U; const std::vector<Nb>& adj = s.adj; std::vector<uint64_t>& shared = s.shared;
    const KM mask = s.mask; const size_t min_cov_vertices = s.o.min_cov_vertices; std::vector<std::string>& cycles = s.cycles; const std::vector<KM>& headk = s.headk; const std::vector<KM>& tailk = s.tailk;
    auto n_km = [&](size_t u) { return U[u].seq.size() - static_cast<size_t>(k) + 1; };
    struct Step { size_t u; bool fw; char base; };
    size_t n_cyc_unitigs = 0;
    auto cycles_of = [&](size_t u0) {
        std::queue<std::vector<Step> > q;
        { std::vector<Step> p0; Step s0; s0.u = u0; s0.fw = true; s0.base = 0; p0.push_back(s0); q.push(p0); }
        while (!q.empty()) {
            const std::vector<Step> path = q.front(); q.pop();
            const Step cur = path.back();
            const KM endk = cur.fw ? tailk[cur.u] : kmer_revcomp(headk[cur.u], k);
            for (uint64_t b = 0; b < 4; ++b) {
                const int64_t w = adj[cur.u].u[cur.fw ? 0 : 1][b];
                if (w < 0) continue;
                const uint64_t bit = cur.fw ? ((1ULL << b) << 4) : (1ULL << b);
                if (!(shared[cur.u] & bit)) continue;                                                       // edge seen in enough reads
                if (shared_count(U[cur.u].colours, U[u0].colours) < min_cov_vertices) continue;            // still read-compatible with the start
                const KM y = ((endk << 2) | static_cast<KM>(b)) & mask;
                const bool w_fw = (y == headk[static_cast<size_t>(w)]);
                if (static_cast<size_t>(w) == u0 && w_fw) { // came back to the start unitig, same strand
                    bool distinct = true;
                    for (size_t i = 1; i < path.size() && distinct; ++i) for (size_t j = i + 1; j < path.size() && distinct; ++j) if (path[i].u == path[j].u && path[i].fw == path[j].fw) distinct = false;
                    if (!distinct) continue;
                    std::vector<uint32_t> pid = U[u0].colours;
                    for (size_t i = 1; i < path.size() && pid.size() >= min_cov_vertices; ++i) { std::vector<uint32_t> t; std::set_intersection(pid.begin(), pid.end(), U[path[i].u].colours.begin(), U[path[i].u].colours.end(), std::back_inserter(t)); pid.swap(t); }
                    if (pid.size() >= min_cov_vertices) { std::string c; for (size_t i = 1; i < path.size(); ++i) c.push_back(path[i].base); cycles[u0] += c; cycles[u0].push_back('\0'); }
                } else {
                    size_t interior = 0; for (size_t i = 1; i < path.size(); ++i) interior += n_km(path[i].u);
                    if (interior + static_cast<size_t>(k) - 1 < 2 * static_cast<size_t>(k)) { // path.length() - um_start.len < 2k
                        std::vector<Step> nx = path; Step st; st.u = static_cast<size_t>(w); st.fw = w_fw; st.base = "ACGT"[b]; nx.push_back(st); q.push(nx);
                    }
                }
            }
        }
    };
    // (the search of one unitig reads the edge bits of others: the short-cycle flags are set afterwards, not during the searches)
    parallel_for(n, s.o.fast ? s.n_thr : 1u, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) cycles_of(u); });
    for (size_t u0 = 0; u0 < n; ++u0) if (!cycles[u0].empty()) { shared[u0] |= 0x100ULL; ++n_cyc_unitigs; }
    fprintf(stderr, "rtk_build_index: %zu unitigs in short cycles\n", n_cyc_unitigs);
}

// The graph k-mers ONE SUBSTITUTION away from a k-mer, without spelling the 3k variants: such a neighbour shares the first k/2 bases or the
// last k - k/2 bases with it. The sorted CANONICAL solid k-mers are view one as they stand (the first half leads; not copied); view two holds the same
// k-mers rotated so that the last half leads, sorted; a table of the first 24 key bits sits in front of each. An oriented k-mer y is in the graph when
// its canonical form is, so the neighbours of x are the entries one substitution away from x plus the reverse complements of the entries one substitution
// away from rc(x) (offset k-1-j, complemented base): a query scans the few entries that share a half with x, then with rc(x). Round 5: 8 bytes per
// solid k-mer beside the k-mer set (26 GB at 3 Gb; the first version kept both orientations in both views, 103 GB + a sorting copy: `--snps` did not fit
// a 3 Gb run). Used by the SNP search of --fast, and of --gpu when the candidates are not found on the device (the plain path probes every variant in the k-mer table;
// csrc/hip/rtk_index_snps.h builds the same two views in HBM for rtk_index_snp_candidates).
template <class KM> struct NeighbourIndex { // KM: uint64_t, or u128 for two-word k-mers (16 bytes per solid k-mer beside the k-mer set)
    int k = 0, hi_n = 0, lo_n = 0; KM lomask = 0;
    const KM* a = nullptr; size_t n = 0; std::vector<KM> b; std::vector<uint64_t> ia, ib; int shift = 0; // ia / ib: first entry of every value of the top 24 bits of the 2k-bit key
    static int ctz(KM m) { const uint64_t lo = static_cast<uint64_t>(m); return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(static_cast<uint64_t>(m >> (sizeof(KM) > 8 ? 64 : 0))); }
    KM rot(KM x) const { return ((x & lomask) << (2 * hi_n)) | (x >> (2 * lo_n)); }
    KM unrot(KM r) const { return ((r & ((static_cast<KM>(1) << (2 * hi_n)) - 1)) << (2 * lo_n)) | (r >> (2 * hi_n)); }
    void build(const std::vector<KM>& solid, int k_, unsigned n_thr) {
        k = k_; hi_n = k / 2; lo_n = k - hi_n; lomask = (static_cast<KM>(1) << (2 * lo_n)) - 1;
        a = solid.data(); n = solid.size();
        // view two without a second copy: the rotated keys are counted by their top 12 bits per thread slice, scattered to their bucket's place, every bucket sorted by a thread
        const int bsh = 2 * k > 12 ? 2 * k - 12 : 0; const size_t nbk = static_cast<size_t>(1) << (2 * k - bsh);
        if (n_thr == 0) n_thr = 1;
        std::vector<std::vector<size_t> > cnt(n_thr, std::vector<size_t>(nbk, 0));
        parallel_for(n, n_thr, [&](size_t bb, size_t ee, unsigned t) { for (size_t i = bb; i < ee; ++i) ++cnt[t][static_cast<size_t>(rot(a[i]) >> bsh)]; });
        std::vector<size_t> start(nbk + 1, 0);
        { size_t at = 0; for (size_t q = 0; q < nbk; ++q) { start[q] = at; for (unsigned t = 0; t < n_thr; ++t) { const size_t c = cnt[t][q]; cnt[t][q] = at; at += c; } } start[nbk] = at; }
        b.resize(n);
        parallel_for(n, n_thr, [&](size_t bb, size_t ee, unsigned t) { for (size_t i = bb; i < ee; ++i) { const KM r = rot(a[i]); b[cnt[t][static_cast<size_t>(r >> bsh)]++] = r; } });
        { std::atomic<size_t> nx(0); std::vector<std::thread> th;
          for (unsigned t = 0; t < n_thr; ++t) th.emplace_back([&]() { for (;;) { const size_t q = nx.fetch_add(1); if (q >= nbk) break; std::sort(b.begin() + start[q], b.begin() + start[q + 1]); } });
          for (size_t t = 0; t < th.size(); ++t) th[t].join(); }
        shift = 2 * k > 24 ? 2 * k - 24 : 0;
        const size_t nb = (static_cast<size_t>(1) << (2 * k - shift)) + 1;
        auto index = [&](const KM* v, std::vector<uint64_t>& ix) { ix.assign(nb, 0); for (size_t i = 0; i < n; ++i) ++ix[static_cast<size_t>(v[i] >> shift) + 1]; for (size_t i = 0; i + 1 < nb; ++i) ix[i + 1] += ix[i]; };
        std::thread t2([&]() { index(b.data(), ib); }); index(a, ia); t2.join();
    }
    // the canonical k-mers one substitution away from x, as (offset << 2 | base) of the ORIENTED neighbour of the caller's k-mer (flipped: x is its reverse complement)
    void scan(KM x, bool flipped, uint32_t* found, int& nf) const {
        const KM m55 = ~static_cast<KM>(0) / 3; // 0101...01
        auto put = [&](int bit, KM y) { int j = k - 1 - bit / 2; uint32_t base = static_cast<uint32_t>((y >> bit) & static_cast<KM>(3)); if (flipped) { j = k - 1 - j; base = 3u - base; } if (nf < 192) found[nf++] = (static_cast<uint32_t>(j) << 2) | base; };
        { // same first half: the differing base lies in the last lo_n bases
            const KM lo_key = x & ~lomask, hi_key = x | lomask;
            size_t i = ia[static_cast<size_t>(lo_key >> shift)]; const size_t e = ia[static_cast<size_t>(hi_key >> shift) + 1];
            i = static_cast<size_t>(std::lower_bound(a + i, a + e, lo_key) - a);
            for (; i < e && a[i] <= hi_key; ++i) { const KM d = a[i] ^ x; if (d == 0) continue; const KM m = (d | (d >> 1)) & m55; if (m & (m - 1)) continue; put(ctz(m), a[i]); }
        }
        { // same last half: the differing base lies in the first hi_n bases
            const KM r = rot(x), himask = (static_cast<KM>(1) << (2 * hi_n)) - 1; const KM lo_key = r & ~himask, hi_key = r | himask;
            size_t i = ib[static_cast<size_t>(lo_key >> shift)]; const size_t e = ib[static_cast<size_t>(hi_key >> shift) + 1];
            i = static_cast<size_t>(std::lower_bound(b.begin() + i, b.begin() + e, lo_key) - b.begin());
            for (; i < e && b[i] <= hi_key; ++i) { const KM y = unrot(b[i]); const KM d = y ^ x; if (d == 0) continue; const KM m = (d | (d >> 1)) & m55; if (m & (m - 1)) continue; put(ctz(m), y); }
        }
    }
    // calls f(offset j, substituted base) for every graph k-mer one substitution away from x, by (j, base) ascending
    template <class F> void neighbours(KM x, F f) const {
        uint32_t found[192]; int nf = 0; // (j << 2 | base): at most 3 per offset, 3k <= 93 in all (a k-mer of a tandem repeat at small k has dozens: 16 slots lost some, found by tests/test_annotators.py)
        scan(x, false, found, nf); scan(kmer_revcomp(x, k), true, found, nf);
        std::sort(found, found + nf);
        for (int i = 0; i < nf; ++i) f(static_cast<int>(found[i] >> 2), static_cast<uint64_t>(found[i] & 3u));
    }
};

// ---- SNP annotations: restatement of detectSNPs (src/Graph.cpp:484-720) with isValidSNPcandidate (src/GraphTraversal.cpp:1057-1147).
// For every unitig with an edge bit: every graph k-mer ONE SUBSTITUTION away from one of its windows (searchSequence(seq, false,
// false, false, true, false), [A2]) that lies on another unitig is a SNP candidate; the position gets the IUPAC union of its base
// and the candidate's base when the other unitig passes isValidSNPcandidate: a breadth-first walk from this unitig, forwards and
// backwards, over edges carrying an edge bit and unitigs sharing >= min_cov colours with this one, until a unitig shares >= min_cov
// colours with the candidate (or 65536 unitigs were seen). The two walks keep their state from candidate to candidate, and a unitig
// that answered one candidate is not expanded further -- reproduced as written. Candidates are visited by (window, substituted
// offset, substituted base): Bifrost's own order inside one window is not known ([D3], canonical rule).
static const char amb_char[16] = {'.', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'}; // getAmbiguity
template <class KM> struct SnpSearch {
    const int k; const KM mask; const size_t min_cov_vertices;
    const std::vector<Unitig>& U; const std::vector<Nb>& adj; const std::vector<uint64_t>& shared; KTable<KM>& km; std::vector<std::vector<uint32_t> >& ambiguity;
    const std::vector<KM>& headk; const std::vector<KM>& tailk;
    std::unique_ptr<NeighbourIndex<KM> > nbx; // --fast: the neighbours from the two sorted views of the k-mer set; else every variant is probed in the table
    // host_search: the candidates are enumerated here (false: they come as a list from the device, no neighbour index is built)
    SnpSearch(IndexBuild<KM>& s, bool host_search) : k(s.k), mask(s.mask), min_cov_vertices(s.o.min_cov_vertices), U(s.U), adj(s.adj), shared(s.shared), km(s.km), ambiguity(s.ambiguity), headk(s.headk), tailk(s.tailk) {
        if (s.o.fast && host_search) { nbx.reset(new NeighbourIndex<KM>()); nbx->build(s.solid, k, s.n_thr); s.lap("1-substitution neighbour index built"); }
    }
    struct Node { size_t u; bool fw; };
    // successors of (u, strand) in A,C,G,T order with the base that is appended
    int successors(const Node& x, Node out[4], int base[4]) const {
        int m = 0;
        const KM endk = x.fw ? tailk[x.u] : kmer_revcomp(headk[x.u], k);
        for (uint64_t b = 0; b < 4; ++b) {
            const int64_t w = adj[x.u].u[x.fw ? 0 : 1][b];
            if (w < 0) continue;
            const KM y = ((endk << 2) | static_cast<KM>(b)) & mask;
            out[m].u = static_cast<size_t>(w); out[m].fw = (y == headk[static_cast<size_t>(w)]); base[m] = static_cast<int>(b); ++m;
        }
        return m;
    }
    bool edge_bit(const Node& x, int b) const { return (shared[x.u] & (x.fw ? ((1ULL << b) << 4) : (1ULL << b))) != 0; }
    struct Walk { std::set<std::pair<size_t, bool> > seen; std::vector<size_t> seen_units; std::queue<Node> q; };
    static const size_t limit_sz_stack = 65536;
    bool explore(Walk& lgt, const Node& a, size_t ub) const {
        if (U[a.u].colours.size() < min_cov_vertices || U[ub].colours.size() < min_cov_vertices) return false;
        if (lgt.seen.empty()) { lgt.q.push(a); lgt.seen.insert(std::make_pair(a.u, a.fw)); lgt.seen_units.push_back(a.u); }
        else if (lgt.seen.size() >= limit_sz_stack) return true;
        while (!lgt.q.empty()) {
            const Node x = lgt.q.front(); lgt.q.pop();
            Node nb[4]; int bs[4];
            const int m = successors(x, nb, bs);
            for (int i = 0; i < m; ++i) {
                if (!edge_bit(x, bs[i])) continue;
                if (!lgt.seen.insert(std::make_pair(nb[i].u, nb[i].fw)).second) continue; // visited (keyed by the mapped head k-mer: unitig + strand)
                lgt.seen_units.push_back(nb[i].u);
                if (shared_count(U[nb[i].u].colours, U[a.u].colours) >= min_cov_vertices) {
                    if (shared_count(U[nb[i].u].colours, U[ub].colours) >= min_cov_vertices) return true;
                    lgt.q.push(nb[i]);
                }
            }
            if (lgt.seen.size() >= limit_sz_stack) return true;
        }
        return false;
    }
    bool is_valid(Walk& fw, Walk& bw, size_t ua, size_t ub) const {
        bool ok_fw = false, ok_bw = false;
        for (size_t i = 0; i < fw.seen_units.size() && !ok_fw; ++i) ok_fw = shared_count(U[fw.seen_units[i]].colours, U[ub].colours) >= min_cov_vertices;
        if (!ok_fw) { Node a; a.u = ua; a.fw = true; ok_fw = explore(fw, a, ub); }
        if (ok_fw) {
            for (size_t i = 0; i < bw.seen_units.size() && !ok_bw; ++i) ok_bw = shared_count(U[bw.seen_units[i]].colours, U[ub].colours) >= min_cov_vertices;
            if (!ok_bw) { Node a; a.u = ua; a.fw = false; ok_bw = explore(bw, a, ub); }
        }
        return ok_fw && ok_bw;
    }
    static unsigned amb_bits(char c) { // getAmbiguityRev (src/Common.hpp:351-399): bit0 A, bit1 C, bit2 G, bit3 T
        switch (c) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8; case 'M': return 3; case 'R': return 5; case 'S': return 6; case 'V': return 7;
                     case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14; case 'N': return 15; default: return 0; } }
    // A candidate of unitig u: the graph holds window p with base `alt` at offset j, on unitig w != u (a SNP candidate cannot be on the same unitig, src/Graph.cpp:523).
    struct Cand { size_t p; int j; uint64_t alt; size_t w; };
    // The candidates of unitig u in the order of the visits: by (window, substituted offset, substituted base). --fast: the neighbours from the two sorted views; else
    // every variant is probed in the table.
    void enumerate(size_t u, std::vector<Cand>& out) {
        out.clear();
        if (!(shared[u] & 0xffULL)) return; // hasSharedPids (src/Graph.cpp:500)
        const std::string& s = U[u].seq;
        KM fw = 0;
        for (size_t i = 0; i < s.size(); ++i) {
            fw = ((fw << 2) | static_cast<KM>(base2bits(s[i]))) & mask;
            if (i + 1 < static_cast<size_t>(k)) continue;
            const size_t p = i + 1 - static_cast<size_t>(k);
            auto probe = [&](int j, uint64_t alt) { // is the window with base `alt` at offset j in the graph, on another unitig?
                const int sh = 2 * (k - 1 - j);
                const KM y = (fw & ~(static_cast<KM>(3) << sh)) | (static_cast<KM>(alt) << sh);
                const uint64_t* v = km.slot(kmer_canonical(y, k), false);
                if (!v) return;
                const size_t w = (*v >> 32) - 1;
                if (w == u) return;
                Cand c; c.p = p; c.j = j; c.alt = alt; c.w = w; out.push_back(c);
            };
            if (nbx) nbx->neighbours(fw, probe); // (the same order)
            else for (int j = 0; j < k; ++j) {
                const uint64_t cur = static_cast<uint64_t>(fw >> (2 * (k - 1 - j))) & 3ULL;
                for (uint64_t alt = 0; alt < 4; ++alt) if (alt != cur) probe(j, alt);
            }
        }
    }
    // The rule over the candidates of unitig u, in the order given: the `tried` bases per position, the unitigs that answered before, the two walks that keep their state
    // from candidate to candidate; then the ambiguity entries of u. A unitig without candidates keeps its bases and gets no entry.
    void replay(size_t u, const Cand* cands, size_t n_cands) {
        if (n_cands == 0) return;
        const std::string& s = U[u].seq;
        std::string seq_final = s, seq_tried = s;
        std::set<size_t> ok, bad;
        Walk lgt_fw, lgt_bw;
        for (size_t c = 0; c < n_cands; ++c) {
            const size_t w = cands[c].w; const uint64_t alt = cands[c].alt;
            const size_t at = cands[c].p + static_cast<size_t>(cands[c].j); // pos_snp_km = first mismatch = the substituted offset
            const unsigned f = amb_bits(seq_final[at]), t = amb_bits(seq_tried[at]), kk = 1u << alt;
            const char cf = amb_char[f | kk], ct = amb_char[t | kk];
            if (seq_tried[at] == ct) continue; // that base was tried at this position before
            seq_tried[at] = ct;
            if (ok.count(w)) seq_final[at] = cf;
            else if (!bad.count(w)) {
                if (is_valid(lgt_fw, lgt_bw, u, w)) { seq_final[at] = cf; ok.insert(w); } else bad.insert(w);
            }
        }
        for (size_t i = 0; i < seq_final.size(); ++i) if (seq_final[i] != 'A' && seq_final[i] != 'C' && seq_final[i] != 'G' && seq_final[i] != 'T') ambiguity[u].push_back(static_cast<uint32_t>((i << 4) + amb_bits(seq_final[i]))); // UnitigData.hpp:448-451
    }
};

// --gpu: the candidates of every unitig with an edge bit from the device (rtk_index_snp_candidates, csrc/hip/rtk_index_snps.h), first per (position, base) only -- the
// later ones return at the `tried` check of the replay (the entry searches in as many passes over the key space as the device's memory asks for). Two words each: u << 32 | p, j << 40 | alt << 32 | w, by (u, p, j, alt). false with the reason in `why`: the
// caller takes the host route.
template <class KM> static bool snp_candidates_device(IndexBuild<KM>& s, std::vector<uint64_t>& cand, std::string& why) {
    HipLib::snp_cand_fn fn = nullptr;
    if (!s.lib.handle || !s.lib.get(fn, "rtk_index_snp_candidates")) { why = s.lib.path + " lacks rtk_index_snp_candidates"; return false; }
    const size_t n_u = s.U.size();
    if (n_u == 0) return true;
    std::vector<uint64_t> off(n_u + 1, 0); for (size_t u = 0; u < n_u; ++u) off[u + 1] = off[u] + s.U[u].seq.size();
    std::string pool(off[n_u], 'A'); std::vector<uint8_t> searched(n_u, 0);
    parallel_for(n_u, s.n_thr, [&](size_t b, size_t e, unsigned) { for (size_t u = b; u < e; ++u) { memcpy(&pool[off[u]], s.U[u].seq.data(), s.U[u].seq.size()); searched[u] = (s.shared[u] & 0xffULL) ? 1 : 0; } });
    uint64_t* list = nullptr; uint64_t n = 0;
    if (fn(0, s.k, pool.data(), off.data(), n_u, searched.data(), 1u /* RTK_SNP_FIRST_PER_SITE */, &list, &n) != 0) { why = s.lib.last_error(); return false; }
    cand.assign(list, list + 2 * n); s.lib.free(list);
    return true;
}

template <class KM> static void snp_annotations(IndexBuild<KM>& s) {
    typedef typename SnpSearch<KM>::Cand Cand;
    std::vector<uint64_t> dev; bool on_device = false;
    if (s.o.gpu && s.knobs.snps_device) {
        std::string why;
        on_device = snp_candidates_device(s, dev, why);
        if (!on_device) fprintf(stderr, "rtk_build_index: --gpu: SNP candidates on the host threads (%s)\n", why.c_str());
    }
    SnpSearch<KM> search(s, !on_device);
    const size_t n = s.U.size();
    // unitigs are independent and the k-mer table is only read: one strided slice per thread
    unsigned nt = std::thread::hardware_concurrency(); if (nt == 0) nt = 1; if (nt > std::max(64u, s.n_thr)) nt = std::max(64u, s.n_thr);
    std::vector<std::thread> th;
    if (on_device) { // only the unitigs that have candidates are replayed: run r of the list = the candidates of one unitig
        std::vector<size_t> run(1, 0); const size_t nc = dev.size() / 2;
        for (size_t c = 1; c < nc; ++c) if ((dev[2 * c] >> 32) != (dev[2 * c - 2] >> 32)) run.push_back(c);
        if (nc) run.push_back(nc);
        for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t]() {
            std::vector<Cand> cands;
            for (size_t r = t; r + 1 < run.size(); r += nt) {
                cands.clear();
                for (size_t c = run[r]; c < run[r + 1]; ++c) { const uint64_t w0 = dev[2 * c], w1 = dev[2 * c + 1]; Cand x; x.p = static_cast<size_t>(w0 & 0xFFFFFFFFULL); x.j = static_cast<int>(w1 >> 40); x.alt = (w1 >> 32) & 3ULL; x.w = static_cast<size_t>(w1 & 0xFFFFFFFFULL); cands.push_back(x); }
                search.replay(static_cast<size_t>(dev[2 * run[r]] >> 32), cands.data(), cands.size());
            } });
    } else {
        std::vector<double> t_search(nt, 0.0), t_replay(nt, 0.0);
        for (unsigned t = 0; t < nt; ++t) th.emplace_back([&, t]() {
            std::vector<Cand> cands; double ts = 0.0, tr = 0.0;
            for (size_t u = t; u < n; u += nt) {
                const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                search.enumerate(u, cands);
                const std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
                search.replay(u, cands.data(), cands.size());
                ts += std::chrono::duration<double>(t1 - t0).count(); tr += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
            }
            t_search[t] = ts; t_replay[t] = tr; });
        for (size_t t = 0; t < th.size(); ++t) th[t].join();
        th.clear();
        if (s.knobs.trace) { double ts = 0.0, tr = 0.0; for (unsigned t = 0; t < nt; ++t) { ts += t_search[t]; tr += t_replay[t]; }
            fprintf(stderr, "rtk_build_index: SNP search on the host threads: candidate search %.2f s, replay %.2f s (summed over %u threads)\n", ts, tr, nt); }
    }
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
    size_t n_amb = 0, n_amb_unitigs = 0;
    for (size_t u = 0; u < n; ++u) { n_amb += s.ambiguity[u].size(); n_amb_unitigs += s.ambiguity[u].empty() ? 0 : 1; }
    fprintf(stderr, "rtk_build_index: %zu SNP annotations on %zu unitigs\n", n_amb, n_amb_unitigs);
}

// ---- global / local colour split (simplified restatement of src/Graph.cpp:2874-2985) ----
// The split is made on the read colours alone: the last s.cover_ids[u].size() colours of unitig u are the ids --cover-edges-from added (cover.hpp); they are
// left out of every set compared here and join the local set at the end (SharedPairID::add puts a fresh id there).
template <class KM> static void colour_split(IndexBuild<KM>& s) {
    const int k = s.k; const size_t n = s.U.size(); const std::vector<Unitig>& U = s.U; const std::vector<Nb>& adj = s.adj; const std::vector<uint64_t>& kmcov = s.kmcov;
    const double global_cov_factor = s.o.global_cov_factor, min_color_sharing = s.o.min_color_sharing;
    std::vector<std::vector<uint32_t> >& global_ids = s.global_ids; std::vector<std::vector<uint32_t> >& local_ids = s.local_ids;
    global_ids.assign(n, std::vector<uint32_t>()); local_ids.assign(n, std::vector<uint32_t>());
    auto n_read = [&](size_t u) { return U[u].colours.size() - (s.cover_ids.empty() ? 0 : s.cover_ids[u].size()); }; // the read colours of u: colours[0 .. n_read(u))
    auto read_end = [&](size_t u) { return U[u].colours.begin() + static_cast<std::ptrdiff_t>(n_read(u)); };
    double tot_cov = 0, tot_km = 0;
    for (size_t u = 0; u < n; ++u) { tot_cov += static_cast<double>(U[u].cov); tot_km += static_cast<double>(U[u].seq.size() - k + 1); }
    const double est_cov = tot_km > 0 ? tot_cov / tot_km : 0.0;
    auto kcov = [&](size_t u) { return static_cast<double>(static_cast<long long>(static_cast<double>(U[u].cov) / static_cast<double>(U[u].seq.size() - k + 1) + 0.5)); };
    std::vector<std::pair<double, size_t> > seeds;
    for (size_t u = 0; u < n; ++u) if ((kmcov[u] >> 63) && kcov(u) >= global_cov_factor * est_cov) seeds.push_back(std::make_pair(-kcov(u), u));
    std::sort(seeds.begin(), seeds.end());
    std::vector<char> visited(n, 0);
    for (size_t si = 0; si < seeds.size(); ++si) {
        const size_t u0 = seeds[si].second;
        if (visited[u0]) continue;
        std::vector<uint32_t> inter(U[u0].colours.begin(), read_end(u0));
        size_t max_card_inter = static_cast<size_t>(static_cast<double>(inter.size()) * min_color_sharing);
        std::set<size_t> seen, valid; seen.insert(u0);
        std::queue<size_t> q; q.push(u0);
        while (!q.empty()) {
            const size_t x = q.front(); q.pop();
            std::vector<std::pair<double, size_t> > nbs;
            for (int d = 0; d < 2; ++d) for (int b = 0; b < 4; ++b) { const int64_t w = adj[x].u[d][b]; if (w >= 0 && seen.insert(static_cast<size_t>(w)).second && !visited[w]) nbs.push_back(std::make_pair(-kcov(static_cast<size_t>(w)), static_cast<size_t>(w))); }
            std::sort(nbs.begin(), nbs.end());
            for (size_t j = 0; j < nbs.size(); ++j) {
                const size_t w = nbs[j].second;
                std::vector<uint32_t> li;
                std::set_intersection(inter.begin(), inter.end(), U[w].colours.begin(), read_end(w), std::back_inserter(li));
                if (static_cast<double>(li.size()) >= static_cast<double>(n_read(w)) * min_color_sharing && li.size() >= max_card_inter && !li.empty()) {
                    inter.swap(li);
                    max_card_inter = std::max(max_card_inter, static_cast<size_t>(static_cast<double>(n_read(w)) * min_color_sharing));
                    valid.insert(w); q.push(w);
                }
            }
        }
        if (!valid.empty()) {
            valid.insert(u0);
            for (std::set<size_t>::const_iterator it = valid.begin(); it != valid.end(); ++it) {
                global_ids[*it] = inter; visited[*it] = 1;
                std::set_difference(U[*it].colours.begin(), read_end(*it), inter.begin(), inter.end(), std::back_inserter(local_ids[*it]));
            }
        }
    }
    size_t ng = 0;
    for (size_t u = 0; u < n; ++u) { if (global_ids[u].empty()) local_ids[u].assign(U[u].colours.begin(), read_end(u)); else ++ng; }
    if (!s.cover_ids.empty()) for (size_t u = 0; u < n; ++u) local_ids[u].insert(local_ids[u].end(), s.cover_ids[u].begin(), s.cover_ids[u].end()); // (larger than every read id: the sets stay sorted)
    fprintf(stderr, "rtk_build_index: est. k-mer coverage %.2f, %zu unitigs carry a global colour set\n", est_cov, ng);
}

} // namespace rtk

#endif
