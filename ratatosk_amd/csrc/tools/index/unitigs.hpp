// rtk_build_index: the k-mer table and the unitigs (maximal non-branching paths over the solid canonical k-mers). The plain construction is the
// definition and the fallback; --fast / --gpu must produce what it produces, byte for byte (one- and two-word k-mers).
#ifndef RTK_TOOLS_INDEX_UNITIGS_HPP
#define RTK_TOOLS_INDEX_UNITIGS_HPP

#include <set>

#include "state.hpp"

namespace rtk {

struct DeviceUnitigs { char* pool = nullptr; uint64_t* off = nullptr; uint64_t* seeds = nullptr; uint64_t n = 0; uint64_t* left = nullptr; uint64_t n_left = 0; }; // what rtk_index_unitigs returns (--gpu; two-word k-mers: two words each)

// every solid k-mer into the table with value 0, on all threads (the table does not grow here). The solid k-mers are distinct and the top word of a 2k-bit
// code (k <= 63) is never all ones, so a slot is claimed with a 64-bit compare-and-swap on the top word of its key; the low word of a two-word k-mer is
// written by the thread that owns the slot (nothing reads the table before the threads join)
template <class KM> static void fast_table_fill(KTable<KM>& km, const std::vector<KM>& solid, unsigned n_thr) {
    const uint64_t EMPTY = ~0ULL; const size_t W = sizeof(KM) / 8, mask = km.mask;
    uint64_t* words = reinterpret_cast<uint64_t*>(km.keys.data()); // slot s: words[W s] the low word, words[W s + W - 1] the top word
    parallel_for(solid.size(), n_thr, [&](size_t b, size_t e, unsigned) {
        for (size_t i = b; i < e; ++i) {
            const KM key = solid[i]; const uint64_t top = static_cast<uint64_t>(key >> (64 * (W - 1))); size_t s = hash_km(key) & mask;
            while (true) {
                uint64_t exp = EMPTY;
                if (__atomic_compare_exchange_n(&words[W * s + W - 1], &exp, top, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { if (W > 1) __atomic_store_n(&words[W * s], static_cast<uint64_t>(key), __ATOMIC_RELAXED); break; }
                s = (s + 1) & mask;
            }
        }
    });
    km.n = solid.size();
}

template <class KM> static void fill_table(IndexBuild<KM>& s) {
    size_t cap = 16; while (cap * 6 < s.solid.size() * 10 + 16) cap <<= 1; if (s.solid.size() < (1ull << 30)) cap <<= 1; // (load <= 0.6; below 2^30 k-mers half of that: a 3 Gb genome's table is 137 GB instead of 275)
    s.km.reset(cap);
    if (s.o.fast) fast_table_fill(s.km, s.solid, s.n_thr);
    else for (size_t i = 0; i < s.solid.size(); ++i) *s.km.slot(s.solid[i], true) = 0;
    fprintf(stderr, "rtk_build_index: %zu solid %d-mers\n", s.solid.size(), s.k);
}

// The plain construction: a unitig starts at the first free k-mer of `seeds` (sorted), in its canonical orientation, and follows the mutually unique
// links both ways until it meets one of its own k-mers (cycle / hairpin guard) or a k-mer that is taken. f(seed, path of oriented k-mers) per unitig.
template <class KM, class Taken, class F> static void plain_walks(IndexBuild<KM>& s, const std::vector<KM>& seeds, Taken taken, F f) {
    const int k = s.k;
    std::set<KM> in_this; // canonical k-mers of the unitig being built
    for (size_t si = 0; si < seeds.size(); ++si) {
        const KM seed = seeds[si];
        if (taken(seed)) continue;
        in_this.clear(); in_this.insert(seed);
        std::vector<KM> fwd(1, seed), bwd; KM nb[4], nb2[4]; // oriented k-mers
        for (KM x = seed;;) { if (s.succs(x, nb) != 1) break; const KM y = nb[0]; if (s.preds(y, nb2) != 1) break; const KM cy = kmer_canonical(y, k); if (in_this.count(cy) || taken(cy)) break; in_this.insert(cy); fwd.push_back(y); x = y; } // extend forward
        for (KM x = seed;;) { if (s.preds(x, nb) != 1) break; const KM y = nb[0]; if (s.succs(y, nb2) != 1) break; const KM cy = kmer_canonical(y, k); if (in_this.count(cy) || taken(cy)) break; in_this.insert(cy); bwd.push_back(y); x = y; } // extend backward
        std::vector<KM> path(bwd.rbegin(), bwd.rend()); path.insert(path.end(), fwd.begin(), fwd.end());
        f(seed, path);
    }
}
template <class KM> static std::string path_text(const std::vector<KM>& path, int k) {
    std::string seq = km_decode<KM>(path[0], k);
    for (size_t j = 1; j < path.size(); ++j) seq.push_back(bits2base(static_cast<int>(path[j] & 3)));
    return seq;
}
template <class KM> static void plain_unitigs(IndexBuild<KM>& s) {
    s.U.clear();
    plain_walks(s, s.solid, [&](KM c) { return *s.km.slot(c, false) != 0; }, [&](KM, const std::vector<KM>& path) {
        Unitig u; u.seq = path_text(path, s.k);
        const uint64_t uid = s.U.size();
        for (size_t i = 0; i < path.size(); ++i) {
            bool is_fw; const KM c = kmer_canonical(path[i], s.k, &is_fw);
            *s.km.slot(c, false) = ((uid + 1) << 32) | (static_cast<uint64_t>(i) << 1) | (is_fw ? 1ULL : 0ULL);
        }
        s.U.push_back(u);
    });
}

// Unitigs by walking every maximal chain of mutually unique links from its ends, on all threads. The plain construction starts a unitig at the
// first unvisited k-mer in sorted order, in its canonical orientation, and follows the links both ways: for a chain that never meets one of its
// own k-mers again that is the chain oriented so that its smallest canonical k-mer reads forwards, and the unitigs are numbered by those
// smallest k-mers. Chains that do meet themselves (closed loops, hairpins through a reverse complement) are left to the plain code, which
// then only sees their k-mers; all unitigs are put in the order of their first k-mers at the end. Returns false (nothing kept) if a k-mer
// ended up on two unitigs -- the caller then runs the plain construction.
template <class KM> static bool fast_unitigs(IndexBuild<KM>& s, const DeviceUnitigs* dev) {
    struct Rec { KM seed; std::string seq; };
    KTable<KM>& km = s.km; const std::vector<KM>& solid = s.solid; const int k = s.k; const unsigned n_thr = s.n_thr;
    std::vector<std::vector<Rec> > out(n_thr);
    auto next = [&](KM x, KM* y) -> bool { KM nb[4], nb2[4]; if (s.succs(x, nb) != 1) return false; if (s.preds(nb[0], nb2) != 1) return false; *y = nb[0]; return true; }; // the link the plain code follows forwards
    auto prev = [&](KM x, KM* y) -> bool { KM nb[4], nb2[4]; if (s.preds(x, nb) != 1) return false; if (s.succs(nb[0], nb2) != 1) return false; *y = nb[0]; return true; };
    std::atomic<bool> clash(false);
    auto claim = [&](KM canonical) { uint64_t* v = km.slot(canonical, false); if (__atomic_exchange_n(v, 1ULL, __ATOMIC_RELAXED) != 0) clash = true; };
    if (!dev) parallel_for(solid.size(), n_thr, [&](size_t b, size_t e, unsigned t) {
        std::vector<KM> path;
        for (size_t i = b; i < e && !clash; ++i) {
            const KM s0 = solid[i]; KM y;
            const bool has_fw = next(s0, &y), has_bw = prev(s0, &y);
            if (has_fw && has_bw) continue; // inside a chain (or on a closed loop)
            // walk inwards from this end: forwards from s0 if nothing links into it from behind, else forwards from its reverse complement
            KM x = has_bw ? kmer_revcomp(s0, k) : s0;
            path.clear(); path.push_back(x);
            while (next(x, &y)) { path.push_back(y); x = y; if (path.size() > solid.size()) break; }
            const KM end_c = kmer_canonical(path.back(), k);
            if (path.size() > 1 && end_c == s0) continue;        // the chain comes back to its own first k-mer (hairpin): plain code
            if (end_c < s0) continue;                             // the other end owns the chain
            if (path.size() > solid.size()) continue;
            // orient: the smallest canonical k-mer of the chain reads forwards
            size_t m = 0; KM mc = kmer_canonical(path[0], k);
            for (size_t j = 1; j < path.size(); ++j) { const KM c = kmer_canonical(path[j], k); if (c < mc) { mc = c; m = j; } }
            // (a chain that holds a k-mer and its reverse complement without coming back to its first k-mer cannot exist (the links are symmetric); checked by the claims below)
            if (path[m] != mc) { std::reverse(path.begin(), path.end()); for (size_t j = 0; j < path.size(); ++j) path[j] = kmer_revcomp(path[j], k); }
            Rec r; r.seed = mc; r.seq = path_text(path, k);
            for (size_t j = 0; j < path.size(); ++j) claim(kmer_canonical(path[j], k));
            out[t].push_back(r);
        }
    });
    if (clash) return false;
    // what is left belongs to chains that meet themselves: the plain construction, which finds every other k-mer taken
    std::vector<Rec> rest;
    {
        // (the k-mers no chain has claimed are looked for on all threads -- one table probe per solid k-mer, a cache miss each -- and come out in
        // sorted order, thread after thread; the plain construction then only visits those)
        std::vector<KM> left;
        if (dev) { const KM* dl = reinterpret_cast<const KM*>(dev->left); left.assign(dl, dl + dev->n_left); } // (--gpu: the chains were walked, written and claimed on the device)
        else {
            std::vector<std::vector<KM> > left_t(n_thr);
            parallel_for(solid.size(), n_thr, [&](size_t b, size_t e, unsigned t) { for (size_t i = b; i < e; ++i) if (*km.slot(solid[i], false) == 0) left_t[t].push_back(solid[i]); });
            for (unsigned t = 0; t < n_thr; ++t) left.insert(left.end(), left_t[t].begin(), left_t[t].end());
        }
        size_t lcap = 16; while (lcap * 6 < left.size() * 10 + 16) lcap <<= 1; lcap <<= 1;
        KTable<KM> lt(lcap); // the left-over k-mers: 0 = free, 1 = on a unitig built below; a k-mer that is not in it lies on a chain built above
        for (size_t li = 0; li < left.size(); ++li) *lt.slot(left[li], true) = 0;
        plain_walks(s, left, [&](KM c) -> bool { const uint64_t* v = lt.slot(c, false); return !v || *v != 0; }, [&](KM seed, const std::vector<KM>& path) {
            Rec r; r.seed = seed; r.seq = path_text(path, k);
            for (size_t j = 0; j < path.size(); ++j) *lt.slot(kmer_canonical(path[j], k), false) = 1;
            rest.push_back(r);
        });
    }
    if (s.knobs.trace) fprintf(stderr, "rtk_build_index: %zu unitigs of chains that meet themselves built by the plain code\n", rest.size());
    // all unitigs in the order of their first k-mers; the table values from the final numbers
    std::vector<Rec*> all;
    std::vector<Rec> dev_recs;
    if (dev) { // (already in the order of their seeds; the sequences are cut out of the pool where the table values are set, below)
        dev_recs.resize(dev->n);
        parallel_for(dev_recs.size(), n_thr, [&](size_t b, size_t e, unsigned) { for (size_t i = b; i < e; ++i) { dev_recs[i].seed = reinterpret_cast<const KM*>(dev->seeds)[i]; dev_recs[i].seq.assign(dev->pool + dev->off[i], dev->pool + dev->off[i + 1]); } });
        for (size_t i = 0; i < dev_recs.size(); ++i) all.push_back(&dev_recs[i]);
    }
    for (unsigned t = 0; t < n_thr; ++t) for (size_t i = 0; i < out[t].size(); ++i) all.push_back(&out[t][i]);
    for (size_t i = 0; i < rest.size(); ++i) all.push_back(&rest[i]);
    std::sort(all.begin(), all.end(), [](const Rec* a, const Rec* b) { return a->seed < b->seed; });
    s.U.resize(all.size());
    parallel_for(all.size(), n_thr, [&](size_t b, size_t e, unsigned) {
        for (size_t uid = b; uid < e; ++uid) {
            s.U[uid].seq.swap(all[uid]->seq);
            const std::string& q = s.U[uid].seq; KM fw = 0;
            for (size_t i = 0; i < q.size(); ++i) {
                fw = ((fw << 2) | static_cast<KM>(base2bits(q[i]))) & s.mask;
                if (i + 1 < static_cast<size_t>(k)) continue;
                bool is_fw; const KM c = kmer_canonical(fw, k, &is_fw);
                *km.slot(c, false) = ((static_cast<uint64_t>(uid) + 1) << 32) | (static_cast<uint64_t>(i + 1 - k) << 1) | (is_fw ? 1ULL : 0ULL);
            }
        }
    });
    return true;
}

// device chains (--gpu), then fast_unitigs (--fast), then the plain construction as the fallback
template <class KM> static void build_unitigs(IndexBuild<KM>& s) {
    bool fast_done = false, have_dev = false;
    DeviceUnitigs dev;
    HipLib::unitigs_fn fn = nullptr;
    if (s.o.gpu && s.lib.get(fn, "rtk_index_unitigs") && !s.knobs.host_unitigs) { // the chains walked and written on the device (csrc/hip/rtk_index_unitigs.h rtk_index_unitigs)
        have_dev = fn(0, s.k, reinterpret_cast<const uint64_t*>(s.solid.data()), s.solid.size(), &dev.pool, &dev.off, &dev.seeds, &dev.n, &dev.left, &dev.n_left) == 0;
        if (!have_dev) fprintf(stderr, "rtk_build_index: --gpu: unitigs on the host threads (%s)\n", s.lib.last_error ? s.lib.last_error() : "?");
    }
    if (s.o.fast) fast_done = fast_unitigs(s, have_dev ? &dev : nullptr);
    if (s.lib.free) { s.lib.free(dev.pool); s.lib.free(dev.off); s.lib.free(dev.seeds); s.lib.free(dev.left); }
    if (!fast_done) {
        if (s.o.fast) for (size_t i = 0; i < s.km.vals.size(); ++i) s.km.vals[i] = 0; // (the thread-parallel construction backed out: every k-mer unvisited again)
        plain_unitigs(s);
    }
    fprintf(stderr, "rtk_build_index: %zu unitigs\n", s.U.size());
}

} // namespace rtk

#endif
