// Host-side count of the canonical k-mers (odd k <= 63; KM: uint64_t up to k = 31, u128 above) of FASTA/FASTQ files: the k-mers seen at least `min_count`
// times, sorted ascending. What rtk_index_count_kmers (csrc/hip/rtk_index_count.h) computes on the device, for the tools' plain paths (no GPU, no library).
// The k-mer space is cut into one shard per thread by a hash; every thread reads the input itself (parsing is cheap next to the rest), collects the
// k-mers of its shard, sorts them and keeps the first of every run of >= min_count equal ones.
#ifndef RTK_COMMON_KMER_COUNT_HPP
#define RTK_COMMON_KMER_COUNT_HPP

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "fastx.hpp"
#include "kmer.hpp"

namespace rtk {

// 0, or with *bad_file set: 1 = that file does not open, 2 = it ends in a damaged or cut-short gzip stream (which is not the end of the reads)
template <class KM> inline int count_kmers_host(const std::vector<std::string>& files, int k, unsigned min_count, unsigned n_thr, std::vector<KM>& solid, size_t* bad_file) {
    if (n_thr < 1) n_thr = 1;
    const KM mask = km_mask<KM>(k);
    std::vector<std::vector<KM> > part(n_thr);
    std::vector<int> bad(n_thr, 0); std::vector<size_t> bad_f(n_thr, 0);
    auto count_shard = [&](unsigned t) {
        std::string name, seq, qual;
        std::vector<KM> all;
        for (size_t f = 0; f < files.size(); ++f) {
            FastxReader fr;
            if (!fr.open(files[f])) { bad[t] = 1; bad_f[t] = f; return; }
            while (fr.next(name, seq, qual)) for_each_canonical_kmer<KM>(seq.data(), seq.size(), k, mask, [&](KM c, size_t) { if ((hash_km(c) >> 40) % n_thr == t) all.push_back(c); });
            if (fr.failed()) { bad[t] = 2; bad_f[t] = f; return; }
        }
        std::sort(all.begin(), all.end());
        for (size_t i = 0; i < all.size();) { size_t j = i; while (j < all.size() && all[j] == all[i]) ++j; if (j - i >= min_count) part[t].push_back(all[i]); i = j; }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(count_shard, t);
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
    for (unsigned t = 0; t < n_thr; ++t) if (bad[t]) { if (bad_file) *bad_file = bad_f[t]; return bad[t]; }
    solid.clear();
    for (unsigned t = 0; t < n_thr; ++t) { solid.insert(solid.end(), part[t].begin(), part[t].end()); std::vector<KM>().swap(part[t]); }
    std::sort(solid.begin(), solid.end());
    return 0;
}

} // namespace rtk

#endif
