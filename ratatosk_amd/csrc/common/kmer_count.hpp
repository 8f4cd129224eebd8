// Host-side count of the canonical one-word k-mers (odd k <= 31) of FASTA/FASTQ files: the k-mers seen at least `min_count` times, sorted ascending.
// What rtk_index_count_kmers (csrc/hip/rtk_index.hip) computes on the device, for the tools' plain paths (no GPU, no library). The k-mer space is cut
// into one shard per thread by a hash; every thread reads the input itself, collects the k-mers of its shard, sorts them and keeps the first of every
// run of >= min_count equal ones.
#ifndef RTK_COMMON_KMER_COUNT_HPP
#define RTK_COMMON_KMER_COUNT_HPP

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "fastx.hpp"
#include "kmer.hpp"

namespace rtk {

inline bool count_kmers_host(const std::vector<std::string>& files, int k, unsigned min_count, unsigned n_thr, std::vector<uint64_t>& solid, std::string* err) {
    if (n_thr < 1) n_thr = 1;
    if (min_count < 1) min_count = 1;
    const uint64_t mask = kmer_mask(k);
    std::vector<std::vector<uint64_t> > part(n_thr);
    std::vector<std::string> bad(n_thr);
    auto count_shard = [&](unsigned t) {
        std::vector<uint64_t> all;
        std::string name, seq, qual;
        for (size_t f = 0; f < files.size(); ++f) {
            FastxReader fr;
            if (!fr.open(files[f])) { bad[t] = "cannot open " + files[f]; return; }
            while (fr.next(name, seq, qual)) {
                uint64_t fw = 0; int valid = 0;
                for (size_t i = 0; i < seq.size(); ++i) {
                    const int b = base2bits(seq[i]);
                    if (b < 0) { valid = 0; fw = 0; continue; }
                    fw = ((fw << 2) | static_cast<uint64_t>(b)) & mask;
                    if (++valid >= k) { const uint64_t c = kmer_canonical(fw, k); if ((hash_km(c) >> 40) % n_thr == t) all.push_back(c); }
                }
            }
            if (fr.failed()) { bad[t] = files[f] + " ends in a damaged or cut-short gzip stream"; return; }
        }
        std::sort(all.begin(), all.end());
        for (size_t i = 0; i < all.size();) { size_t j = i; while (j < all.size() && all[j] == all[i]) ++j; if (j - i >= min_count) part[t].push_back(all[i]); i = j; }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n_thr; ++t) th.emplace_back(count_shard, t);
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
    for (unsigned t = 0; t < n_thr; ++t) if (!bad[t].empty()) { if (err) *err = bad[t]; return false; }
    solid.clear();
    for (unsigned t = 0; t < n_thr; ++t) { solid.insert(solid.end(), part[t].begin(), part[t].end()); std::vector<uint64_t>().swap(part[t]); }
    std::sort(solid.begin(), solid.end());
    return true;
}

} // namespace rtk

#endif
