// Sorted runs of distinct k-mer codes merged into one sorted array on several threads: the end of the device side's k-mer count (hip/rtk_index_count.h), whose hash
// partitions are sorted each. Host code only (tools/chunks_step.cpp runs it alone; tests/test_index_host_steps.py holds it to the sorted union).
#ifndef RTK_SORTED_RUNS_HPP
#define RTK_SORTED_RUNS_HPP

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

namespace rtk {

// solid[run_start[r] .. run_start[r + 1]) is run r (the last one ends with `solid`): ascending 2k-bit codes, KM = uint64_t (k <= 31) or unsigned __int128 (k <= 63).
// out has room for solid.size() keys. Merged by ranges of the key space, one range per thread: every thread finds its stretch of every run by bisection, and the
// stretches of the ranges before it give it its place in the output.
template <class KM>
void merge_sorted_runs(const std::vector<KM>& solid, std::vector<size_t> run_start, int k, int n_threads, KM* out) {
    if (run_start.size() <= 1) { if (!solid.empty()) memcpy(out, solid.data(), sizeof(KM) * solid.size()); return; }
    const size_t P = run_start.size(); run_start.push_back(solid.size());
    const int T = n_threads < 1 ? 1 : (n_threads > 256 ? 256 : n_threads);
    std::vector<std::vector<size_t> > cut(static_cast<size_t>(T) + 1, std::vector<size_t>(P));
    const unsigned __int128 span = static_cast<unsigned __int128>(1) << (2 * k);
    for (int t = 0; t <= T; ++t) for (size_t r = 0; r < P; ++r) {
        if (t == T) { cut[t][r] = run_start[r + 1]; continue; }
        const KM v = sizeof(KM) == 8 ? static_cast<KM>(span * static_cast<unsigned __int128>(t) / static_cast<unsigned __int128>(T)) : static_cast<KM>(span / static_cast<unsigned __int128>(T) * static_cast<unsigned __int128>(t)); // (2^126 * t would not fit)
        cut[t][r] = static_cast<size_t>(std::lower_bound(solid.begin() + static_cast<std::ptrdiff_t>(run_start[r]), solid.begin() + static_cast<std::ptrdiff_t>(run_start[r + 1]), v) - solid.begin());
    }
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back([&, t]() {
        size_t at = 0; for (size_t r = 0; r < P; ++r) at += cut[t][r] - run_start[r];
        std::vector<size_t> head(cut[t]); const std::vector<size_t>& end = cut[t + 1];
        for (;;) { size_t best = P; KM bv = 0; for (size_t r = 0; r < P; ++r) if (head[r] < end[r] && (best == P || solid[head[r]] < bv)) { best = r; bv = solid[head[r]]; } if (best == P) break; out[at++] = bv; ++head[best]; }
    });
    for (size_t t = 0; t < th.size(); ++t) th[t].join();
}

} // namespace rtk

#endif
