// rtk_subsample_step: the colour subsampling step of rtk_build_index (tools/index/subsample.hpp) on unitigs given by hand -- for tests of the rule on crafted
// graphs that no set of reads would give (fewer than twenty unitigs, all at one coverage, a unitig with exactly min_cov_vertices colours). Host code only.
//   rtk_subsample_step K SEED FAST < unitigs.txt      one line per unitig: SEQUENCE COVERAGE [id ...] (ids ascending)
// The sequences are the unitigs of a compacted graph (neighbours overlap by K - 1 bases); their k-mers go into the table, the structural half of the adjacency
// runs as in the tool, then the step. stdout: one line per unitig with its colours afterwards; stderr: the step's line.
#include <iostream>
#include <sstream>

#include "index/annotate.hpp"
#include "index/subsample.hpp"

using namespace rtk;

template <class KM> static int run(const IndexOptions& o) {
    IndexBuild<KM> s(o);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line); Unitig u; uint32_t id;
        if (!(is >> u.seq >> u.cov)) continue;
        while (is >> id) u.colours.push_back(id);
        if (u.seq.size() < static_cast<size_t>(s.k)) { fprintf(stderr, "rtk_subsample_step: a unitig shorter than k\n"); return 2; }
        s.U.push_back(u);
    }
    for (size_t u = 0; u < s.U.size(); ++u)
        for_each_canonical_kmer<KM>(s.U[u].seq.data(), s.U[u].seq.size(), s.k, s.mask, [&](KM km, size_t p) { *s.km.slot(km, true) = (static_cast<uint64_t>(u + 1) << 32) | (static_cast<uint64_t>(p) << 1); });
    adjacency_structure(s);
    if (!subsample_colours(s)) return 1;
    for (size_t u = 0; u < s.U.size(); ++u) { printf("%zu:", u); for (size_t i = 0; i < s.U[u].colours.size(); ++i) printf(" %u", s.U[u].colours[i]); printf("\n"); }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: rtk_subsample_step K SEED FAST(0|1) < unitigs.txt (SEQUENCE COVERAGE [id ...] per line)\n"); return 2; }
    IndexOptions o; o.k = atoi(argv[1]); o.subsample = true; o.subsample_seed = strtoull(argv[2], nullptr, 10); o.fast = atoi(argv[3]) != 0;
    if (o.k < 3 || o.k > RTK_MAX_K || !(o.k & 1)) { fprintf(stderr, "rtk_subsample_step: odd k <= 63\n"); return 2; }
    return o.k <= 31 ? run<uint64_t>(o) : run<u128>(o);
}
