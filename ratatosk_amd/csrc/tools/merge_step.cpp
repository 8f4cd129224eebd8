// rtk_merge_step: the merging step of rtk_build_index (tools/index/merge.hpp) on events given by hand -- for tests of the rule on crafted events that no set of
// reads would give (ids up to 2^32 - 1, ids without events, classes of chosen shape). Host code only.
//   rtk_merge_step THREADS events.bin merged.bin
// events.bin: 64-bit words unitig << 32 | id in the machine's byte order, ascending and distinct. merged.bin: the merged events in the same form.
// stderr: the step's line.
#include <fstream>

#include "index/merge.hpp"

using namespace rtk;

int main(int argc, char** argv) {
    if (argc != 4 || atoi(argv[1]) < 1) { fprintf(stderr, "usage: rtk_merge_step THREADS(>= 1) events.bin merged.bin (64-bit words unitig << 32 | id, ascending and distinct)\n"); return 2; }
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) { fprintf(stderr, "rtk_merge_step: cannot open %s\n", argv[2]); return 1; }
    std::vector<uint64_t> ev; uint64_t w = 0;
    while (in.read(reinterpret_cast<char*>(&w), 8)) ev.push_back(w);
    if (in.gcount() != 0) { fprintf(stderr, "rtk_merge_step: %s is no whole number of 64-bit words\n", argv[2]); return 2; }
    for (size_t i = 1; i < ev.size(); ++i) if (ev[i] <= ev[i - 1]) { fprintf(stderr, "rtk_merge_step: the events are not ascending and distinct\n"); return 2; }
    std::vector<Unitig> U(ev.empty() ? 0 : static_cast<size_t>(ev.back() >> 32) + 1);
    for (size_t i = 0; i < ev.size(); ++i) U[static_cast<size_t>(ev[i] >> 32)].colours.push_back(static_cast<uint32_t>(ev[i]));
    MergeCounts c; merge_host(U, static_cast<unsigned>(atoi(argv[1])), c);
    merge_line(c);
    std::ofstream out(argv[3], std::ios::binary);
    for (size_t u = 0; u < U.size(); ++u) for (size_t i = 0; i < U[u].colours.size(); ++i) { w = (static_cast<uint64_t>(u) << 32) | U[u].colours[i]; out.write(reinterpret_cast<const char*>(&w), 8); }
    out.close();
    if (!out.good()) { fprintf(stderr, "rtk_merge_step: cannot write %s\n", argv[3]); return 1; }
    return 0;
}
