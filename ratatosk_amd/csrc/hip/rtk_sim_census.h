// Developer statistics of the simulator build (-DRTK_SIM; no reference routine): alignments by call site (RTK_SITE names the site of the calls
// that follow, RtkSite in rtk_region_types.h; rtk_site_note counts one) and the census of repeated alignments (rtk_pair_note;
// profiles/scripts/sim_pairs.py). Host only, with the standard library; a device build reduces this file to four empty macros.
#ifndef RTK_SIM_CENSUS_H
#define RTK_SIM_CENSUS_H

#include "rtk_region_types.h"

#ifdef RTK_SIM
#include <algorithm>
#include <atomic>
#include <string>
#include <vector>
// alignments by call site: RTK_SITE(id) names the site of the calls that follow
extern thread_local int rtk_sim_site;
extern std::atomic<unsigned long long> rtk_sim_site_stat[32][8]; // calls, 32-bit word-columns, sum m, sum n, stored sweeps, stored word-columns, bounded (k >= 0), m > 2048
#define RTK_SITE(id) (rtk_sim_site = (id))
static inline void rtk_site_note(uint32_t m, uint32_t n, int k, bool stored) {
    std::atomic<unsigned long long>* t = rtk_sim_site_stat[rtk_sim_site & 31];
    const unsigned long long cells = static_cast<unsigned long long>((m + 31) / 32) * n;
    // (rows 26, 27: the calls and columns of one site by target length)
    if ((rtk_sim_site & 31) == RTK_SITE_SCORE_REF_IN_PATH) { int b = 0; while (b < 7 && (256u << b) <= n) ++b; rtk_sim_site_stat[26][b] += 1; rtk_sim_site_stat[27][b] += n; }
    t[0] += 1; t[1] += cells; t[2] += m; t[3] += n; if (stored) { t[4] += 1; t[5] += cells; } if (k >= 0) t[6] += 1; if (m > 2048) t[7] += 1;
}
// Census of repeated alignments (profiles/scripts/sim_pairs.py; off until rtk_sim_pairs(1)): the strings of every alignment of the region in progress, and per site the
// calls and 32-bit word-columns [site][2 c], [site][2 c + 1] of class c: 0 all; the pair repeats an earlier one of the region 1 exactly, 2 transposed, 3 with a query
// that is a prefix of the other's on the same target, 4 with a query of the same length at Hamming distance 1 .. 8 on the same target (the first class that holds)
struct RtkSimPair { std::string q, t; };
extern thread_local std::vector<RtkSimPair> rtk_sim_pair_log;
extern std::atomic<int> rtk_sim_pairs_on;
extern std::atomic<unsigned long long> rtk_sim_pair_stat[32][10];
#define RTK_PAIR_REGION() (rtk_sim_pair_log.clear())
static inline void rtk_pair_note(const char* q, uint32_t m, const char* t, uint32_t n) {
    if (!rtk_sim_pairs_on.load(std::memory_order_relaxed)) return;
    RtkSimPair p; p.q.assign(q, m); p.t.assign(t, n);
    int cls = 5;
    for (const RtkSimPair& e : rtk_sim_pair_log) {
        int c = 5;
        if (e.q == p.q && e.t == p.t) c = 1;
        else if (e.q == p.t && e.t == p.q) c = 2;
        else if (e.t == p.t && e.q.size() != p.q.size()) { const size_t l = std::min(e.q.size(), p.q.size()); if (l > 0 && e.q.compare(0, l, p.q, 0, l) == 0) c = 3; }
        else if (e.t == p.t) { size_t d = 0; for (size_t i = 0; i < p.q.size() && d <= 8; ++i) d += e.q[i] != p.q[i]; if (d <= 8) c = 4; } // (d == 0 is class 1)
        cls = std::min(cls, c);
    }
    std::atomic<unsigned long long>* st = rtk_sim_pair_stat[rtk_sim_site & 31];
    const unsigned long long cells = static_cast<unsigned long long>((m + 31) / 32) * n;
    st[0] += 1; st[1] += cells; if (cls < 5) { st[2 * cls] += 1; st[2 * cls + 1] += cells; }
    rtk_sim_pair_log.push_back(std::move(p));
}
#else
#define RTK_SITE(id) ((void)0)
#define rtk_site_note(m, n, k, stored) ((void)0)
#define RTK_PAIR_REGION() ((void)0)
#define rtk_pair_note(q, m, t, n) ((void)0)
#endif

#endif
