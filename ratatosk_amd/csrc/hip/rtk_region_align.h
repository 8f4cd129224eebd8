// Region stage, the alignment calls of the region program: edlibAlign as the `correct` lambda and the path search call it (reference:
// src/Alignment.cpp, src/GraphTraversal.cpp:867-909), counted and timed, and the forward trim of src/Correction.cpp:727-747 read off a
// stored NW sweep that the consensus resumes (rtk_trim_by_column, rtk_park_walk).
#ifndef RTK_REGION_ALIGN_H
#define RTK_REGION_ALIGN_H

#include "rtk_region_paths.h"
#include "rtk_sim_census.h"

#ifdef RTK_SIM
#include <assert.h>
#endif

RTK_FN_HOT MyersResult rtk_align(const RCtx& c, const char* q_, uint32_t m_, const char* t_, uint32_t n_, int kk_, int mode_, bool iupac_ = true) {
    RegionScratch& s = *rtk_u(c.sc); const char* q = rtk_u(q_); const char* t = rtk_u(t_);
    const uint32_t m = rtk_u(m_), n = rtk_u(n_); const int kk = rtk_u(kk_), mode = rtk_u(mode_); const bool iupac = rtk_u(iupac_);
    s.cnt[RTK_RC_ALIGN] += 1; s.cnt[RTK_RC_CELLS] += static_cast<unsigned long long>((m + 63) / 64) * n;
    const unsigned long long t0 = rtk_clock();
    rtk_site_note(m, n, kk, false); rtk_pair_note(q, m, t, n);
    const MyersResult r = rtk_myers_distance(s.my, q, static_cast<int>(m), t, static_cast<int>(n), kk, mode, iupac);
    s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t0;
    return r;
}

// alignment with its moves (left in s.my.moves); counted like the distance call + path call pair it replaces
RTK_FN_HOT MyersResult rtk_align_path(const RCtx& c_, const char* q_, uint32_t m_, const char* t_, uint32_t n_, int mode_, uint32_t* n_moves_) {
    const RCtx& c = *rtk_u(&c_); RegionScratch& s = rtk_hdr(c); const char* q = rtk_u(q_); const char* t = rtk_u(t_);
    const uint32_t m = rtk_u(m_), n = rtk_u(n_); const int mode = rtk_u(mode_); uint32_t* n_moves = rtk_u(n_moves_);
    s.cnt[RTK_RC_ALIGN] += (m > 0 && n > 0) ? 2 : 1; s.cnt[RTK_RC_CELLS] += static_cast<unsigned long long>((m + 63) / 64) * n;
    const unsigned long long t0 = rtk_clock();
    rtk_site_note(m, n, -1, true); rtk_pair_note(q, m, t, n);
    const MyersResult r = rtk_myers_path(s.my, q, static_cast<int>(m), t, static_cast<int>(n), mode, true, n_moves);
    s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t0;
    return r;
}

// The walk of a pending park (TrimPark, rtk_trim_by_column below) and its copy to rbuf[RTK_RB_PARK_MOVES]; no park pending: nothing. Between the trim and this call nothing may write the Myers table: the trim is
// the last alignment of rtk_correct_region, and rtk_region_program calls this at its decision about the second strand, with rtk_strand2_skippable -- which
// aligns nothing -- in between. (s.my.moves is written here and copied at once, so what it held does not matter.)
// A trim that kept only the last column of its sweep (pending == RTK_PARK_NO_TABLE) has no table to walk: the sweep of (corr[0, len), raw) is run again here, stored
// this time -- rows up to len of the trim's own sweep, so the walk is the same. The few regions that come here pay a second sweep (rtk_stats::n_park_resweeps; not
// an alignment of n_align / n_align_cells: the reference makes none); the many that do not have stored no table. corr, raw: the strings of the trim.
RTK_FN void rtk_park_walk(const RCtx& c_, const char* corr_, const char* raw_) {
    const RCtx& c = *rtk_u(&c_); RegionScratch& s = rtk_hdr(c); const char* corr = rtk_u(corr_); const char* raw = rtk_u(raw_);
    TrimPark& pk = s.loc.park;
    if (!pk.pending) return;
    const unsigned long long t1 = rtk_clock();
    if (pk.pending == RTK_PARK_NO_TABLE) {
        const bool ok = rtk_myers_shw_by_column(s.my, corr, static_cast<int>(pk.len), raw, static_cast<int>(pk.n), true, 1, 0, nullptr, nullptr);
        s.cnt[RTK_RC_PARK_RESWEEPS] += 1;
        if (!ok) { pk.pending = 0; pk.nm = 0; s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t1; return; } // (cannot happen: the trim's sweep of a longer string passed the same tests) nothing parked, the consensus sweeps the pair itself
        pk.gen = rtk_ld(&s.my.tb_gen);
    }
#ifdef RTK_SIM
    assert(pk.gen == s.my.tb_gen); // the table still holds the sweep of the trim
#endif
    pk.pending = 0;
    uint32_t& nm = pk.nm; nm = 0;
    rtk_myers_walk(s.my, static_cast<int>(pk.len), static_cast<int>(pk.n), static_cast<int>(pk.n), pk.dist, &nm);
    if (nm <= s.str_cap) rtk_wcopy(s.rbuf[RTK_RB_PARK_MOVES], s.my.moves, nm);
    else nm = 0;
    s.cnt[RTK_RC_PARK_WALKED] += 1; s.cnt[RTK_RC_PARK_DEFERRED] -= 1;
    s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t1;
}

// The trim of rtk_correct_region, edlibAlign(raw, corr, SHW), read off the last column of ONE NW sweep of (corr, raw) (rtk_myers_shw_by_column): a plain
// NW step instead of the distance call's step with last-row tracking.
// park: the same sweep also holds the consensus's forward alignment, the NW path of the trimmed string corr[0, keep) against this raw region
// (rtk_generate_consensus): its moves can be walked from row keep (D[keep][|raw|] is the minimum the trim found) and parked in rbuf[RTK_RB_PARK_MOVES], which
// otherwise only the consensus writes (as RTK_RB_CONS_QUAL), after it has read them (hand-over H2, rtk_region_types.h). Most gap regions never run a consensus
// (rtk_strand2_skippable), and the rule that decides so asks three things of the park: that it exists, its distance and its LAST move. All three are in the
// last column of the sweep. So the sweep of a park stores no table: it keeps the delta vectors of that column (store 2 of rtk_myers_shw_by_column), the trim
// notes the three things (rtk_myers_last_move_column) and leaves the park pending. Where the region does go on to its second strand, rtk_region_program calls
// rtk_park_walk, which sweeps corr[0, keep) against the raw region again, stored this time, walks the path and copies the moves. RTK_TRIM_STORE=1 stores the
// table at the trim and walks that. RTK_PARK_EAGER=1 (tests, A/B runs) walks right here; so does a pair whose moves might not fit the string buffers (the walk
// then clears the park; the consensus sweeps the pair itself and reports the overflow).
// false: the route does not apply (no result, no alignment counted) and the caller makes the distance call.
RTK_FN bool rtk_trim_by_column(const RCtx& c_, const char* raw_, uint32_t n_, const char* corr_, uint32_t m_, bool park_, MyersResult* out_) {
    const RCtx& c = *rtk_u(&c_); RegionScratch& s = rtk_hdr(c); const char* raw = rtk_u(raw_); const char* corr = rtk_u(corr_);
    const uint32_t n = rtk_u(n_), m = rtk_u(m_); const bool park = rtk_u(park_); MyersResult* out = rtk_u(out_);
    const unsigned long long t0 = rtk_clock();
    // park: the sweep keeps its last column (store 2), which holds what the rule of the skip asks; RTK_TRIM_STORE=1 (rtk_knobs.h): the whole table (store 1), as before
    const bool table = rtk_u(c.o.trim_store) != 0u;
    const bool ok = rtk_myers_shw_by_column(s.my, corr, static_cast<int>(m), raw, static_cast<int>(n), true, park ? (table ? 1 : 2) : 0, 0, out, nullptr);
    s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t0;
    if (!ok) return false;
    s.cnt[RTK_RC_ALIGN] += 1; s.cnt[RTK_RC_CELLS] += static_cast<unsigned long long>((m + 63) / 64) * n;
    RTK_SITE(park ? RTK_SITE_TRIM_STORED : RTK_SITE_TRIM_COLUMN); rtk_site_note(m, n, -1, park); rtk_pair_note(corr, m, raw, n);
    s.cnt[park ? RTK_RC_TRIM_STORED : RTK_RC_TRIM_COLUMN] += 1;
    if (!park) return true;
    s.cnt[RTK_RC_PARK_DEFERRED] += 1; // a stored sweep that nothing has walked (yet: rtk_park_walk takes it back)
    // the conditions of rtk_myers_path's in-memory route for (corr[0, keep), raw) that the stored sweep of all of corr has not checked already
    const uint32_t keep = (out->first == -1) ? 0u : static_cast<uint32_t>(out->last + 1);
    if (keep == 0 || keep > s.my.r_cap || keep + n > s.my.mv_cap || !rtk_tb_in_memory(static_cast<int>(keep), n)) return true;
    const unsigned long long t1 = rtk_clock();
    TrimPark& pk = s.loc.park;
    pk.nm = 0; pk.len = keep; pk.dist = out->dist; pk.n = n; pk.gen = rtk_ld(&s.my.tb_gen); pk.pending = table ? RTK_PARK_TABLE : RTK_PARK_NO_TABLE;
    pk.last_move = table ? rtk_myers_last_move(s.my, static_cast<int>(keep), static_cast<int>(n), static_cast<int>(n), out->dist) : rtk_myers_last_move_column(s.my, static_cast<int>(keep));
    s.cnt[RTK_RC_CYC_MYERS] += rtk_clock() - t1;
    if (rtk_u(c.o.park_eager) || keep + n > s.str_cap) rtk_park_walk(c, corr, raw);
    return true;
}

#endif
