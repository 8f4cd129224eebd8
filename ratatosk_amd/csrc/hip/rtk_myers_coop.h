// One pass, or one round of passes, gangs or leaf tracebacks, on the waves of a workgroup (RTK_MULTIWAVE: rtk_phase_long.hip). The protocol of the mailbox RtkCoop (LDS):
//   seq         written by the program wave (wave 0) only, +1 per round, AFTER the jobs, first[], n_items, the zeroed progress[], n_done = 0 and next_item = 0, behind a
//               workgroup release fence; a helper that sees seq move takes an acquire fence and then reads the mailbox (the kernel zeroes seq; exit_flag ends the helpers).
//   next_item   fetch-added by every wave, relaxed: who takes which item. Items are claimed in ascending order, and a row block only waits for the block above it in
//               its own pass, a lower item that somebody holds: the lowest unfinished item can always run.
//   progress[i] written by the ONE wave that holds row block i: columns whose bottom-row delta is in `carry` (global memory), each store behind a release fence; read
//               by the wave that holds block i + 1, which takes an acquire fence before it reads those carries (rtk_myers_block).
//   n_done      fetch-added (release) by each helper once it finds no item left, behind a release fence over what it wrote; the program wave spins until it reads
//               n_waves - 1 and takes an acquire fence: the round's results are then visible to it.
// The waves of a workgroup share a CU and its L1, so workgroup-scope fences, without cache maintenance, order global memory against the counters in LDS.
// rtk_myers_leaf_item, the item of a leaf round, is defined at the end of rtk_myers_lvl.h, behind rtk_myers_traceback which it calls, where it always stood in the code object.
#ifndef RTK_MYERS_COOP_H
#define RTK_MYERS_COOP_H
#include "rtk_myers_blocks.h"

#if defined(RTK_MULTIWAVE) && !defined(RTK_SIM)

// The row blocks (64 words = 4096 query rows each) of ONE pass run on the waves of the workgroup at the same time: block b consumes
// the horizontal deltas block b-1 leaves at its bottom row one 64-column chunk behind it, so a pass over B blocks takes about n + 128 B steps instead of B n.
#define RTK_COOP_MAXB 512 // row blocks of all the passes of a round
#define RTK_COOP_MAXJ 64  // passes of a round (two per Hirschberg sub-problem)
struct RtkCoop { RtkCoopJob job[RTK_COOP_MAXJ]; int first[RTK_COOP_MAXJ + 1]; int node[RTK_COOP_MAXJ / 2][8]; int n_jobs, n_items, seq, n_done, exit_flag, n_waves, next_item; int progress[RTK_COOP_MAXB];
                 // a round of leaf tracebacks (rtk_myers_alignment_bfs): every wave of the workgroup takes leaves, each with its own traceback table
                 int n_gangs; RtkGangCtx gctx; // gang sweeps of a round (items 0 .. n_gangs - 1; the row blocks of the jobs follow)
                 int n_leaf_waves; // waves that own a work area for leaf tracebacks (the others sit a leaf round out)
                 int leaf_mode, liupac; const char* lq; const char* lt; int32_t* llist; uint8_t* lmoves; MyersScratch* lsc; uint32_t lnm[16]; const uint64_t* lneed; };
__device__ __noinline__ void rtk_myers_leaf_item(RtkCoop* st, int wave, int x);
__device__ __noinline__ void rtk_myers_gang(const RtkGangCtx& C_, int gang_);
__device__ __forceinline__ RtkCoop* rtk_coop() { __shared__ RtkCoop st; return &st; }

__device__ __forceinline__ void rtk_myers_coop_run(RtkCoop* st, int wave) {
    // A round is a list of passes; pass j owns the row blocks first[j] .. first[j + 1) of the round's block list (next_item, above: why nobody waits for ever).
    const int nit = rtk_coop_ld(&st->n_items);
    const bool leaves = rtk_coop_ld(&st->leaf_mode) != 0;
    if (leaves && wave >= rtk_coop_ld(&st->n_leaf_waves)) return; // no work area for a traceback table
    const int ng = leaves ? 0 : rtk_coop_ld(&st->n_gangs);
    int j = 0;
    for (;;) {
        int i = 0;
        if (rtk_lane() == 0) i = __hip_atomic_fetch_add(&st->next_item, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= nit) break;
        if (leaves) { rtk_myers_leaf_item(st, wave, i); continue; }
        if (i < ng) { rtk_myers_gang(st->gctx, i); continue; }
        i -= ng;
        while (i >= rtk_coop_ld(&st->first[j + 1])) ++j;
        const int f = rtk_coop_ld(&st->first[j]);
        if (rtk_coop_ld(&st->job[j].ring)) rtk_myers_ring(st->job[j]); // a banded pass on one wave
        else rtk_myers_block(st->job[j], i - f, st->progress + f);
    }
}

// helper waves of the workgroup: wait for passes until the program wave says it is done
__device__ __forceinline__ void rtk_myers_coop_helper(int wave) {
    RtkCoop* st = rtk_coop();
    int seen = 0;
    while (true) {
        int sq;
        while ((sq = rtk_coop_ld(&st->seq)) == seen) { if (rtk_coop_ld(&st->exit_flag)) return; __builtin_amdgcn_s_sleep(32); }
        seen = sq;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        rtk_myers_coop_run(st, wave);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (rtk_lane() == 0) __hip_atomic_fetch_add(&st->n_done, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// program wave: publish one pass -- or two passes of the same query length (q2 != nullptr: the second one works on the columns behind
// the first one's in the carry / score arrays) --, take part, wait for the helpers. Returns false when not worth sharing (caller runs them alone).
__device__ __forceinline__ bool rtk_myers_pass_coop(const MyersScratch& sc, const MySeq& q, const MySeq& t, int top_h, bool iupac, const RtkBand& band, uint64_t* fin_pv, uint64_t* fin_mv,
                                                    const MySeq* q2 = nullptr, const MySeq* t2 = nullptr, uint64_t* fin_pv2 = nullptr, uint64_t* fin_mv2 = nullptr) {
    RtkCoop* st = rtk_coop();
    const int nwv = rtk_coop_ld(&st->n_waves);
    const int W = (q.n + 63) >> 6, nj = q2 ? 2 : 1;
    const int it1 = rtk_pass_items(q.n, t.n, band), it2 = q2 ? rtk_pass_items(q2->n, t2->n, band) : 0;
    if (nwv < 2 || it1 + it2 < 2 || it1 + it2 > RTK_COOP_MAXB || (q2 && q2->n != q.n)) return false;
    if (static_cast<uint64_t>(8 * W + 8) > 15ull * sc.w_cap) return false; // two profile tables
    if (rtk_lane() == 0) {
        st->job[0] = rtk_make_job(sc, q, t, top_h, iupac, band, fin_pv, fin_mv);
        if (q2) { RtkCoopJob j = rtk_make_job(sc, *q2, *t2, top_h, iupac, band, fin_pv2, fin_mv2); j.carry += t.n; j.colscore += t.n; j.peq4 += 4ull * W + 4; st->job[1] = j; }
        st->n_jobs = nj; st->n_items = it1 + it2; st->first[0] = 0; st->first[1] = it1; st->first[2] = it1 + it2;
    }
    for (int i = rtk_lane(); i < it1 + it2; i += RTK_WAVE) st->progress[i] = 0;
    if (rtk_lane() == 0) { st->n_done = 0; st->next_item = 0; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // the strings of the pass (global memory) and the mailbox
    rtk_coop_st(&st->seq, rtk_coop_ld(&st->seq) + 1);
    rtk_myers_coop_run(st, 0);
    while (rtk_coop_ld(&st->n_done) < nwv - 1) __builtin_amdgcn_s_sleep(8);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return true;
}

// program wave: the passes in st->job[0 .. n_jobs) with their block ranges st->first[] are ready: run them with the helpers
__device__ __forceinline__ void rtk_myers_round_coop(RtkCoop* st, int n_items) {
    const int nwv = rtk_coop_ld(&st->n_waves);
    for (int i = rtk_lane(); i < n_items; i += RTK_WAVE) st->progress[i] = 0;
    if (rtk_lane() == 0) { st->n_done = 0; st->next_item = 0; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    rtk_coop_st(&st->seq, rtk_coop_ld(&st->seq) + 1);
    rtk_myers_coop_run(st, 0);
    while (rtk_coop_ld(&st->n_done) < nwv - 1) __builtin_amdgcn_s_sleep(8);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#endif
#endif
