// A pass over several row blocks as work items of one wave or of the waves of a workgroup: the 4096-row block sweep and the ring sweep of a narrow band.
#ifndef RTK_MYERS_BLOCKS_H
#define RTK_MYERS_BLOCKS_H
#include "rtk_myers_band.h"
#include "rtk_myers_step.h"

#ifndef RTK_SIM // the simulator sweeps column by column: rtk_myers_sim.h

struct RtkGangCtx { const char* q; const char* t; char* stage; uint64_t* peq; uint64_t* fin; int32_t* nodes; int n_nodes, iupac; }; // one round of gang sweeps (rtk_myers_lvl.h)
struct RtkCoopJob { const char* qp; const char* tp; int m, n, qrev, trev, top_h, iupac; uint64_t* fin_pv; uint64_t* fin_mv; int8_t* carry; int32_t* colscore; int dlo, dhi, ring; uint64_t* peq4; };
__device__ __forceinline__ int rtk_coop_ld(const int* p) { return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }
__device__ __forceinline__ void rtk_coop_st(int* p, int v) { if (rtk_lane() == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// One row block (64 words = 4096 query rows) of a pass over several blocks: same arithmetic as the general loop of rtk_myers_pass, without
// branches in the step when the target holds A/C/G/T only. progress == nullptr: the blocks are swept one after the other by this wave;
// otherwise the counters of the pass (completed columns per block), through which the waves of a workgroup follow each other.
// Band (J.dlo, J.dhi): the block only sweeps the columns [cb_lo, cb_hi] in which one of its words has a row inside the band; it starts from
// the "+1 per row" vertical deltas, takes "+1 per column" from above once the block above is past its own last column, and leaves the
// vertical deltas of column cb_hi in fin_pv / fin_mv (rtk_myers_column knows which rows of them are inside the band at the last column).
__device__ __noinline__ void rtk_myers_block(const RtkCoopJob& J, int b, int* progress) {
    const char* __restrict__ const qp = rtk_u(J.qp); const char* __restrict__ const tp = rtk_u(J.tp);
    const int m = rtk_u(J.m), n = rtk_u(J.n), qrev = rtk_u(J.qrev), trev = rtk_u(J.trev), top_h = rtk_u(J.top_h); const bool iupac = rtk_u(J.iupac) != 0;
    const int dlo = rtk_u(J.dlo), dhi = rtk_u(J.dhi);
    int8_t* __restrict__ const carry = rtk_u(J.carry); int32_t* __restrict__ const colscore = rtk_u(J.colscore);
    uint64_t* const fin_pv = rtk_u(J.fin_pv); uint64_t* const fin_mv = rtk_u(J.fin_mv);
    const int W = (m + 63) >> 6, last_bit = (m - 1) & 63;
    const int lane = rtk_lane();
    const int w0 = 64 * b;
    const int nw = (W - w0) < 64 ? (W - w0) : 64;
    const int w = w0 + lane;
    const bool has_word = lane < nw;
    const bool is_last_word = has_word && (w == W - 1);
    const bool is_block_tail = (lane == nw - 1);
    const int bit = is_last_word ? last_bit : 63;
    const bool last_block = (w0 + nw >= W);
    const bool banded = !(dlo <= -m && dhi >= n);
    const int cb_lo = rtk_band_clo(w0, dlo, 64), cb_hi = rtk_band_chi(w0, W, n, dhi, 64); // columns of this block
    const int prev_hi = b > 0 ? rtk_band_chi(w0 - 1, W, n, dhi, 64) : -1;               // last column of the block above
    const int above_h = b == 0 ? top_h : 1;                                              // delta entering the block where nothing is above it
    if (cb_lo > cb_hi) { // no column (below the band): nothing to do, nobody waits
        if (progress) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); if (!last_block) rtk_coop_st(&progress[b], n); } else rtk_sync();
        return;
    }
    const int nc = cb_hi - cb_lo + 1;
    uint64_t eqA = 0, eqC = 0, eqG = 0, eqT = 0;
    if (has_word) rtk_myers_eq4(qp, m, qrev, w, iupac, eqA, eqC, eqG, eqT);
    uint64_t Pv = ~0ull, Mv = 0ull;
    int hout_prev = 0; unsigned tc_prev = 0;
    int score = m;
    const int steps = nc + nw - 1;
    int sbuf = 0;
    const bool track = last_block && !banded; // bottom-row scores of every column: only meaningful when the sweep starts at column 0
    bool plain = true; // target made of A/C/G/T only: the profile word is a select, no branches in the step
    for (int c0 = cb_lo; c0 <= cb_hi && plain; c0 += 64) {
        const int cj = c0 + lane; bool okc = true;
        if (cj <= cb_hi) { const unsigned char ch = static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj]); okc = (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
        plain = (rtk_ballot(!okc) == 0ull);
    }
    for (int c0 = 0; c0 < steps; c0 += 64) {
        const int cj = cb_lo + c0 + lane; // absolute column this lane fetches for the chunk
        if (b > 0 && progress && cb_lo + c0 <= prev_hi) { // the deltas of the chunk's columns must have left the block above (as far as it goes)
            const int need = (cb_lo + c0 + 64) <= prev_hi ? (cb_lo + c0 + 64) : (prev_hi + 1);
            while (rtk_coop_ld(&progress[b - 1]) < need) __builtin_amdgcn_s_sleep(8);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        int my_t = (cj <= cb_hi) ? static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj])) : 0;
        int my_c = (b != 0 && cj <= prev_hi) ? static_cast<int>(carry[cj]) : above_h;
        asm volatile("" : "+v"(my_t), "+v"(my_c));
        const int lim = (steps - c0) < 64 ? (steps - c0) : 64;
        if (plain && track) { // the block that holds the last query row of an unbanded pass: its bottom-row scores are parked 64 columns at a time
            for (int j = 0; j < lim; ++j) {
                const int s = c0 + j;
                const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
                const int in_c = __builtin_amdgcn_readlane(my_c, j);
                const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
                const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(in_c + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
                const int hin = static_cast<int>(got & 0xFFu) - 1;
                const unsigned tc = got >> 8;
                const unsigned sel = (tc >> 1) & 3u;
                const uint64_t Eq = (sel & 2u) ? ((sel & 1u) ? eqG : eqT) : ((sel & 1u) ? eqC : eqA);
                uint64_t nPv = Pv, nMv = Mv, Ph, Mh;
                const int hout = rtk_myers_step(nPv, nMv, Eq, hin, bit, Ph, Mh);
                const int lc = s - lane; // column index inside the block's range
                const bool active = has_word && lc >= 0 && lc < nc;
                Pv = active ? nPv : Pv; Mv = active ? nMv : Mv; hout_prev = active ? hout : hout_prev;
                score += (active && is_block_tail) ? hout : 0;
                tc_prev = tc;
                const int tcol = s - (nw - 1);
                if (tcol >= 0 && tcol < n) { // uniform
                    const int sv = __builtin_amdgcn_readlane(score, nw - 1);
                    sbuf = (lane == (tcol & 63)) ? sv : sbuf;
                    if ((tcol & 63) == 63 || tcol == n - 1) { const int cc = (tcol & ~63) + lane; if (cc <= tcol) colscore[cc] = sbuf; }
                }
            }
        } else
        if (plain) { // the common case, predicated instead of branched (scalar branches cost an instruction-fetch restart)
            for (int j = 0; j < lim; ++j) {
                const int s = c0 + j;
                const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
                const int in_c = __builtin_amdgcn_readlane(my_c, j);
                const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
                const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(in_c + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
                const int hin = static_cast<int>(got & 0xFFu) - 1;
                const unsigned tc = got >> 8;
                const unsigned sel = (tc >> 1) & 3u; // 'A' -> 0, 'C' -> 1, 'T' -> 2, 'G' -> 3
                const uint64_t Eq = (sel & 2u) ? ((sel & 1u) ? eqG : eqT) : ((sel & 1u) ? eqC : eqA);
                uint64_t nPv = Pv, nMv = Mv, Ph, Mh;
                const int hout = rtk_myers_step(nPv, nMv, Eq, hin, bit, Ph, Mh);
                const int lc = s - lane;
                const bool active = has_word && lc >= 0 && lc < nc;
                Pv = active ? nPv : Pv; Mv = active ? nMv : Mv; hout_prev = active ? hout : hout_prev;
                if (active && is_block_tail && !last_block) carry[cb_lo + lc] = static_cast<int8_t>(hout);
                tc_prev = tc;
            }
        } else
        for (int j = 0; j < lim; ++j) {
            const int s = c0 + j;
            const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
            const int in_c = __builtin_amdgcn_readlane(my_c, j);
            const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
            const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(in_c + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
            const int hin = static_cast<int>(got & 0xFFu) - 1;
            const unsigned tc = got >> 8;
            const int lc = s - lane;
            const bool active = has_word && lc >= 0 && lc < nc;
            if (active) {
                uint64_t Eq;
                if (tc == 'A') Eq = eqA; else if (tc == 'C') Eq = eqC; else if (tc == 'G') Eq = eqG; else if (tc == 'T') Eq = eqT;
                else {
                    Eq = 0; const int lim2 = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
                    for (int i = 0; i < lim2; ++i) Eq |= static_cast<uint64_t>(rtk_chars_equal(rtk_job_qc(qp, m, qrev, 64 * w + i), static_cast<unsigned char>(tc), iupac)) << i;
                }
                uint64_t Ph, Mh;
                const int hout = rtk_myers_step(Pv, Mv, Eq, hin, bit, Ph, Mh);
                if (is_block_tail) { if (!last_block) carry[cb_lo + lc] = static_cast<int8_t>(hout); else score += hout; }
                hout_prev = hout;
            }
            tc_prev = tc;
            if (track) {
                const int tcol = s - (nw - 1);
                if (tcol >= 0 && tcol < n) {
                    const int sv = __builtin_amdgcn_readlane(score, nw - 1);
                    if (lane == (tcol & 63)) sbuf = sv;
                    if ((tcol & 63) == 63 || tcol == n - 1) { const int cc = (tcol & ~63) + lane; if (cc <= tcol) colscore[cc] = sbuf; }
                }
            }
        }
        if (!last_block && progress) { // columns whose delta has left this block: the tail lane is nw - 1 columns behind lane 0
            int done = c0 + lim - (nw - 1); done = done < 0 ? 0 : (done > nc ? nc : done);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            rtk_coop_st(&progress[b], cb_lo + done);
        }
    }
    if (fin_pv && has_word) { fin_pv[w] = Pv; fin_mv[w] = Mv; }
    if (progress) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); if (!last_block) rtk_coop_st(&progress[b], n); }
    else rtk_sync();
}

// ------------------------------------------------------------------------------------------------ banded pass on one wave: the ring
// NW pass (top row +1 per column) over a band of at most RTK_RING_MAX_BAND diagonals, any number of query words. Word w owns lane w & 63
// and is swept over its own columns [64 w + dlo, 64 w + 63 + dhi] (clipped to the matrix) at step column + w, as in the anti-diagonal
// pipeline of the row blocks; the words above and below it at that moment sit in the neighbouring lanes (the ring closes from lane 63 to
// lane 0: DPP wave_ror:1). The word at the top of the band (the "head": nothing above it any more) takes +1 per column from above and the
// target character of its column from the chunk register; every other word takes both from the lane above. A word that is past its last
// column parks its vertical deltas in fin_pv / fin_mv and its lane moves on to word + 64, whose first column lies at least 65 steps later
// because the band is narrower than 4096 - 65 - 31 diagonals: the switch is done lazily, once per chunk of 64 steps. J.peq4: 4 words
// (A, C, G, T profile) per query word, filled here.
template <int PLAIN>
__device__ __forceinline__ void rtk_myers_ring_sweep(const RtkCoopJob& J) {
    const char* __restrict__ const qp = rtk_u(J.qp); const char* __restrict__ const tp = rtk_u(J.tp);
    const int m = rtk_u(J.m), n = rtk_u(J.n), qrev = rtk_u(J.qrev), trev = rtk_u(J.trev); const bool iupac = rtk_u(J.iupac) != 0;
    const int dlo = rtk_u(J.dlo), dhi = rtk_u(J.dhi);
    uint64_t* const fin_pv = rtk_u(J.fin_pv); uint64_t* const fin_mv = rtk_u(J.fin_mv);
    const uint64_t* __restrict__ const peq4 = rtk_u(J.peq4);
    const int W = (m + 63) >> 6, last_bit = (m - 1) & 63;
    const int Wa = rtk_u(rtk_band_words(m, n, dlo));
    const int lane = rtk_lane();
    // this lane's current word
    int w = lane; bool live = w < Wa;
    uint64_t eqA = 0, eqC = 0, eqG = 0, eqT = 0, Pv = ~0ull, Mv = 0ull;
    int clo_w = 0x7fffffff, chi_w = -1, head_from = 0x7fffffff, bit = 63;
#define RTK_RING_LOAD_WORD()                                                                                                                  \
    {                                                                                                                                        \
        eqA = peq4[4ull * w]; eqC = peq4[4ull * w + 1]; eqG = peq4[4ull * w + 2]; eqT = peq4[4ull * w + 3];                                   \
        Pv = ~0ull; Mv = 0ull;                                                                                                               \
        clo_w = rtk_band_clo(w, dlo, 1); chi_w = rtk_band_chi(w, W, n, dhi, 1);                                                               \
        head_from = (w == 0) ? -0x7fffffff : 64 * w + dhi; /* columns at which no word is above this one (dhi < 2^29: no overflow) */       \
        bit = (w == W - 1) ? last_bit : 63;                                                                                                  \
    }
    if (live) RTK_RING_LOAD_WORD()
    int hout_prev = 0; unsigned tc_prev = 0;
    const int steps = rtk_u(n + Wa - 1);
    int s = 0, w_head = 0, head_chi = rtk_u(rtk_band_chi(0, W, n, dhi, 1)), cb = 0;
    int nxt_t = 0;
    { const int cn = lane; if (cn < n) nxt_t = static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cn] : tp[cn])); }
    int my_t = nxt_t;
    { const int cn = 64 + lane; nxt_t = 0; if (cn < n) nxt_t = static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cn] : tp[cn])); }
    // The sweep is cut into runs in which nothing wave-level changes: the head of the band stays the same word and its columns stay in
    // the chunk register, so the run is a counted loop with scalar control (column of the head = c0 + j).
    while (s < steps) {
        s = rtk_u(s); w_head = rtk_u(w_head); head_chi = rtk_u(head_chi); cb = rtk_u(cb);
        { // words that are past their last column: park the deltas, take the next word of this lane
            const bool done = live && (s - w > chi_w);
            if (rtk_ballot(done) != 0ull) {
                if (done) {
                    if (fin_pv) { fin_pv[w] = Pv; fin_mv[w] = Mv; }
                    w += 64; live = w < Wa;
                    if (live) RTK_RING_LOAD_WORD() else { clo_w = 0x7fffffff; chi_w = -1; }
                }
            }
        }
        asm volatile("" : "+v"(my_t));
        const int c0 = s - w_head; // column of the head at step s
        int run = steps - s;
        { const int r1 = head_chi - c0 + 1, r2 = cb + 64 - c0; run = run < r1 ? run : r1; run = run < r2 ? run : r2; run = run < 64 ? run : 64; run = rtk_u(run); }
        const int ci = c0 - cb;
        for (int j = 0; j < run; ++j) {
            const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, ci + j));
            const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
            unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(mine), 0x13C, 0xF, 0xF, false)); // wave_ror:1
            const int c = s + j - w;
            got = (c >= head_from) ? (2u | (in_t << 8)) : got;
            const int hin = static_cast<int>(got & 0xFFu) - 1;
            const unsigned tc = got >> 8;
            const bool active = c >= clo_w && c <= chi_w;
            if (PLAIN) {
                const unsigned sel = (tc >> 1) & 3u; // 'A' -> 0, 'C' -> 1, 'T' -> 2, 'G' -> 3
                const uint64_t Eq = (sel & 2u) ? ((sel & 1u) ? eqG : eqT) : ((sel & 1u) ? eqC : eqA);
                uint64_t nPv = Pv, nMv = Mv, Ph, Mh;
                const int hout = rtk_myers_step(nPv, nMv, Eq, hin, bit, Ph, Mh);
                Pv = active ? nPv : Pv; Mv = active ? nMv : Mv; hout_prev = active ? hout : hout_prev;
            } else if (active) {
                uint64_t Eq;
                if (tc == 'A') Eq = eqA; else if (tc == 'C') Eq = eqC; else if (tc == 'G') Eq = eqG; else if (tc == 'T') Eq = eqT;
                else { // rare: IUPAC code, N or foreign byte in the target -> compare the 64 query characters of this word directly
                    Eq = 0; const int lim2 = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
                    for (int i = 0; i < lim2; ++i) Eq |= static_cast<uint64_t>(rtk_chars_equal(rtk_job_qc(qp, m, qrev, 64 * w + i), static_cast<unsigned char>(tc), iupac)) << i;
                }
                uint64_t Ph, Mh;
                hout_prev = rtk_myers_step(Pv, Mv, Eq, hin, bit, Ph, Mh);
            }
            tc_prev = tc;
        }
        s += run;
        if (s - w_head > head_chi && w_head + 1 < Wa) { ++w_head; head_chi = rtk_band_chi(w_head, W, n, dhi, 1); } // the head of the band moves down (one step without a new column)
        if (s - w_head >= cb + 64) {
            cb += 64; my_t = nxt_t;
            const int cn = cb + 64 + lane; nxt_t = 0; if (cn < n) nxt_t = static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cn] : tp[cn]));
        }
    }
#undef RTK_RING_LOAD_WORD
    if (live && fin_pv) { fin_pv[w] = Pv; fin_mv[w] = Mv; }
}
__device__ __noinline__ void rtk_myers_ring(const RtkCoopJob& J) {
    const char* __restrict__ const qp = rtk_u(J.qp); const char* __restrict__ const tp = rtk_u(J.tp);
    const int m = rtk_u(J.m), n = rtk_u(J.n), qrev = rtk_u(J.qrev), trev = rtk_u(J.trev); const bool iupac = rtk_u(J.iupac) != 0;
    uint64_t* const peq4 = rtk_u(J.peq4);
    const int Wa = rtk_band_words(m, n, rtk_u(J.dlo));
    const int lane = rtk_lane();
    for (int w = lane; w < Wa; w += RTK_WAVE) { // the profile of every word that gets a column
        uint64_t a, c, g, t; rtk_myers_eq4(qp, m, qrev, w, iupac, a, c, g, t);
        peq4[4ull * w] = a; peq4[4ull * w + 1] = c; peq4[4ull * w + 2] = g; peq4[4ull * w + 3] = t;
    }
    bool plain = true;
    for (int c0 = 0; c0 < n && plain; c0 += 64) {
        const int cj = c0 + lane; bool okc = true;
        if (cj < n) { const unsigned char ch = static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj]); okc = (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
        plain = (rtk_ballot(!okc) == 0ull);
    }
    rtk_sync(); // the profile words are read by other lanes than wrote them
    if (plain) rtk_myers_ring_sweep<1>(J); else rtk_myers_ring_sweep<0>(J);
    rtk_sync();
}
// work items of a pass: one for the ring, else its row blocks that have a column
__device__ __forceinline__ bool rtk_pass_is_ring(int m, const RtkBand& band) { return rtk_band_gran(m, band.dlo, band.dhi) == 1; }
__device__ __forceinline__ int rtk_pass_items(int m, int n, const RtkBand& band) { return rtk_pass_is_ring(m, band) ? 1 : ((rtk_band_words(m, n, band.dlo) + 63) >> 6); }
__device__ __forceinline__ RtkCoopJob rtk_make_job(const MyersScratch& sc, const MySeq& q, const MySeq& t, int top_h, bool iupac, const RtkBand& band, uint64_t* fin_pv, uint64_t* fin_mv) {
    RtkCoopJob j; j.qp = q.p; j.tp = t.p; j.m = q.n; j.n = t.n; j.qrev = q.rev; j.trev = t.rev; j.top_h = top_h; j.iupac = iupac ? 1 : 0;
    j.fin_pv = fin_pv; j.fin_mv = fin_mv; j.carry = rtk_u(sc.carry); j.colscore = rtk_u(sc.colscore);
    j.dlo = band.dlo; j.dhi = band.dhi; j.ring = rtk_pass_is_ring(q.n, band) ? 1 : 0; j.peq4 = rtk_u(sc.peq);
    return j;
}
#endif
#endif
