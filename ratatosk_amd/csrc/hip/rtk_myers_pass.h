// The generic pass of a query over a target on the device: any length, any byte in the target, optionally the traceback table; and the
// banded NW pass. Both pick their schedule here: shared with the helper waves, row blocks or ring on this wave, or the loop below.
#ifndef RTK_MYERS_PASS_H
#define RTK_MYERS_PASS_H
#include "rtk_myers_sweep.h"
#include "rtk_myers_blocks.h"
#include "rtk_myers_coop.h"

#ifndef RTK_SIM // the simulator's passes: rtk_myers_sim.h

// Full pass of query q over target t. Writes colscore[j] = D[m][j+1] for every column; optionally the traceback
// table (store != 0) and the final vertical delta vectors (fin_pv/fin_mv, W words each) for column extraction.
// top_h: +1 NW/SHW, 0 HW (edlib.cpp:584).
RTK_FN void rtk_myers_pass(const MyersScratch& sc_, MySeq q_, MySeq t_, int top_h_, bool iupac_, int store_, uint64_t* fin_pv_, uint64_t* fin_mv_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    MySeq q, t; q.p = rtk_u(q_.p); q.n = rtk_u(q_.n); q.rev = rtk_u(q_.rev); t.p = rtk_u(t_.p); t.n = rtk_u(t_.n); t.rev = rtk_u(t_.rev);
    const int top_h = rtk_u(top_h_), store = rtk_u(store_); const bool iupac = rtk_u(iupac_); uint64_t* fin_pv = rtk_u(fin_pv_); uint64_t* fin_mv = rtk_u(fin_mv_);
    const int m = q.n, n = t.n, W = (m + 63) >> 6, last_bit = (m - 1) & 63;
    const int lane = rtk_lane();
#ifdef RTK_MULTIWAVE
    if (!store && rtk_myers_pass_coop(sc, q, t, top_h, iupac, rtk_band_full(), fin_pv, fin_mv)) { rtk_sync(); return; } // several row blocks: shared with the helper waves of the workgroup
#endif
    if (!store && W > 64) { // several row blocks on this wave: the block sweep without branches in the step
        const RtkCoopJob j = rtk_make_job(sc, q, t, top_h, iupac, rtk_band_full(), fin_pv, fin_mv);
        for (int b = 0; b < ((W + 63) >> 6); ++b) rtk_myers_block(j, b, nullptr);
        rtk_sync();
        return;
    }
    // local copies: the scratch descriptor lives in private memory and its fields could alias the stores below,
    // which would force a (slow) reload of every pointer on every step
    int8_t* __restrict__ const carry = rtk_u(sc.carry); int32_t* __restrict__ const colscore = rtk_u(sc.colscore); uint64_t* __restrict__ const tb = rtk_u(sc.tb);
    const char* __restrict__ const tp = t.p; const int trev = t.rev;
    const char* __restrict__ const qp = q.p; const int qrev = q.rev;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int nw = (W - w0) < 64 ? (W - w0) : 64;
        const int w = w0 + lane;
        const bool has_word = lane < nw;
        const bool is_last_word = has_word && (w == W - 1);
        const bool is_block_tail = (lane == nw - 1);
        const int bit = is_last_word ? last_bit : 63;
        // this lane's profile words for A, C, G, T stay in registers for the whole pass; other classes are fetched on demand
        uint64_t eqA = 0, eqC = 0, eqG = 0, eqT = 0;
        if (has_word) { // built straight from the query characters of this word (no profile table in memory on the device); rtk_myers_eq4 computes the same words
            const int lim = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
            for (int i = 0; i < lim; ++i) {
                const unsigned char qc = static_cast<unsigned char>(qrev ? qp[m - 1 - (64 * w + i)] : qp[64 * w + i]);
                const uint32_t bm = rtk_eq_classes(rtk_cls(qc), iupac) & 0xFu; // bases this query character equals
                eqA |= static_cast<uint64_t>(bm & 1u) << i; eqC |= static_cast<uint64_t>((bm >> 1) & 1u) << i;
                eqG |= static_cast<uint64_t>((bm >> 2) & 1u) << i; eqT |= static_cast<uint64_t>((bm >> 3) & 1u) << i;
            }
        }
        uint64_t Pv = ~0ull, Mv = 0ull;
        if (W <= 64) { // single row block: is the target plain A/C/G/T? then take the branch-free sweep
            bool plain = true;
            for (int c0 = 0; c0 < n && plain; c0 += 64) {
                const int cj = c0 + lane;
                bool okc = true;
                if (cj < n) { const unsigned char ch = static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj]); okc = (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
                plain = (rtk_ballot(!okc) == 0ull);
            }
            if (plain) {
                if (store) rtk_myers_sweep_acgt<1>(m, n, W, top_h, last_bit, tp, trev, eqA, eqC, eqG, eqT, colscore, tb, Pv, Mv);
                else rtk_myers_sweep_acgt<0>(m, n, W, top_h, last_bit, tp, trev, eqA, eqC, eqG, eqT, colscore, tb, Pv, Mv);
                if (fin_pv && has_word) { fin_pv[w] = Pv; fin_mv[w] = Mv; }
                rtk_sync();
                continue;
            }
        }
        int hout_prev = 0; unsigned tc_prev = 0;
        int score = m;
        const int steps = n + nw - 1;
        // The target character of a column enters at lane 0 and then rides down the lanes together with the horizontal
        // delta (one packed __shfl_up per step): no memory access on the step-to-step dependency chain.
        const bool last_block = (w0 + nw >= W);
        int sbuf = 0;       // last-row scores of up to 64 columns, one per lane (lane = column & 63), flushed with one coalesced store
        for (int c0 = 0; c0 < steps; c0 += 64) {
            const int cj = c0 + lane;
            int my_t = (cj < n) ? static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj])) : 0; // lane j holds t[c0 + j] ...
            int my_c = (w0 != 0 && cj < n) ? static_cast<int>(carry[cj]) : top_h; // ... and the delta entering row block w0
            asm volatile("" : "+v"(my_t), "+v"(my_c)); // the loads are complete here, so the step loop below carries no memory wait
            const int lim = (steps - c0) < 64 ? (steps - c0) : 64;
            for (int j = 0; j < lim; ++j) {
                const int s = c0 + j;
                const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
                const int in_c = __builtin_amdgcn_readlane(my_c, j);
                const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
                // wave_shr:1 (DPP): lane l receives lane l-1's value, lane 0 keeps `old` = the values entering the block
                const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(in_c + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
                const int hin = static_cast<int>(got & 0xFFu) - 1;
                const unsigned tc = got >> 8;
                const int col = s - lane;
                const bool active = has_word && col >= 0 && col < n;
                if (active) {
                    uint64_t Eq;
                    if (tc == 'A') Eq = eqA; else if (tc == 'C') Eq = eqC; else if (tc == 'G') Eq = eqG; else if (tc == 'T') Eq = eqT;
                    else { // rare: IUPAC code, N or foreign byte in the target -> compare the 64 query characters of this word directly
                        Eq = 0; const int lim2 = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
                        for (int i = 0; i < lim2; ++i) Eq |= static_cast<uint64_t>(rtk_chars_equal(static_cast<unsigned char>(qrev ? qp[m - 1 - (64 * w + i)] : qp[64 * w + i]), static_cast<unsigned char>(tc), iupac)) << i;
                    }
                    uint64_t Ph, Mh;
                    const int hout = rtk_myers_step(Pv, Mv, Eq, hin, bit, Ph, Mh);
                    if (store) { rtk_tb_put(tb + 4ull * RTK_TB(col, w, n), Pv, Mv, Ph, Mh); }
                    if (is_block_tail) { if (!last_block) carry[col] = static_cast<int8_t>(hout); else score += hout; }
                    hout_prev = hout;
                }
                tc_prev = tc;
                if (last_block) { // park the tail lane's score of column (s - nw + 1) in lane (column & 63); store 64 of them at once
                    const int tcol = s - (nw - 1);
                    if (tcol >= 0 && tcol < n) {
                        const int sv = __builtin_amdgcn_readlane(score, nw - 1);
                        if (lane == (tcol & 63)) sbuf = sv;
                        if ((tcol & 63) == 63 || tcol == n - 1) { const int cc = (tcol & ~63) + lane; if (cc <= tcol) colscore[cc] = sbuf; }
                    }
                }
            }
        }
        if (fin_pv && has_word) { fin_pv[w] = Pv; fin_mv[w] = Mv; }
        rtk_sync();
    }
    rtk_sync();
}

// NW pass (top row +1 per column) over the band [dlo, dhi] of diagonals only. Leaves the vertical deltas of every word at the word's last
// column in fin_pv / fin_mv (both required) and returns the granularity of the schedule it took (1: ring, 64: row blocks), which
// rtk_myers_column needs to tell the rows that are inside the band at the last column from the others.
RTK_FN int rtk_myers_pass_banded(const MyersScratch& sc_, MySeq q_, MySeq t_, bool iupac_, int dlo_, int dhi_, uint64_t* fin_pv_, uint64_t* fin_mv_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    MySeq q, t; q.p = rtk_u(q_.p); q.n = rtk_u(q_.n); q.rev = rtk_u(q_.rev); t.p = rtk_u(t_.p); t.n = rtk_u(t_.n); t.rev = rtk_u(t_.rev);
    const bool iupac = rtk_u(iupac_); uint64_t* fin_pv = rtk_u(fin_pv_); uint64_t* fin_mv = rtk_u(fin_mv_);
    RtkBand band; band.dlo = rtk_u(dlo_); band.dhi = rtk_u(dhi_);
    const int m = q.n, n = t.n, W = (m + 63) >> 6;
    const int gran = rtk_band_gran(m, band.dlo, band.dhi);
#ifdef RTK_MULTIWAVE
    if (rtk_myers_pass_coop(sc, q, t, 1, iupac, band, fin_pv, fin_mv)) { rtk_sync(); return gran; }
#endif
    const RtkCoopJob j = rtk_make_job(sc, q, t, 1, iupac, band, fin_pv, fin_mv);
    if (gran == 1) rtk_myers_ring(j);
    else { const int nb = (rtk_band_words(m, n, band.dlo) + 63) >> 6; for (int b = 0; b < nb; ++b) rtk_myers_block(j, b, nullptr); }
    rtk_sync();
    return gran;
}
#endif
#endif
