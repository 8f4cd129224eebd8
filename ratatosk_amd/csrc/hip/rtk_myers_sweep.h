// The device sweeps over ONE row block (query <= 4096 characters) against a target of A/C/G/T: the anti-diagonal pipeline without branches in its step.
#ifndef RTK_MYERS_SWEEP_H
#define RTK_MYERS_SWEEP_H
#include "rtk_myers_step.h"

#ifndef RTK_SIM // the simulator sweeps column by column: rtk_myers_sim.h

// Branch-free anti-diagonal sweep for the common case: query <= 64 words (one row block), target made of A/C/G/T only.
// Scalar branches are expensive on CDNA (instruction-fetch restart), so everything per step is predicated with
// v_cndmask; the only branch left is the once-per-64-columns flush of the score buffer.
template <int STORE>
__device__ __forceinline__ void rtk_myers_sweep_acgt(int m, int n, int W, int top_h, int last_bit, const char* __restrict__ tp, int trev,
                                                     uint64_t eqA, uint64_t eqC, uint64_t eqG, uint64_t eqT,
                                                     int32_t* __restrict__ colscore, uint64_t* __restrict__ tb, uint64_t& Pv_out, uint64_t& Mv_out) {
    const int lane = rtk_lane();
    const int w = lane;
    const bool has_word = lane < W;
    const int bit = (w == W - 1) ? last_bit : 63;
    uint64_t Pv = ~0ull, Mv = 0ull;
    int hout_prev = 0; unsigned tc_prev = 0;
    int score = m, sbuf = 0;
    const int steps = n + W - 1;
    for (int c0 = 0; c0 < steps; c0 += 64) {
        const int cj = c0 + lane;
        int my_t = (cj < n) ? static_cast<int>(static_cast<unsigned char>(trev ? tp[n - 1 - cj] : tp[cj])) : 0;
        asm volatile("" : "+v"(my_t));
        const int lim = (steps - c0) < 64 ? (steps - c0) : 64;
        for (int j = 0; j < lim; ++j) {
            const int s = c0 + j;
            const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
            const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
            const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(top_h + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
            const int hin = static_cast<int>(got & 0xFFu) - 1;
            const unsigned tc = got >> 8;
            const unsigned sel = (tc >> 1) & 3u; // 'A' -> 0, 'C' -> 1, 'T' -> 2, 'G' -> 3
            const uint64_t Eq = (sel & 2u) ? ((sel & 1u) ? eqG : eqT) : ((sel & 1u) ? eqC : eqA);
            uint64_t nPv = Pv, nMv = Mv, Ph, Mh;
            const int hout = rtk_myers_step(nPv, nMv, Eq, hin, bit, Ph, Mh);
            const int col = s - lane;
            const bool active = has_word && col >= 0 && col < n;
            if (STORE) { if (active) { rtk_tb_put(tb + 4ull * RTK_TB(col, w, n), nPv, nMv, Ph, Mh); } }
            Pv = active ? nPv : Pv; Mv = active ? nMv : Mv;
            hout_prev = active ? hout : hout_prev;
            score += (active && lane == W - 1) ? hout : 0;
            tc_prev = tc;
            const int tcol = s - (W - 1);
            if (tcol >= 0) { // uniform
                const int sv = __builtin_amdgcn_readlane(score, W - 1);
                sbuf = (lane == (tcol & 63)) ? sv : sbuf;
                if ((tcol & 63) == 63 || tcol == n - 1) { const int cc = (tcol & ~63) + lane; if (cc <= tcol) colscore[cc] = sbuf; }
            }
        }
    }
    Pv_out = Pv; Mv_out = Mv;
}

// The LAST COLUMN of a finished sweep, from the vertical deltas its words hold once the pipeline has drained (lane w: query rows [B w, B w + B) in a word
// of B = 32 or 64 bits): D[i + 1][n] = n + the deltas of rows 0 .. i, a popcount prefix over the lanes as in rtk_myers_column. Reduced to its minimum
// over the query rows, the first and the last row that hold it and their number (st.best / first / last / cnt), and st.at_score = D[at][n] (0 <= at <= m).
__device__ __forceinline__ void rtk_last_column_stat(uint64_t pv, uint64_t mv, int B, int m, int n, int at, SweepStat& st) {
    const int lane = rtk_lane();
    const int row0 = B * lane;
    int rows = m - row0; rows = rows < 0 ? 0 : (rows > B ? B : rows);
    const uint64_t mask = rows >= 64 ? ~0ull : ((1ull << rows) - 1ull);
    pv &= mask; mv &= mask;
    int total;
    int v = n + rtk_wave_excl_scan(rtk_popc(pv) - rtk_popc(mv), &total);
    int best = 0x7fffffff, first = -1, last = -1, cnt = 0, atv = 0;
    for (int b = 0; b < rows; ++b) {
        v += static_cast<int>((pv >> b) & 1ull) - static_cast<int>((mv >> b) & 1ull);
        const bool lt = v < best, eq = v == best;
        best = lt ? v : best; first = lt ? row0 + b : first; last = (lt || eq) ? row0 + b : last; cnt = lt ? 1 : (cnt + (eq ? 1 : 0));
        atv = (row0 + b + 1 == at) ? v : atv;
    }
    const int gb = rtk_wave_min(best);
    const uint64_t has = rtk_ballot(cnt > 0 && best == gb); // lanes in row order: the first row is in the lowest of them, the last in the highest
    st.best = gb; st.first = __shfl(first, rtk_ffs(has) - 1, 64); st.last = __shfl(last, 63 - __builtin_clzll(has), 64);
    st.cnt = rtk_wave_sum((cnt > 0 && best == gb) ? cnt : 0);
    st.at_score = (at <= 0) ? n : __shfl(atv, (at - 1) / B, 64);
}
// Self-contained fast path for forward sequences with <= 64 query words: profile words built from 8 wide loads per lane,
// branch-free sweep, running minimum kept in scalar registers (no per-column score array), A/C/G/T check folded into the
// per-64-column target load. Returns plain == false (and no result) when the target holds another character.
// It keeps its own profile loop, not rtk_myers_eq4's: it reads forward sequences only, and 8 bytes at a time.
// COLUMN = 1: no last-row tracking; the last column is read once the sweep is done (rtk_last_column_stat, row `at`)
template <int STORE, int COLUMN = 0>
__device__ __forceinline__ SweepStat rtk_myers_fast(const char* __restrict__ qp, int m, const char* __restrict__ tp, int n, int top_h, bool iupac, uint64_t* __restrict__ tb, int at = 0) {
    SweepStat st; st.final_score = m; st.best = 0x7fffffff; st.first = -1; st.last = -1; st.cnt = 0; st.plain = true; st.at_score = 0;
    const int lane = rtk_lane();
    const int W = (m + 63) >> 6, last_bit = (m - 1) & 63;
    const int w = lane;
    const bool has_word = lane < W;
    uint64_t eqA = 0, eqC = 0, eqG = 0, eqT = 0;
    if (has_word) {
        const int lim = (m - 64 * w) < 64 ? (m - 64 * w) : 64;
        uint64_t qw[8];
        for (int j = 0; j < 8; ++j) { uint64_t x = 0; if (8 * j < lim) __builtin_memcpy(&x, qp + 64 * w + 8 * j, 8); qw[j] = x; } // may read up to 7 bytes past the query inside its padded buffer
        for (int i = 0; i < lim; ++i) {
            const unsigned char qc = static_cast<unsigned char>((qw[i >> 3] >> (8 * (i & 7))) & 0xFFull);
            uint32_t bm;
            if (qc == 'A') bm = 1u; else if (qc == 'C') bm = 2u; else if (qc == 'G') bm = 4u; else if (qc == 'T') bm = 8u;
            else bm = rtk_eq_classes(rtk_cls(qc), iupac) & 0xFu;
            eqA |= static_cast<uint64_t>(bm & 1u) << i; eqC |= static_cast<uint64_t>((bm >> 1) & 1u) << i;
            eqG |= static_cast<uint64_t>((bm >> 2) & 1u) << i; eqT |= static_cast<uint64_t>((bm >> 3) & 1u) << i;
        }
    }
    const int bit = (w == W - 1) ? last_bit : 63;
    uint64_t Pv = ~0ull, Mv = 0ull;
    int hout_prev = 0; unsigned tc_prev = 0;
    int score = m;
    int best = 0x7fffffff, first = -1, last = -1, cnt = 0, fin = m;
    uint64_t lastPh = 0, lastMh = 0; // STORE == 2: the horizontal deltas of this word's latest column
    const int steps = n + W - 1;
    for (int c0 = 0; c0 < steps; c0 += 64) {
        const int cj = c0 + lane;
        int my_t = 'A';
        if (cj < n) my_t = static_cast<int>(static_cast<unsigned char>(tp[cj]));
        if (rtk_ballot(!(my_t == 'A' || my_t == 'C' || my_t == 'G' || my_t == 'T')) != 0ull) { st.plain = false; return st; }
        asm volatile("" : "+v"(my_t));
        const int lim = (steps - c0) < 64 ? (steps - c0) : 64;
        for (int j = 0; j < lim; ++j) {
            const int s = c0 + j;
            const unsigned in_t = static_cast<unsigned>(__builtin_amdgcn_readlane(my_t, j));
            const unsigned mine = static_cast<unsigned>(hout_prev + 1) | (tc_prev << 8);
            const unsigned got = static_cast<unsigned>(__builtin_amdgcn_update_dpp(static_cast<int>(static_cast<unsigned>(top_h + 1) | (in_t << 8)), static_cast<int>(mine), 0x138, 0xF, 0xF, false));
            const int hin = static_cast<int>(got & 0xFFu) - 1;
            const unsigned tc = got >> 8;
            const unsigned sel = (tc >> 1) & 3u; // 'A' -> 0, 'C' -> 1, 'T' -> 2, 'G' -> 3
            const uint64_t Eq = (sel & 2u) ? ((sel & 1u) ? eqG : eqT) : ((sel & 1u) ? eqC : eqA);
            uint64_t nPv = Pv, nMv = Mv, Ph, Mh;
            const int hout = rtk_myers_step(nPv, nMv, Eq, hin, bit, Ph, Mh);
            const int col = s - lane;
            const bool active = has_word && col >= 0 && col < n;
            if (STORE == 1) { if (active) { rtk_tb_put(tb + 4ull * RTK_TB(col, w, n), nPv, nMv, Ph, Mh); } }
            if (STORE == 2) { lastPh = active ? Ph : lastPh; lastMh = active ? Mh : lastMh; }
            Pv = active ? nPv : Pv; Mv = active ? nMv : Mv;
            hout_prev = active ? hout : hout_prev;
            score += (active && lane == W - 1) ? hout : 0;
            tc_prev = tc;
            const int tcol = s - (W - 1);
            if (!COLUMN && tcol >= 0) { // wave-uniform: last-row score of column tcol, tracked in scalar registers
                const int sv = __builtin_amdgcn_readlane(score, W - 1);
                fin = sv;
                if (sv < best) { best = sv; first = tcol; last = tcol; cnt = 1; }
                else if (sv == best) { last = tcol; ++cnt; }
            }
        }
    }
    if (STORE == 2 && has_word) rtk_tb_put(tb + 4ull * w, Pv, Mv, lastPh, lastMh); // the last column, as a table of one column
    if (COLUMN) { rtk_last_column_stat(has_word ? Pv : 0ull, has_word ? Mv : 0ull, 64, m, n, at, st); return st; }
    st.final_score = fin; st.best = best; st.first = first; st.last = last; st.cnt = cnt;
    return st;
}

// The same sweep on 32-bit words (queries up to 2048 characters = 64 lanes): every bit-vector operation is one VALU instruction
// instead of two, and twice as many lanes work per step. The deltas are properties of the DP matrix, not of the word size, so the
// results - and the traceback table, written as the two halves of the 64-bit entries rtk_myers_walk reads - are the same.
// TRACK = 0: only the final score is wanted (NW); 1: minimum of the last row with its first / last position and count (SHW, HW);
// 2: the same of the last COLUMN, read once the sweep is done (rtk_last_column_stat, row `at`).
// STORE = 0: nothing is written; 1: the traceback table; 2: the table entries of the LAST column only, as a table of one column at the start of tb
// (entry w = Pv, Mv, Ph, Mh of word w at column n - 1: what rtk_myers_last_move_column reads) -- no store inside the sweep.
template <int STORE, int TRACK>
__device__ __forceinline__ SweepStat rtk_myers_fast32(const char* __restrict__ qp, int m, const char* __restrict__ tp, int n, int top_h, bool iupac, uint64_t* __restrict__ tb, int at = 0) {
    SweepStat st; st.final_score = m; st.best = 0x7fffffff; st.first = -1; st.last = -1; st.cnt = 0; st.plain = true; st.at_score = 0;
    const int lane = rtk_lane();
    const int W = (m + 31) >> 5, W64 = (m + 63) >> 6, last_bit = (m - 1) & 31;
    const int w = lane;
    const bool has_word = lane < W;
    uint32_t eqA = 0, eqC = 0, eqG = 0, eqT = 0;
    if (has_word) {
        const int lim = (m - 32 * w) < 32 ? (m - 32 * w) : 32;
        uint64_t qw[4];
        for (int j = 0; j < 4; ++j) { uint64_t x = 0; if (8 * j < lim) __builtin_memcpy(&x, qp + 32 * w + 8 * j, 8); qw[j] = x; } // may read up to 7 bytes past the query inside its padded buffer
        // four characters at a time: bits 1 and 2 of 'A' 0x41, 'C' 0x43, 'T' 0x54, 'G' 0x47 are a 2-bit code (0, 1, 2, 3); the two bit
        // planes are gathered into 32-bit masks and the four profile words are their boolean combinations. A word holding anything
        // else than A/C/G/T (IUPAC codes, N, the bytes past the query) is left to the character-by-character loop below.
        uint32_t p1 = 0, p2 = 0, done = 0;
        for (int j = 0; j < 8; ++j) {
            if (4 * j >= lim) break;
            const uint32_t x = static_cast<uint32_t>(qw[j >> 1] >> (32 * (j & 1)));
            const uint32_t b1 = (x >> 1) & 0x01010101u, b2 = (x >> 2) & 0x01010101u;
            const uint32_t b12 = b1 & b2, b2n = b2 & ~b1;
            const uint32_t recon = 0x41414141u + (b1 << 1) + (b12 << 2) + (b2n << 4) + (b2n << 1) + b2n; // 0x41 + 2*b1 + 4*b1*b2 + 0x13*(b2 & !b1), per byte
            if (x != recon || 4 * j + 4 > lim) continue;
            const uint32_t n1 = (b1 & 1u) | ((b1 >> 7) & 2u) | ((b1 >> 14) & 4u) | ((b1 >> 21) & 8u);
            const uint32_t n2 = (b2 & 1u) | ((b2 >> 7) & 2u) | ((b2 >> 14) & 4u) | ((b2 >> 21) & 8u);
            p1 |= n1 << (4 * j); p2 |= n2 << (4 * j); done |= 0xFu << (4 * j);
        }
        eqA = ~p1 & ~p2 & done; eqC = p1 & ~p2 & done; eqT = ~p1 & p2 & done; eqG = p1 & p2 & done;
        if (done != ((lim >= 32) ? ~0u : ((1u << lim) - 1u))) {
            for (int i = 0; i < lim; ++i) {
                if ((done >> i) & 1u) continue;
                const unsigned char qc = static_cast<unsigned char>((qw[i >> 3] >> (8 * (i & 7))) & 0xFFull);
                uint32_t bm;
                if (qc == 'A') bm = 1u; else if (qc == 'C') bm = 2u; else if (qc == 'G') bm = 4u; else if (qc == 'T') bm = 8u;
                else bm = rtk_eq_classes(rtk_cls(qc), iupac) & 0xFu;
                eqA |= (bm & 1u) << i; eqC |= ((bm >> 1) & 1u) << i; eqG |= ((bm >> 2) & 1u) << i; eqT |= ((bm >> 3) & 1u) << i;
            }
        }
    }
    const int bit = (w == W - 1) ? last_bit : 31;
    uint32_t Pv = ~0u, Mv = 0u;
    int hout_prev = 0; uint32_t m1_prev = 0, m2_prev = 0;
    uint32_t lastPh = 0, lastMh = 0; // STORE == 2: the horizontal deltas of this word's latest column
    int score = m;
    int vbest = 0x7fffffff, vfirst = -1, vlast = -1, vcnt = 0;
    const int steps = n + W - 1;
    // table entry of (column, 64-bit word) = two RtkTbHalf (low halves, high halves of Pv, Mv, Ph, Mh); this lane owns one of them
    RtkTbHalf* const tbh = reinterpret_cast<RtkTbHalf*>(tb) + 2ull * RTK_TB(0, w >> 1, n) + (w & 1); // this lane's half of the entries of its 64-bit word
    // one step of the anti-diagonal pipeline. MASKED = 1 while the pipeline fills or drains (some words have no column yet / any
    // more); in between every word has one and the activity test, the column range checks and the conditional updates fall away.
#define RTK_STEP32(MASKED)                                                                                                                   \
    {                                                                                                                                        \
        const int s = c0 + j;                                                                                                                \
        const int in_t = __builtin_amdgcn_readlane(my_t, j);                                                                                 \
        /* 'A' 0x41, 'C' 0x43, 'G' 0x47, 'T' 0x54: bit 1 picks C/G over A/T, bit 2 picks T/G over A/C. The two choices travel down the  */ \
        /* lanes as full-width masks next to the horizontal delta (three DPP moves), so that the profile word is three bitwise selects.  */ \
        const int hin = __builtin_amdgcn_update_dpp(top_h, hout_prev, 0x138, 0xF, 0xF, false);                                              \
        const uint32_t m1 = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(__builtin_amdgcn_sbfe(in_t, 1, 1), static_cast<int>(m1_prev), 0x138, 0xF, 0xF, false)); \
        const uint32_t m2 = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(__builtin_amdgcn_sbfe(in_t, 2, 1), static_cast<int>(m2_prev), 0x138, 0xF, 0xF, false)); \
        const uint32_t lo_ = (eqC & m1) | (eqA & ~m1), hi_ = (eqG & m1) | (eqT & ~m1);                                                       \
        const uint32_t Eq = (hi_ & m2) | (lo_ & ~m2);                                                                                        \
        uint32_t nPv = Pv, nMv = Mv, Ph, Mh;                                                                                                 \
        const int hout = rtk_myers_step32(nPv, nMv, Eq, hin, bit, Ph, Mh);                                                                   \
        const int col = s - lane;                                                                                                            \
        if (MASKED) {                                                                                                                        \
            const bool active = has_word && col >= 0 && col < n;                                                                             \
            if (STORE == 1) { if (active) { RtkTbHalf hv; hv.pv = nPv; hv.mv = nMv; hv.ph = Ph; hv.mh = Mh; tbh[2ull * static_cast<uint64_t>(col)] = hv; } } \
            if (STORE == 2) { lastPh = active ? Ph : lastPh; lastMh = active ? Mh : lastMh; }                                                \
            Pv = active ? nPv : Pv; Mv = active ? nMv : Mv;                                                                                  \
            hout_prev = active ? hout : hout_prev;                                                                                           \
            score += active ? hout : 0;                                                                                                      \
        } else {                                                                                                                             \
            if (STORE == 1) { if (has_word) { RtkTbHalf hv; hv.pv = nPv; hv.mv = nMv; hv.ph = Ph; hv.mh = Mh; tbh[2ull * static_cast<uint64_t>(col)] = hv; } } \
            if (STORE == 2) { lastPh = Ph; lastMh = Mh; }                                                                                    \
            Pv = nPv; Mv = nMv; hout_prev = hout; score += hout;                                                                             \
        }                                                                                                                                    \
        m1_prev = m1; m2_prev = m2;                                                                                                          \
        if (TRACK == 1) {                                                                                                                    \
            const int tcol = s - (W - 1);                                                                                                    \
            if (!(MASKED) || tcol >= 0) { /* every lane follows the minimum of ITS word's last row (selects, no branches); lane W - 1's is the one read at the end */ \
                const bool lt_ = score < vbest, eq_ = score == vbest;                                                                        \
                vbest = lt_ ? score : vbest; vfirst = lt_ ? tcol : vfirst; vlast = (lt_ || eq_) ? tcol : vlast; vcnt = lt_ ? 1 : (vcnt + (eq_ ? 1 : 0)); \
            }                                                                                                                                \
        }                                                                                                                                    \
    }
    int nxt_t = 'A'; // target characters of the NEXT 64 columns: requested one block ahead, so their latency hides behind 64 steps
    if (lane < n) nxt_t = static_cast<int>(static_cast<unsigned char>(tp[lane]));
    for (int c0 = 0; c0 < steps; c0 += 64) {
        int my_t = nxt_t;
        { const int cn = c0 + 64 + lane; nxt_t = 'A'; if (cn < n) nxt_t = static_cast<int>(static_cast<unsigned char>(tp[cn])); }
        if (rtk_ballot(!(my_t == 'A' || my_t == 'C' || my_t == 'G' || my_t == 'T')) != 0ull) { st.plain = false; return st; }
        asm volatile("" : "+v"(my_t));
        const int lim = (steps - c0) < 64 ? (steps - c0) : 64;
        // steps [0, W-1) fill the pipeline, [W-1, n) run it full, [n, n+W-1) drain it
        int j_fill = (W - 1) - c0; j_fill = j_fill < 0 ? 0 : (j_fill > lim ? lim : j_fill);
        int j_full = n - c0; j_full = j_full < j_fill ? j_fill : (j_full > lim ? lim : j_full);
        int j = 0;
        for (; j < j_fill; ++j) RTK_STEP32(1)
        for (; j < j_full; ++j) RTK_STEP32(0)
        for (; j < lim; ++j) RTK_STEP32(1)
    }
#undef RTK_STEP32
    if (STORE == 2 && has_word) { RtkTbHalf hv; hv.pv = Pv; hv.mv = Mv; hv.ph = lastPh; hv.mh = lastMh; reinterpret_cast<RtkTbHalf*>(tb)[w] = hv; } // the last column, as a table of one column
    st.final_score = __builtin_amdgcn_readlane(score, W - 1);
    if (TRACK == 2) rtk_last_column_stat(has_word ? Pv : 0u, has_word ? Mv : 0u, 32, m, n, at, st);
    if (TRACK == 1) { st.best = __builtin_amdgcn_readlane(vbest, W - 1); st.first = __builtin_amdgcn_readlane(vfirst, W - 1); st.last = __builtin_amdgcn_readlane(vlast, W - 1); st.cnt = __builtin_amdgcn_readlane(vcnt, W - 1); }
    return st;
}

// dispatcher: 32-bit words up to 2048 query characters, 64-bit words beyond
template <int STORE, int TRACK>
__device__ __forceinline__ SweepStat rtk_myers_fast_any(const char* __restrict__ qp, int m, const char* __restrict__ tp, int n, int top_h, bool iupac, uint64_t* __restrict__ tb, int at = 0) {
    if (m <= 2048) return rtk_myers_fast32<STORE, TRACK>(qp, m, tp, n, top_h, iupac, tb, at);
    return rtk_myers_fast<STORE, TRACK == 2 ? 1 : 0>(qp, m, tp, n, top_h, iupac, tb, at);
}

// The two sweeps whose simulator stand-ins (rtk_myers_sim.h) go through the generic pass instead. Both decline (plain == false) a target with another byte than A/C/G/T.
// NW sweep of (corr, raw) reduced over its LAST COLUMN (rtk_myers_shw_by_column); store: 0 nothing, 1 the table, 2 the entries of the last column at the table's start
RTK_DEV SweepStat rtk_myers_sweep_column(const MyersScratch& sc, const char* corr, int m, const char* raw, int n, bool iupac, int store, int at) {
    const SweepStat st = store == 2 ? rtk_myers_fast_any<2, 2>(corr, m, raw, n, 1, iupac, rtk_ld(&sc.tb), at)
                       : store ? rtk_myers_fast_any<1, 2>(corr, m, raw, n, 1, iupac, rtk_ld(&sc.tb), at) : rtk_myers_fast_any<0, 2>(corr, m, raw, n, 1, iupac, nullptr, at);
    rtk_sync();
    return st;
}
// stored NW sweep reduced over its LAST ROW (rtk_myers_nw_and_save); *gen = the generation of the table it wrote
RTK_DEV SweepStat rtk_myers_sweep_saved(const MyersScratch& sc, const char* q, int m, const char* t, int n, bool iupac, uint32_t* gen) {
    *gen = rtk_tb_written(sc);
    const SweepStat st = rtk_myers_fast_any<1, 1>(q, m, t, n, 1, iupac, rtk_ld(&sc.tb));
    rtk_sync();
    return st;
}
#endif
#endif
