// The traceback over a stored table: the walk, the last move alone, and sweep + walk of one in-memory problem.
#ifndef RTK_MYERS_WALK_H
#define RTK_MYERS_WALK_H
#include "rtk_myers_pass.h"
#include "rtk_myers_sim.h"

// Canonical NW traceback over the stored table, preferring up (insert) > left (delete) > diagonal
// (edlib.cpp:1021-1137). Appends the moves (already in forward order) to sc.moves at *n_moves.
// Walks the stored table from cell (m, n) back to the origin; `cur` = D[m][n]. Appends the moves to sc.moves (after *n_moves).
// The simulator's walk (rtk_myers_sim.h) makes every move with rtk_walk_cell; this one takes whole runs of moves and falls back to the same step.
#ifndef RTK_SIM
RTK_FN void rtk_myers_walk(const MyersScratch& sc_, int m_, int n_, int ncols_, int cur_, uint32_t* n_moves_) { // ncols: columns of the sweep that stored the table (>= n)
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); uint32_t* n_moves = rtk_u(n_moves_);
    const int m = rtk_u(m_), n = rtk_u(n_), ncols = rtk_u(ncols_);
    int cur = rtk_u(cur_);
    const unsigned long long tw0 = rtk_clock(); unsigned n_rel = 0, n_sc = 0;
    int i = m, j = n;
    uint32_t nt = 0; // moves are produced backwards into moves_tmp, from its end
    uint8_t* tmp = rtk_ld(&sc.moves_tmp);
    const uint32_t cap = rtk_ld(&sc.mv_cap);
    uint64_t* const tbp = rtk_ld(&sc.tb);
    // The wave keeps, for the current query word, the four delta words of 64 consecutive columns in registers
    // (lane l <-> column c_hi - l); a traceback step is then scalar (v_readlane), with one table reload per ~60 moves.
    const int lane = rtk_lane();
    int w_cur = -1, c_hi = -1;
    uint64_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
#define RTK_RL64(v, l) ((static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>((v) >> 32), (l)))) << 32) | static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>((v) & 0xFFFFFFFFull), (l))))
    while (i > 0 && j > 0) {
        const int r = i - 1, c = j - 1, w = r >> 6, b = r & 63;
        if (w != w_cur || c > c_hi || c_hi - c > 62) {
            c_hi = c; w_cur = w; ++n_rel;
            const int col = c - lane;
            if (col >= 0) rtk_tb_get(tbp + 4ull * RTK_TB(col, w, ncols), e0, e1, e2, e3);
        }
        const int li = c_hi - c;
        { // run of inserts (moves up column c): consecutive rows from r downwards whose vertical delta is +1 = ones of Pv & ~Mv below bit b
            const uint64_t up = RTK_RL64(e0, li) & ~RTK_RL64(e1, li);
            if ((up >> b) & 1ull) {
                const uint64_t nup = ~(up << (63 - b));
                const int run = nup ? __builtin_clzll(nup) : 64; // >= 1, stays inside this 64-row word
                if (lane < run) tmp[cap - (nt + 1u + static_cast<uint32_t>(lane))] = 1;
                i -= run; cur -= run; nt += static_cast<uint32_t>(run);
                continue;
            }
        }
        { // run of deletes (moves left along row r): leading columns whose cell has no +1 vertical delta but a +1 horizontal one
            const int l = lane - li;
            const int vd_ = static_cast<int>((e0 >> b) & 1ull) - static_cast<int>((e1 >> b) & 1ull);
            const int hd_ = static_cast<int>((e2 >> b) & 1ull) - static_cast<int>((e3 >> b) & 1ull);
            const bool isleft = l >= 0 && (c - l) >= 0 && vd_ != 1 && hd_ == 1;
            const uint64_t nleft = ~(rtk_ballot(isleft) >> li);
            const int run = nleft ? __builtin_ctzll(nleft) : 64;
            if (run > 0) {
                if (l >= 0 && l < run) tmp[cap - (nt + 1u + static_cast<uint32_t>(l))] = 2;
                j -= run; cur -= run; nt += static_cast<uint32_t>(run);
                continue;
            }
        }
        { // Runs of diagonal moves, up to 62 at a time: the move out of a cell only depends on the deltas stored around it, so the lane
          // holding column c - l looks at cell (r - l, c - l) of the diagonal through (r, c); the leading lanes that see neither an
          // insert nor a delete form one run of match / mismatch moves, written out together.
            const int l = lane - li;
            const int rl = r - l;
            const bool valid = l >= 0 && lane <= 62 && rl >= 64 * w && (c - l) >= 1;
            const int bb = rl & 63, bn = (bb + 1) & 63;
            const int vd_ = static_cast<int>((e0 >> bb) & 1ull) - static_cast<int>((e1 >> bb) & 1ull);
            const int hd_ = static_cast<int>((e2 >> bb) & 1ull) - static_cast<int>((e3 >> bb) & 1ull);
            const int vdn = static_cast<int>((e0 >> bn) & 1ull) - static_cast<int>((e1 >> bn) & 1ull); // my column, one row further down: what lane - 1 needs
            const int vdl = __shfl_down(vdn, 1, 64);
            const bool isdiag = valid && vd_ != 1 && hd_ != 1;
            const uint64_t dm = rtk_ballot(isdiag) >> li;
            const uint64_t ndm = ~dm;
            const int run = ndm ? __builtin_ctzll(ndm) : 64;
            if (run > 0) {
                const bool mine = l >= 0 && l < run;
                const bool mism = (hd_ + vdl) != 0;
                const uint64_t mm = rtk_ballot(mine && mism);
                if (mine) tmp[cap - (nt + 1u + static_cast<uint32_t>(l))] = mism ? 3 : 0;
                cur -= rtk_popc(mm); i -= run; j -= run; nt += static_cast<uint32_t>(run);
                continue;
            }
        }
        ++n_sc;
        const uint64_t a0 = RTK_RL64(e0, li), a1 = RTK_RL64(e1, li), a2 = RTK_RL64(e2, li), a3 = RTK_RL64(e3, li);
        const uint64_t l0 = RTK_RL64(e0, li + 1), l1 = RTK_RL64(e1, li + 1); // column c-1 (unused when c == 0)
        const uint8_t mv = rtk_walk_cell(a0, a1, a2, a3, l0, l1, b, c, i, j, cur);
        ++nt; tmp[cap - nt] = mv;
    }
#undef RTK_RL64
    const unsigned long long tw1 = rtk_clock();
    // whatever is left is a run of inserts (query only) or deletes (target only)
    if (i > 0) { rtk_wfill(tmp + (cap - nt - static_cast<uint32_t>(i)), 1, static_cast<uint64_t>(i)); nt += static_cast<uint32_t>(i); i = 0; }
    if (j > 0) { rtk_wfill(tmp + (cap - nt - static_cast<uint32_t>(j)), 2, static_cast<uint64_t>(j)); nt += static_cast<uint32_t>(j); j = 0; }
    rtk_sync(); // runs were written by their lanes
    rtk_wcopy(rtk_ld(&sc.moves) + *n_moves, tmp + (cap - nt), nt);
    *n_moves += nt;
    { MyersScratch& msc = const_cast<MyersScratch&>(sc); msc.walk_cycles += rtk_clock() - tw0; msc.walk_moves += nt; msc.walk_reloads += n_rel; msc.walk_scalar += n_sc; msc.walk_calls += 1; msc.walk_tail_cycles += rtk_clock() - tw1; }
}
#endif

// The LAST move of the path rtk_myers_walk(sc, m, n, ncols, cur, ...) would append (m, n >= 1): the walk produces its moves backwards, so that is its first
// step, out of cell (m, n) -- one look at the two table entries around that cell with the walk's own preferences (insert > delete > diagonal; a diagonal
// is a match, 0, when it keeps the score and a mismatch, 3, when it does not). Nothing is walked and sc.moves is not touched. Wave-uniform: every lane
// reads the same two entries, of word (m - 1) / 64 whatever the word count of the table.
RTK_DEV uint8_t rtk_myers_last_move(const MyersScratch& sc_, int m_, int n_, int ncols_, int cur_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    const int m = rtk_u(m_), n = rtk_u(n_), ncols = rtk_u(ncols_), cur = rtk_u(cur_);
    const uint64_t* const tbp = rtk_ld(&sc.tb);
    const int r = m - 1, c = n - 1, w = r >> 6, b = r & 63;
    uint64_t a0, a1, a2, a3; rtk_tb_get(tbp + 4ull * RTK_TB(c, w, ncols), a0, a1, a2, a3);
    if (static_cast<int>((a0 >> b) & 1ull) - static_cast<int>((a1 >> b) & 1ull) == 1) return 1; // vertical delta +1: up
    const int hd = static_cast<int>((a2 >> b) & 1ull) - static_cast<int>((a3 >> b) & 1ull);
    if (hd == 1) return 2; // horizontal delta +1: left
    int diag = m - 1; // column 0: D[m - 1][0]
    if (c > 0) { uint64_t l0, l1, l2, l3; rtk_tb_get(tbp + 4ull * RTK_TB(c - 1, w, ncols), l0, l1, l2, l3); diag = cur - hd - (static_cast<int>((l0 >> b) & 1ull) - static_cast<int>((l1 >> b) & 1ull)); }
    return (diag == cur) ? 0 : 3;
}

// The same move from the LAST COLUMN alone, as a sweep with store = 2 leaves it (rtk_myers_shw_by_column: entry w at the start of the table holds Pv, Mv, Ph, Mh
// of word w at column n - 1): the last move of the NW path of (query[0, m), target). The
// vertical delta of cell (m, n) is bit m - 1 of Pv / Mv, its horizontal delta the same bit of Ph / Mh; the diagonal neighbour is reached over the cell above,
// D[m - 1][n - 1] = D[m][n] - vertical delta - horizontal delta of row m - 1, and that delta is bit m - 2 of Ph / Mh (the word before when m - 1 is the first
// row of its word; +1 in the matrix's row 0). Same preferences, same values as rtk_myers_last_move. Wave-uniform; one entry read, two at a word boundary.
RTK_DEV uint8_t rtk_myers_last_move_column(const MyersScratch& sc_, int m_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc);
    const int m = rtk_u(m_);
    const uint64_t* const tbp = rtk_ld(&sc.tb);
    const int r = m - 1, w = r >> 6, b = r & 63;
    uint64_t a0, a1, a2, a3; rtk_tb_get(tbp + 4ull * static_cast<uint64_t>(w), a0, a1, a2, a3);
    const int vd = static_cast<int>((a0 >> b) & 1ull) - static_cast<int>((a1 >> b) & 1ull);
    if (vd == 1) return 1; // up
    if (static_cast<int>((a2 >> b) & 1ull) - static_cast<int>((a3 >> b) & 1ull) == 1) return 2; // left
    int hu = 1; // row 0 of the matrix: D[0][n] - D[0][n - 1]
    if (b > 0) hu = static_cast<int>((a2 >> (b - 1)) & 1ull) - static_cast<int>((a3 >> (b - 1)) & 1ull);
    else if (w > 0) { uint64_t u0, u1, u2, u3; rtk_tb_get(tbp + 4ull * static_cast<uint64_t>(w - 1), u0, u1, u2, u3); hu = static_cast<int>((u2 >> 63) & 1ull) - static_cast<int>((u3 >> 63) & 1ull); }
    return (vd + hu == 0) ? 0 : 3; // diagonal neighbour D[m - 1][n - 1] = D[m][n] - vd - hu: a match keeps the score
}

RTK_FN void rtk_myers_traceback(const MyersScratch& sc_, MySeq q_, MySeq t_, bool iupac_, uint32_t* n_moves_) {
    const MyersScratch& sc = *rtk_u(&sc_); RTK_ASSUME_LDS(&sc); uint32_t* n_moves = rtk_u(n_moves_); const bool iupac = rtk_u(iupac_);
    MySeq q, t; q.p = rtk_u(q_.p); q.n = rtk_u(q_.n); q.rev = rtk_u(q_.rev); t.p = rtk_u(t_.p); t.n = rtk_u(t_.n); t.rev = rtk_u(t_.rev);
    const int m = q.n, n = t.n;
    int cur;
    SweepStat fst; fst.plain = false;
    if (m <= 4096 && !q.rev && !t.rev) fst = rtk_myers_fast_any<1, 0>(q.p, m, t.p, n, 1, iupac, rtk_ld(&sc.tb)); // (the simulator's declines)
    if (fst.plain) { cur = fst.final_score; rtk_sync(); }
    else
    { rtk_myers_pass(sc, q, t, 1, iupac, 1, nullptr, nullptr); cur = rtk_ld(rtk_ld(&sc.colscore) + (n - 1)); }
    rtk_myers_walk(sc, m, n, n, cur, n_moves);
}
#endif
