// What the parts of the Myers aligner hand to each other: the modes, the work area of one wave (MyersScratch) and who uses which of its
// buffers as what, the traceback-table layout, sequences read forwards or backwards, results, and the carve of a work area.
#ifndef RTK_MYERS_TYPES_H
#define RTK_MYERS_TYPES_H
#include "rtk_wave.h"

#define RTK_MODE_NW 0
#define RTK_MODE_SHW 1
#define RTK_MODE_HW 2

// Which routine uses which buffer of the work area as what:
//   buffer      routine                                          holds
//   tb          stored sweeps (rtk_myers_pass store != 0,        the traceback table, 4 words per (column, query word); store == 2: one column of
//               rtk_myers_fast_any STORE != 0), rtk_myers_walk,  it at the table's start
//               rtk_myers_last_move(_column)
//   tb          rtk_myers_distance (banded NW),                  NOT a table: the final vertical delta vectors of the passes, fin .. fin + 2 W (one
//               rtk_myers_alignment, rtk_myers_alignment_lvl     pass) or + 4 W (left and right half pass); the level driver keeps those of a round
//   rowL, rowR  rtk_myers_alignment(_lvl)                        last-column scores of the left / the reversed right half pass (rtk_myers_column)
//   rowL        rtk_myers_distance (banded NW)                   the last column of the pass; only its last row is read
//   hstack      rtk_myers_alignment                              the explicit Hirschberg stack, 5 ints per sub-problem
//   hstack      rtk_myers_alignment_lvl                          the node records of a round, RTK_LVL_NODE ints each (rtk_myers_lvl.h)
//   carry       rtk_myers_pass, rtk_myers_block                  horizontal deltas leaving a row block, one byte per column; the second pass of a
//                                                                shared pair works behind the first one's columns (rtk_myers_pass_coop)
//   colscore    rtk_myers_pass, rtk_myers_block (unbanded)       last-row score of every column; read by rtk_myers_distance and rtk_myers_traceback
//   peq         rtk_myers_build_peq (simulator)                  the profile by character class;
//               rtk_myers_ring, rtk_myers_pass_coop              on the device 4 words (A, C, G, T) per query word, two such tables for a shared pair
//   moves_tmp   rtk_myers_walk                                   the walk's moves, produced backwards from the buffer's end, then copied to moves
// tb_gen counts the writers of tb (rtk_tb_written). Two readers rely on it: rtk_myers_path_from_saved, which resumes a MyersSaved only on the table of its own sweep,
// and the region stage's TrimPark (rtk_region_align.h), which notes the generation of the trim's stored sweep and asserts it before it walks that table later.
struct MyersScratch {
    U<uint64_t*> peq;       // [15 * w_cap]
    U<uint32_t> w_cap;      // max query words
    U<int8_t*> carry;       // [t_cap]
    U<int32_t*> colscore;   // [t_cap] last-row score of every column
    U<uint32_t> t_cap;      // max target columns
    U<uint64_t*> tb;        // [tb_cap_words] traceback table, 4 words per (column, query word): Pv, Mv, Ph, Mh
    U<uint64_t> tb_cap_words;
    U<int32_t*> rowL;       // [r_cap] Hirschberg: D(left half)[row]
    U<int32_t*> rowR;       // [r_cap]
    U<uint32_t> r_cap;
    U<uint8_t*> moves;      // [mv_cap] alignment moves: 0 match, 1 insert (query only), 2 delete (target only), 3 mismatch
    U<uint8_t*> moves_tmp;  // [mv_cap]
    U<uint32_t> mv_cap;
    U<int32_t*> hstack;     // [5 * 64] explicit Hirschberg stack
    UL<uint32_t*> overflow; // (device memory, or the header's own word in LDS) set to non-zero when a capacity is exceeded (work item is re-run with a bigger arena)
    U<uint32_t> tb_gen;     // bumped by everything that writes the traceback table: a saved sweep (MyersSaved) is only resumed on its own table
    U<unsigned long long> walk_cycles, walk_moves, walk_reloads, walk_scalar, walk_calls, walk_tail_cycles; // profile of the traceback walks
    U<unsigned long long> hb_pass, hb_split, hb_leaf, hb_total; // profile of the Hirschberg driver: half passes, column extraction + split search, leaf tracebacks, all
    // Optional, set by a caller around ONE rtk_myers_path call: a bit per target position, bit i set = the caller looks at the moves that happen at target position i
    // (the moves over target character i and the insertions in front of it). A sub-problem of the Hirschberg recursion none of whose target positions t0 .. t0 + tn
    // (both ends) has its bit set is not solved: its moves are written as tn deletions then qm insertions, which carry the only facts such a caller uses -- how many query
    // and target characters the stretch consumes (phasing(), rtk_phasing.h: the walk of src/Graph.cpp:991-1069 copies the corrected read wherever pos2rm has no bit).
    // Everything the split of a level decides (distance, split rows) is computed as always, so the sub-problems that ARE solved are those of the full recursion.
    U<uint64_t*> need_bm; // (NOT a pointer to const: the bitmap is written by the kernel that reads it; a pointer-to-const field is read through the scalar cache, rtk_types.h)
};
// no position of [lo, hi] (both included) has its bit set
RTK_DEV bool rtk_need_none(const uint64_t* bm, int lo, int hi) {
    for (int w = lo >> 6; w <= (hi >> 6); ++w) {
        uint64_t mk = ~0ull;
        if (w == (lo >> 6)) mk &= ~0ull << (lo & 63);
        if (w == (hi >> 6)) mk &= ~0ull >> (63 - (hi & 63));
        if (bm[w] & mk) return false;
    }
    return true;
}
// The traceback table's memory is about to be written (entries, or the delta vectors that the Hirschberg and banded passes keep there): bumps the generation that a
// saved sweep is checked against (MyersSaved::gen) and returns it. The only write through a const MyersScratch&: the generation belongs to the work area.
RTK_DEV uint32_t rtk_tb_written(const MyersScratch& sc) { MyersScratch& msc = const_cast<MyersScratch&>(sc); const uint32_t gen = rtk_ld(&msc.tb_gen) + 1u; msc.tb_gen = gen; return gen; }
// One stored sweep of m query characters over n columns, and the walk of its table, fit this work area: tb_cap_words holds the table (4 words per word and
// column); mv_cap the m + n moves of the longest path, in moves and in moves_tmp (mv_slack: room a caller wants beyond them); t_cap the per-column arrays
// (colscore, carry) of the generic pass that takes over when the target is not plain; w_cap that pass's profile table.
RTK_DEV bool rtk_fits_stored_sweep(const MyersScratch& sc, int m, int n, uint32_t mv_slack = 0u) {
    const long long W = (m + 63) >> 6;
    return static_cast<uint64_t>(4 * W * n) <= sc.tb_cap_words && static_cast<uint32_t>(m + n) + mv_slack <= sc.mv_cap && static_cast<uint32_t>(n) <= sc.t_cap && static_cast<uint32_t>(W) <= sc.w_cap;
}

// traceback table entry of (column, 64-bit query word): word-major, so that the walk's window of 64 consecutive columns of one word is
// one contiguous 2 KB run (16 cache lines) instead of 64 entries a table row apart. `ncols` = number of columns of the sweep that stored it.
#define RTK_TB(col, w, ncols) (static_cast<uint64_t>(w) * static_cast<uint64_t>(ncols) + static_cast<uint64_t>(col))
// An entry is 32 bytes: the low 32-bit halves of {Pv, Mv, Ph, Mh}, then their high halves, so that each of the two lanes that share a
// 64-bit word in the 32-bit sweep writes its four words with ONE 16-byte store.
struct RtkTbHalf { uint32_t pv, mv, ph, mh; };
RTK_DEV void rtk_tb_put(uint64_t* e, uint64_t Pv, uint64_t Mv, uint64_t Ph, uint64_t Mh) {
    RtkTbHalf lo, hi;
    lo.pv = static_cast<uint32_t>(Pv); lo.mv = static_cast<uint32_t>(Mv); lo.ph = static_cast<uint32_t>(Ph); lo.mh = static_cast<uint32_t>(Mh);
    hi.pv = static_cast<uint32_t>(Pv >> 32); hi.mv = static_cast<uint32_t>(Mv >> 32); hi.ph = static_cast<uint32_t>(Ph >> 32); hi.mh = static_cast<uint32_t>(Mh >> 32);
    reinterpret_cast<RtkTbHalf*>(e)[0] = lo; reinterpret_cast<RtkTbHalf*>(e)[1] = hi;
}
RTK_DEV void rtk_tb_get(const uint64_t* e, uint64_t& Pv, uint64_t& Mv, uint64_t& Ph, uint64_t& Mh) {
    const RtkTbHalf lo = reinterpret_cast<const RtkTbHalf*>(e)[0], hi = reinterpret_cast<const RtkTbHalf*>(e)[1];
    Pv = static_cast<uint64_t>(lo.pv) | (static_cast<uint64_t>(hi.pv) << 32); Mv = static_cast<uint64_t>(lo.mv) | (static_cast<uint64_t>(hi.mv) << 32);
    Ph = static_cast<uint64_t>(lo.ph) | (static_cast<uint64_t>(hi.ph) << 32); Mh = static_cast<uint64_t>(lo.mh) | (static_cast<uint64_t>(hi.mh) << 32);
}
// The traceback's step out of ONE cell (i, j) with score cur, preferring up (insert, 1) > left (delete, 2) > diagonal (match 0 / mismatch 3; edlib.cpp:1021-1137):
// a0 .. a3 = Pv, Mv, Ph, Mh of the entry of (column c = j - 1, word of row i - 1), b = the row's bit in it, l0 / l1 = Pv / Mv of the entry one column to the
// left (not looked at when c == 0). Moves i, j and cur to the cell the path came from and returns the move. Both builds of rtk_myers_walk step through it.
RTK_DEV uint8_t rtk_walk_cell(uint64_t a0, uint64_t a1, uint64_t a2, uint64_t a3, uint64_t l0, uint64_t l1, int b, int c, int& i, int& j, int& cur) {
    const int vd = static_cast<int>((a0 >> b) & 1ull) - static_cast<int>((a1 >> b) & 1ull);
    const int hd = static_cast<int>((a2 >> b) & 1ull) - static_cast<int>((a3 >> b) & 1ull);
    uint8_t mv;
    if (vd == 1) { mv = 1; --i; cur -= 1; }
    else if (hd == 1) { mv = 2; --j; cur -= 1; }
    else {
        const int left = cur - hd;
        int diag;
        if (c == 0) diag = i - 1;
        else diag = left - (static_cast<int>((l0 >> b) & 1ull) - static_cast<int>((l1 >> b) & 1ull));
        mv = (diag == cur) ? 0 : 3;
        --i; --j; cur = diag;
    }
    return mv;
}

struct MySeq { // a character sequence read forwards or backwards (Hirschberg aligns reversed halves, edlib.cpp:1259-1263)
    const char* p; int32_t n; int32_t rev;
};
RTK_DEV MySeq rtk_seq(const char* p, int32_t n, int32_t rev = 0) { MySeq s; s.p = p; s.n = n; s.rev = rev; return s; }
RTK_DEV unsigned char rtk_seq_at(const MySeq& s, int32_t i) { return static_cast<unsigned char>(s.rev ? s.p[s.n - 1 - i] : s.p[i]); }

struct MyersResult { int32_t dist, first, last, nloc; };
struct SweepStat { int final_score, best, first, last, cnt; bool plain; int at_score; };
struct MyersSaved { uint32_t valid, gen; int32_t m, n, nw_dist; MyersResult shw; uint8_t* stash; uint32_t stash_cap, stash_n; }; // stash (set by the caller, may be null): room for the moves of the alignment, kept from the sweep on (LDS-table route: the table does not outlive the call)
// one problem of the stage entry rtk_myers_batch (offsets into one character pool)
struct MyersProb { uint64_t q_off, t_off; uint32_t qlen, tlen; int32_t k, mode; };

// ------------------------------------------------------------------------------------------------ work area of one wave
struct ScratchCfg { uint32_t w_cap, t_cap, r_cap, mv_cap; uint64_t tb_cap_words; };

// edlib traces back in memory -- one stored sweep and a walk -- when the table is under 1 MiB by its own count, and splits the problem (Hirschberg) otherwise:
// (2 * sizeof(Word) + sizeof(int)) bytes per block and column plus 8 per column (edlib.cpp:1191-1193), for m query and n target characters. Every route that
// stands in for that branch asks here, so that the same problems are walked and split as in the reference.
#define RTK_TB_IN_MEMORY_BYTES (1024 * 1024)
RTK_HD constexpr bool rtk_tb_in_memory(int m, long long n) { return (2LL * 8 + 4) * ((m + 63) >> 6) * n + 8LL * n < RTK_TB_IN_MEMORY_BYTES; }

// Work area of a helper wave for the leaf tracebacks of a multi-wave alignment: whatever passes rtk_tb_in_memory with one row block (W <= 64 words) fits it.
#define RTK_LEAF_WAVES 8 // waves of a workgroup that take part in leaf rounds (the program wave + 7 helpers with a work area each)
#define RTK_LEAF_CELLS 52429  // W * n stays below it: 20 W n < 1 MiB
#define RTK_LEAF_T_MAX 37449  // the longest target: one query word, 28 n < 1 MiB
#define RTK_LEAF_T_CAP 37504  // ... in whole 64-byte lines
#define RTK_LEAF_MV_CAP 53248 // m + n moves and the 64 of slack rtk_fits_stored_sweep asks for: at most 4096 + RTK_LEAF_T_MAX + 64; RTK_LEAF_CELLS + 64 in whole KiB
static_assert(20LL * RTK_LEAF_CELLS >= RTK_TB_IN_MEMORY_BYTES && 20LL * (RTK_LEAF_CELLS - 1) < RTK_TB_IN_MEMORY_BYTES, "RTK_LEAF_CELLS");
static_assert(rtk_tb_in_memory(1, RTK_LEAF_T_MAX) && !rtk_tb_in_memory(1, RTK_LEAF_T_MAX + 1), "RTK_LEAF_T_MAX");
static_assert(RTK_LEAF_T_CAP == (RTK_LEAF_T_MAX + 63) / 64 * 64, "RTK_LEAF_T_CAP");
static_assert(RTK_LEAF_MV_CAP == (RTK_LEAF_CELLS + 64 + 1023) / 1024 * 1024 && RTK_LEAF_MV_CAP >= 64 * 64 + RTK_LEAF_T_MAX + 64, "RTK_LEAF_MV_CAP");
RTK_HD ScratchCfg rtk_leaf_cfg() { ScratchCfg c; c.w_cap = 64; c.t_cap = RTK_LEAF_T_CAP; c.r_cap = 64; c.mv_cap = RTK_LEAF_MV_CAP; c.tb_cap_words = 4ull * RTK_LEAF_CELLS + 64; return c; }
RTK_HD uint64_t scratch_bytes(const ScratchCfg& c) {
    uint64_t b = 0;
    b += 8ull * 15 * c.w_cap; b += (c.t_cap + 63) / 64 * 64; b += 4ull * c.t_cap; b += 8ull * c.tb_cap_words; b += 8ull * c.r_cap;
    b += 2ull * ((c.mv_cap + 63) / 64 * 64); b += 4 * 5 * 64; b += 64;
    return (b + 255) / 256 * 256;
}

RTK_HD MyersScratch scratch_carve(char* base, const ScratchCfg& c) {
    MyersScratch s; char* p = base;
    s.peq = reinterpret_cast<uint64_t*>(p); p += 8ull * 15 * c.w_cap; s.w_cap = c.w_cap;
    s.tb = reinterpret_cast<uint64_t*>(p); p += 8ull * c.tb_cap_words; s.tb_cap_words = c.tb_cap_words;
    s.colscore = reinterpret_cast<int32_t*>(p); p += 4ull * c.t_cap; s.t_cap = c.t_cap;
    s.rowL = reinterpret_cast<int32_t*>(p); p += 4ull * c.r_cap; s.rowR = reinterpret_cast<int32_t*>(p); p += 4ull * c.r_cap; s.r_cap = c.r_cap;
    s.hstack = reinterpret_cast<int32_t*>(p); p += 4 * 5 * 64;
    s.overflow = reinterpret_cast<uint32_t*>(p); p += 64;
    s.tb_gen = 0;
    s.walk_cycles = 0; s.walk_moves = 0; s.walk_reloads = 0; s.walk_scalar = 0; s.walk_calls = 0; s.walk_tail_cycles = 0;
    s.hb_pass = 0; s.hb_split = 0; s.hb_leaf = 0; s.hb_total = 0; s.need_bm = nullptr;
    s.carry = reinterpret_cast<int8_t*>(p); p += (c.t_cap + 63) / 64 * 64;
    s.moves = reinterpret_cast<uint8_t*>(p); p += (c.mv_cap + 63) / 64 * 64; s.moves_tmp = reinterpret_cast<uint8_t*>(p); s.mv_cap = c.mv_cap;
    return s;
}
#endif
