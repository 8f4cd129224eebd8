// What every stage of the per-read correction reads its batch through: the options and the batch as the device sees them (OptsView, BatchView), the work area
// of a wave of the per-read seed programs (SeedScratch) and a wave's slice of the raw-hit pool (PoolChunk).
#ifndef RTK_SEED_TYPES_H
#define RTK_SEED_TYPES_H

#include "rtk_types.h"
#include "rtk_wave.h"

struct OptsView {
    U<uint32_t> insert_sz, min_cov_vertices, max_len_weak_region1, max_km_cov;
    U<double> weak_region_len_factor, large_k_factor, min_score;
    U<int32_t> max_qual, out_qual;
    U<double> min_confidence_snp_corr;
    // second pass (`correct -2`, long_read_correct in the reference): qualities of pass 1 are carried over, no 1-edit search
    U<int32_t> long_read_correct;
    U<uint32_t> max_len_weak_region2;
    U<uint32_t> d1_desc; // [D1] switch (rtk_opts::d1_desc): anchors of equal colour-set cardinality by unitig id, 0 ascending, 1 descending
    U<uint32_t> a3_strand_order; // [A3] switch (rtk_opts::a3_strand_order): 1 = neighbours of a reverse-strand end visited in the order of the unitig's own strand
    U<uint32_t> a2_exclusive; // [A2] switch (rtk_opts::a2_exclusive): 0 = union; 1, 2 = a window matched by one kind of edit is not searched with the next kind (1: substitution, insertion, deletion; 2: insertion, deletion, substitution)
    U<uint32_t> fa_linked_always; // RTK_FA_LINKED_ALWAYS (rtk_knobs.h): 1 = rtk_fix_ambiguity runs every linked-allele search, also those that cannot append (parity test, A/B traces)
    U<uint32_t> strand2_mode; // RTK_STRAND2_ALWAYS / RTK_STRAND2_AUDIT (rtk_knobs.h): 0 = a gap region whose forward result decides the bytes skips its second strand (rtk_strand2_skippable, rtk_region.h), 1 = every second strand runs, 2 = they run where the rule says skip, and the two results are compared
    U<uint32_t> colours_mode; // RTK_COLOURS_ROUTE / RTK_COLOURS_AUDIT / RTK_TEST_COLOURS_FAULT (rtk_knobs.h): RTK_CM_* (rtk_types.h). 0 = rtk_choose_colors (rtk_colours.h) asks its programs in their usual order and nothing is compared
    U<uint32_t> park_eager; // RTK_PARK_EAGER (rtk_knobs.h): 1 = the forward trim of a gap region walks its alignment at once (rtk_trim_by_column, rtk_region_align.h), 0 = only where a consensus is going to run
    U<uint32_t> inexact_route; // RTK_INEXACT_SHARED / RTK_INEXACT_PLANES (rtk_knobs.h): RTK_IR_* bits, 0 = rtk_inexact_tile_seeded looks every read position of a tile up once and builds the window codes from bit planes; a set bit takes that part's old route
    U<uint32_t> trim_store; // RTK_TRIM_STORE (rtk_knobs.h): 1 = the forward trim of a gap region stores the table of its sweep (rtk_trim_by_column, rtk_region_align.h), 0 = it keeps the last column alone
};

struct BatchView {
    U<uint32_t> n_reads;
    U<uint64_t> n_bases;
    U<const char*> seq;          // upper-cased reads, concatenated
    U<const char*> qual;         // pass 2: the reads' quality strings (same offsets as seq); null in pass 1, which writes its own
    U<const uint64_t*> roff;     // [n_reads+1]
    U<const uint32_t*> order;    // [n_reads] read indices, longest first (per-read kernels start their longest items first)
    U<uint64_t*> hits;           // [n_bases] exact hit of the window starting at each base (packed, RTK_NO_HIT if none)
    U<uint64_t*> hitmap;         // [n_bases/64 + 2] bit b&63 of word b>>6: window b has an exact hit
    U<char*> masked;             // [n_bases] the 'N'-masked copy searched inexactly (src/Graph.cpp:102)
    U<uint64_t*> wdesc;          // [n_bases] group of raw inexact hits of the window: pool offset << 24 | count
    U<uint64_t*> ipool;          // raw inexact hits {k-mer code in read orientation, packed hit}
    U<uint64_t> ipool_cap;       // entries
    U<unsigned long long*> ipool_top;
    U<uint32_t*> s_pos;          // solid anchor positions of read r at [roff[r], roff[r] + n_solid[r])
    U<uint32_t*> n_solid;        // [n_reads]
    U<uint32_t*> wk_pos;         // weak anchors (all reads), read r at [w_off[r], w_off[r] + w_cnt[r])
    U<uint64_t*> wk_hit;
    U<uint64_t> wk_cap;
    U<unsigned long long*> wk_top;
    U<uint64_t*> w_off;          // [n_reads]
    U<uint32_t*> w_cnt;          // [n_reads]
    U<uint32_t*> status;         // [n_reads] non-zero: a scratch capacity was exceeded for this read
    U<unsigned long long*> counters; // [RTK_CNT_TOTAL] event and cycle counters: the map is RtkCounterSlot (rtk_types.h)
};

// The work area of one wave of k_mask / k_finalize. k_mask uses set[0 .. 3] (the running unions of rtk_union_unitig and the parked left union) and `overflow` alone.
// rtk_finalize_read (rtk_seed_finalize.h) uses every other buffer, several of them twice; a phase receives a buffer under the name of its role:
//   buffer                        phase              as                                                              until
//   sflag                         junction           emptied: 1 = solid candidate i is dropped                        the phase ends
//   vkey                          junction           jl: the junction list, 2 v_cap + 512 entries                     the phase ends
//   vpos, vcode, vhit             gather             the weak hits of the read: position, k-mer code, packed hit      vcode: classify+sort ends; vpos, vhit: write
//   vkey, vidx                    gather             skey, sval: the raw hits of ONE window with more than 64, sorted   that window is done
//   vflag                         classify+sort      cleared; conflicts sets 1 = the hit is kept                      write
//   vkey, vidx                    classify+sort      skey, sidx: key and hit index of the classified hits, sorted     conflicts ends
//   gstart, gcnt, gps, gpe        classify+sort      Ka, Ia, Kb, Ib: 32-bit keys / indices of the radix sort          the phase ends
//   gstart, gcnt, gps, gpe, gkeep groups             per group: first sorted index, size, position span, 1 = kept     conflicts ends
//   vcode                         groups             ginfo: per group, its variant's position and first hit's unitig  conflicts ends
//   overflow                      gather, write      *overflow = 1: a capacity of the work area or of the weak pool was exceeded
struct SeedScratch {
    U<uint32_t*> set[6]; U<uint32_t> set_cap;           // sorted-id buffers
    U<uint32_t*> vpos; U<uint64_t*> vcode; U<uint64_t*> vhit; U<uint64_t*> vkey; U<uint64_t*> vidx; U<uint32_t> v_cap; // weak-hit work lists (vkey/vidx hold 2*v_cap)
    U<uint32_t*> gstart; U<uint32_t*> gcnt; U<uint32_t*> gps; U<uint32_t*> gpe; U<uint8_t*> gkeep; U<uint8_t*> vflag; // variant groups
    U<uint8_t*> sflag;                               // per solid candidate
    U<uint32_t*> overflow;
};


struct SeedScratchCfg { uint32_t set_cap, v_cap, s_cap; };

RTK_HD uint64_t seed_scratch_bytes(const SeedScratchCfg& c) {
    uint64_t b = 0;
    b += 6ull * 4 * c.set_cap;                    // set[6]
    b += 4ull * c.v_cap + 8ull * c.v_cap * 2;     // vpos, vcode, vhit
    b += 2ull * 8 * (2ull * c.v_cap + 512);       // vkey, vidx (padded to a power of two for the sort)
    b += 4ull * 4 * c.v_cap + 2ull * c.v_cap;     // gstart, gcnt, gps, gpe, gkeep, vflag
    b += c.s_cap; b += 64;
    return (b + 255) / 256 * 256;
}

RTK_HD SeedScratch seed_scratch_carve(char* base, const SeedScratchCfg& c) {
    SeedScratch s; char* p = base;
    s.vcode = reinterpret_cast<uint64_t*>(p); p += 8ull * c.v_cap;
    s.vhit = reinterpret_cast<uint64_t*>(p); p += 8ull * c.v_cap;
    s.vkey = reinterpret_cast<uint64_t*>(p); p += 8ull * (2ull * c.v_cap + 512);
    s.vidx = reinterpret_cast<uint64_t*>(p); p += 8ull * (2ull * c.v_cap + 512);
    for (int i = 0; i < 6; ++i) { s.set[i] = reinterpret_cast<uint32_t*>(p); p += 4ull * c.set_cap; }
    s.set_cap = c.set_cap;
    s.vpos = reinterpret_cast<uint32_t*>(p); p += 4ull * c.v_cap; s.v_cap = c.v_cap;
    s.gstart = reinterpret_cast<uint32_t*>(p); p += 4ull * c.v_cap; s.gcnt = reinterpret_cast<uint32_t*>(p); p += 4ull * c.v_cap;
    s.gps = reinterpret_cast<uint32_t*>(p); p += 4ull * c.v_cap; s.gpe = reinterpret_cast<uint32_t*>(p); p += 4ull * c.v_cap;
    s.overflow = reinterpret_cast<uint32_t*>(p); p += 64;
    s.gkeep = reinterpret_cast<uint8_t*>(p); p += c.v_cap; s.vflag = reinterpret_cast<uint8_t*>(p); p += c.v_cap;
    s.sflag = reinterpret_cast<uint8_t*>(p);
    return s;
}

struct PoolChunk { unsigned long long base; uint32_t left; }; // wave-private slice of the raw-hit pool (one device atomic per 4096 entries)
#define RTK_POOL_CHUNK 4096u

#endif
