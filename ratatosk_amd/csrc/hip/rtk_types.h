// POD views shared by the host loader, the HIP kernels and the C-ABI layer.
//
// Flat, read-only image of the compacted coloured de Bruijn graph as it lives in HBM (SoA / CSR):
// everything the reference reaches through Bifrost's CompactedDBG<UnitigData> on the hot path
// (reference: src/UnitigData.hpp:258-491, src/SharedPairID.cpp, Bifrost find()/getSuccessors()).
#ifndef RTK_TYPES_H
#define RTK_TYPES_H

#include <stdint.h>

#if defined(__HIPCC__) && !defined(RTK_SIM)
#include <hip/hip_runtime.h>
#define RTK_HD __host__ __device__ __forceinline__
#else
#define RTK_HD inline
#endif

// ---- wave-uniform values -------------------------------------------------------------------------------------------------
// rtk_u(v): "v is the same in every lane". Identity on the value; on the device it moves the value to scalar registers, so that
// the wave-level programs keep their control state, pointers and loop counters in SGPRs (scalar ALU and branches, spills into
// VGPR lanes instead of 64-wide stores to the stack). Only ever applied to values that are wave-uniform by construction.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RTK_SIM)
template <class T> __device__ __forceinline__ T rtk_u(T v) {
    static_assert(sizeof(T) <= 8, "rtk_u: scalar types only");
    if (sizeof(T) <= 4) {
        uint32_t x = 0; __builtin_memcpy(&x, &v, sizeof(T));
        x = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)));
        T r; __builtin_memcpy(&r, &x, sizeof(T)); return r;
    } else {
        uint64_t x = 0; __builtin_memcpy(&x, &v, sizeof(T));
        const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x & 0xFFFFFFFFull)));
        const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x >> 32)));
        x = (static_cast<uint64_t>(hi) << 32) | lo;
        T r; __builtin_memcpy(&r, &x, sizeof(T)); return r;
    }
}
#else
template <class T> RTK_HD T rtk_u(T v) { return v; }
#endif

// rtk_gp(p): "p points into device (global) memory" -- never into LDS or the wave's private stack. Pointers that the wave programs read from
// their descriptors are generic to the compiler (they come out of LDS or out of structs), and a generic access is a FLAT instruction: it takes the
// LDS address path as well as the memory path, counts in both wait counters (so that a wait for an LDS read also waits for it) and computes its
// 64-bit address per lane. With the address space known the same access is a GLOBAL instruction (scalar base + lane offset, memory counter only).
// Applied to every pointer FIELD of the views and work-area descriptors (U<T*>); the few fields that may point into LDS are UL<T*> below.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RTK_SIM) && !defined(RTK_NO_GLOBAL_PTRS)
template <class T> __device__ __forceinline__ T rtk_gp(T v) { return v; }
// (through an integer: a generic -> global -> generic pointer cast is folded away, and an assumption about the address space is not picked up)
template <class T> __device__ __forceinline__ T* rtk_gp(T* p) { return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)(p); }
// A pointer-to-const FIELD of a view (the graph's arrays, the reads, the anchors of the seed stage: everything a kernel is handed as input) points to
// memory that no running kernel writes: the CONSTANT address space. An access through it with a wave-uniform address -- and most of the wave programs'
// reads of the graph are that: neighbour slots, flag words, offsets of ONE unitig -- becomes a SCALAR load (s_load: scalar cache, no vector-memory
// instruction, the value lands in SGPRs), with a per-lane address it stays a global load.
// RULE: a pointer-to-const field must never point to memory the same launch writes (the scalar cache is not coherent with the vector stores of the wave: a read may return
// what was there before). A bitmap, list or string a wave program builds and then reads is held in a pointer to NON-const (MyersScratch::need_bm is the case that went wrong).
#ifndef RTK_NO_CONST_PTRS
template <class T> __device__ __forceinline__ const T* rtk_gp(const T* p) { return (const T*)(__attribute__((address_space(4))) const T*)(unsigned long long)(p); }
#endif
#else
template <class T> RTK_HD T rtk_gp(T v) { return v; }
#endif

// U<T>: a struct field that holds a wave-uniform value (all the view / scratch descriptors below are per wave or per launch).
// Reads go through rtk_u, so every use site gets the scalar form without being written differently. Same layout as T.
template <class T> struct U {
    T v;
    RTK_HD operator T() const { return rtk_gp(rtk_u(v)); }
    RTK_HD T get() const { return rtk_gp(rtk_u(v)); }
    RTK_HD U& operator=(T x) { v = x; return *this; }
    template <class X> RTK_HD U& operator+=(X x) { v = static_cast<T>(rtk_u(v) + x); return *this; }
    template <class X> RTK_HD U& operator-=(X x) { v = static_cast<T>(rtk_u(v) - x); return *this; }
    template <class X> RTK_HD U& operator*=(X x) { v = static_cast<T>(rtk_u(v) * x); return *this; }
    template <class X> RTK_HD U& operator|=(X x) { v = static_cast<T>(rtk_u(v) | x); return *this; }
    RTK_HD U& operator++() { v = rtk_u(v) + 1; return *this; }
    RTK_HD U& operator--() { v = rtk_u(v) - 1; return *this; }
    RTK_HD T operator++(int) { const T o = rtk_u(v); v = o + 1; return o; }
    RTK_HD T operator--(int) { const T o = rtk_u(v); v = o - 1; return o; }
    RTK_HD T operator->() const { return rtk_gp(rtk_u(v)); }
    RTK_HD decltype(auto) operator*() const { return *rtk_gp(rtk_u(v)); }
    template <class I> RTK_HD decltype(auto) operator[](I i) const { return rtk_gp(rtk_u(v))[i]; }
};
// UL<T*>: a wave-uniform pointer field that may point into LDS (the work-area header of the region kernels and the overflow word inside it)
template <class T> struct UL {
    T v;
    RTK_HD operator T() const { return rtk_u(v); }
    RTK_HD T get() const { return rtk_u(v); }
    RTK_HD UL& operator=(T x) { v = x; return *this; }
    RTK_HD T operator->() const { return rtk_u(v); }
    RTK_HD decltype(auto) operator*() const { return *rtk_u(v); }
};

#define RTK_NONE32 0xFFFFFFFFu
#define RTK_EMPTY_KEY 0xFFFFFFFFFFFFFFFFull

// per-unitig flag word
#define RTK_F_EDGE_MASK 0xFFu      // bits 4..7 fw successor-base mask, bits 0..3 bw mask (UnitigData.hpp:275-289)
#define RTK_F_SHORT_CYCLE (1u << 8) // UnitigData.hpp:302-305
#define RTK_F_BRANCHING (1u << 9)   // UnitigData.hpp:407-410
#define RTK_F_AMBIGUITY (1u << 10)  // UnitigData.hpp:483-486

struct GraphView {
    U<int32_t> k;
    U<uint32_t> n_unitigs;
    U<uint64_t> n_kmers;
    U<uint64_t> ht_slots;         // slots of the k-mer table (any number: a hash is mapped to its slot by multiply-high, rtk_ht_slot)
    U<const uint64_t*> useq;      // unitig bases, 2 bits each, base i of the pool at bits [2*(i&31), +1] of word i>>5
    U<const uint64_t*> uoff;      // [n+1] first base of unitig u in the pool
    U<const uint32_t*> adj;       // [n*8] fw A,C,G,T then reverse-strand A,C,G,T: neighbour unitig<<1|strand or RTK_NONE32
    U<const uint32_t*> flags;     // [n]
    U<const uint32_t*> kcov;      // [n] round(cov/(size-k+1)) (UnitigData.hpp:396-399), precomputed in double on the host
    U<const uint32_t*> card;      // [n] |global| + |local|
    U<const uint64_t*> loff;      // [n+1] local colour set of u = col[loff[u] .. loff[u+1])
    U<const int32_t*> gid;        // [n] global colour set id or -1
    U<const uint64_t*> goff;      // [n_global+1] global set g = col[goff[g] .. goff[g+1])
    U<const uint32_t*> col;       // sorted u32 pair ids
    U<const uint64_t*> ht;        // [2*slots] {canonical k-mer, unitig<<32 | dist<<1 | stored_is_canonical}, empty key = RTK_EMPTY_KEY
    U<const uint64_t*> bf;        // [bf_mask+1] blocked Bloom filter over the canonical k-mers (2 bits of one 64-bit word per k-mer)
    U<uint64_t> bf_mask;
    U<const uint64_t*> bf1;       // cache-sized first-level filter in front of `bf`: one bit per k-mer in a bit array of bf1_mask + 1 bits (a single all-ones word when disabled)
    U<uint64_t> bf1_mask;
    U<const uint64_t*> cycoff;    // [n+1] compact cycles of unitig u = cyc[cycoff[u] .. cycoff[u+1]) (NUL-terminated strings of successor bases)
    U<const char*> cyc;
    U<const uint64_t*> amb;       // SNP annotations: amb[u]..amb[u+1] index the entries of unitig u, entry j = amb[n_unitigs + 1 + j] = position<<4 | IUPAC index, by (position, code)
    U<const uint64_t*> hap;       // haplotype ids: hap[u]..hap[u+1] index the ids of unitig u at hap[n_unitigs + 1 + j] (not read by `correct` without -p/-P)
    U<uint64_t> n_amb;            // number of annotation entries (0: getAmbiguityVector / fixAmbiguity are identities)
    U<const uint64_t*> hx;        // [hx_mask+1] half-k-mer index for the 1-edit search: slot = CANONICAL h-mer << 34 | first (h = (k-1)/2; the smaller of an h-mer of the forward unitig
    U<uint64_t> hx_mask;          //   sequences and its reverse complement), empty = RTK_EMPTY_KEY; hxl[first] = number of places, then two words per place: flanks (h + 1 bases in front << 32 | h + 1 bases behind, as the unitig spells them), reversed<<63 | unitig<<32 | front-exists<<31 | offset.
    U<const uint64_t*> hxl;       //   hx_mask == 0: no index (the search spells the variants instead)
};

RTK_HD uint32_t rtk_ulen(const GraphView& g, uint32_t u) { return static_cast<uint32_t>(g.uoff[u + 1] - g.uoff[u]); }
RTK_HD uint32_t rtk_nkm(const GraphView& g, uint32_t u) { return rtk_ulen(g, u) - static_cast<uint32_t>(g.k) + 1u; }
RTK_HD uint32_t rtk_base(const GraphView& g, uint64_t pos) { return static_cast<uint32_t>((g.useq[pos >> 5] >> (2 * (pos & 31))) & 3ull); }

RTK_HD uint64_t rtk_hash64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

RTK_HD uint64_t rtk_revcomp(uint64_t x, int k) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64 - 2 * k);
}

// ---- the map of BatchView::counters (rtk_seed_types.h): every slot or range that any kernel or the host uses, with who writes it. The block is cleared at the start
// of the seed stage (rtk_seed_stage.inc) and of the pass-2 phasing step (rtk_pipeline.inc) and copied back once at the end of the region stage. Slots outside a range are free.
enum RtkCounterSlot {
    RTK_CNT_WINDOWS = 0, RTK_CNT_PROBES_EXACT = 1, RTK_CNT_PROBES_INEXACT = 2, RTK_CNT_HITS_INEXACT = 3, RTK_CNT_REGIONS = 4, RTK_CNT_ITEMS = 5, // seed kernels -> rtk_stats
    RTK_CNT_OVERFLOW = 6,           // seed kernels: a pool ran out (the host grows it and redoes the stage)
    RTK_CNT_EXPAND = 7, RTK_CNT_COLOUR = 8, RTK_CNT_PATHBASE = 9, RTK_CNT_ALIGN = 10, RTK_CNT_CELLS = 11, // k_regions, k_regions_lanes -> rtk_stats
    RTK_CNT_SLOTS_EXACT = 12, RTK_CNT_SLOTS_INEXACT = 13, // table slots read by the two scans -> rtk_stats
    RTK_CNT_EVENTS_END = 14,        // (what the seed stage reads back after every attempt: [0, RTK_CNT_SEED_READBACK))
    RTK_CNT_SEED_READBACK = 16,
    RTK_CNT_CYC = 16,               // [8] k_regions wave cycles -> rtk_stats: colour, paths, consensus, total, myers, sets + path records, to_string, path quality
    RTK_CNT_CYC_COLOUR = 16, RTK_CNT_CYC_PATHS = 17, RTK_CNT_CYC_CONSENSUS = 18, RTK_CNT_CYC_TOTAL = 19, RTK_CNT_CYC_MYERS = 20, RTK_CNT_CYC_SETS = 21, RTK_CNT_CYC_TOSTRING = 22, RTK_CNT_CYC_PATHQUAL = 23,
    RTK_CNT_CYC_END = 24,
    RTK_CNT_FINALIZE = 24,          // [7] k_finalize: wave cycles of its phases (trace)
    RTK_CNT_FINALIZE_SLOWEST = 31,  // k_finalize: cycles of the slowest read (atomicMax; trace)
    RTK_CNT_FINALIZE_END = 32,
    RTK_CNT_WALK = 32,              // [6] k_regions, traceback walks: cycles, moves (both -> rtk_stats), reloads, scalar steps, calls, tail cycles (trace)
    RTK_CNT_WALK_CYCLES = 32, RTK_CNT_WALK_MOVES = 33, RTK_CNT_WALK_RELOADS = 34, RTK_CNT_WALK_SCALAR = 35, RTK_CNT_WALK_CALLS = 36, RTK_CNT_WALK_TAIL = 37,
    RTK_CNT_CYC_DFS = 38, RTK_CNT_CYC_COLOUR_OK = 39, // k_regions: DFS bookkeeping, of which colour checks (trace)
    RTK_CNT_WALK_END = 40,
    RTK_CNT_FINE = 40,              // [16] k_regions: RegionScratch::fine (RTK_FINE_*; trace)
    RTK_CNT_FINE_END = 56,
    RTK_CNT_HIST = 56,              // [32] k_regions: RegionScratch::hist, the size-class table (trace)
    RTK_CNT_HIST_END = 88,
    RTK_CNT_PHASE_TRACE = 59,       // [5] pass 2, k_phase_long: alignment cycles, then the Hirschberg driver's pass / split / leaf / total cycles (trace). INSIDE RTK_CNT_HIST
    RTK_CNT_PHASE_TRACE_END = 64,
    RTK_CNT_FINALIZE_SLOWEST_PHASES = 72, // [7] k_finalize: the phases of the slowest read (trace). INSIDE RTK_CNT_HIST
    RTK_CNT_FINALIZE_SLOWEST_PHASES_END = 79,
    RTK_CNT_PROF = 96,              // [48] k_regions of a -DRTK_PROF build: RegionScratch::prof (trace)
    RTK_CNT_PROF_END = 144,
    RTK_CNT_WAVE_TRACE = 144,       // [8] k_regions of a traced run: longest region, ~first start, last end, sum of lifetimes, waves, longest region again, its place, most regions on a wave
    RTK_CNT_WAVE_TRACE_END = 152,
    RTK_CNT_LANE_HANDED = 152, RTK_CNT_LANE_DONE = 153, // k_regions_lanes: regions handed on to the wave kernel / finished -> rtk_stats
    RTK_CNT_LANE_END = 154,
    RTK_CNT_ROUTES = 154,           // [5] k_regions: trims stored / by column / by the distance call, consensus calls resumed / swept (RTK_RC_TRIM_STORED ..) -> rtk_stats
    RTK_CNT_ROUTES_END = 159,
    RTK_CNT_LANE_PROF = 160,        // [24 = RL_NPROF] k_regions_lanes of a -DRTK_LANE_PROF build: lane cycles by slot (trace)
    RTK_CNT_LANE_PROF2 = 184,       // [24] the same build: wave-time estimate by slot (trace)
    RTK_CNT_LANE_PROF_END = 208,
    RTK_CNT_PHASE_SKIPPED = 210,    // pass 2: reads whose whole-read alignment was skipped (rtk_phasing.h) -> rtk_stats
    RTK_CNT_FA_LINKED = 211,        // [3] k_regions, fixAmbiguity: linked-allele searches run / skipped, entries they produced (RTK_RC_FA_LINKED_RUN ..) -> rtk_stats
    RTK_CNT_FA_LINKED_END = 214,
    RTK_CNT_STRAND2 = 214,          // [3] k_regions, gap regions whose forward strand did not decide alone: second strand run / skipped, audit mismatches (RTK_RC_STRAND2_RUN ..) -> rtk_stats
    RTK_CNT_STRAND2_END = 217,
    RTK_CNT_PARK = 217,             // [2] k_regions, stored sweeps of the forward trims: walked for a consensus / never walked (RTK_RC_PARK_WALKED ..) -> rtk_stats
    RTK_CNT_PARK_END = 219,
    RTK_CNT_COLOURS = 219,          // [6] k_regions, calls of rtk_choose_colors by the program that answered: small, wide, bits, general; audit mismatches; calls the register program declined for room (RTK_RC_COLOURS_SMALL ..) -> rtk_stats
    RTK_CNT_COLOURS_END = 225,
    RTK_CNT_PARK_RESWEEPS = 225,    // k_regions, forward trims without a table whose path was walked from a second sweep (RTK_RC_PARK_RESWEEPS) -> rtk_stats
    RTK_CNT_USED_END = 226,
    RTK_CNT_TOTAL = (RTK_CNT_USED_END + 31) / 32 * 32 // words in the block: what is used, rounded up to 256 bytes (the tail is free)
};
static_assert(RTK_CNT_TOTAL == 256, "counter map: the size of the block changed (it is part of what the kernels and the host agree on)");
// Two trace-only users sit INSIDE the size-class table today: RTK_CNT_PHASE_TRACE (written by the phasing step, which runs before the seed stage clears the block
// -- so it is read back right there) and RTK_CNT_FINALIZE_SLOWEST_PHASES (written by k_finalize, read back by the seed stage; k_regions then adds its table on top).
// Both only garble developer trace lines of the size-class table; renumbering them is a follow-up, because it changes device code. What reaches rtk_stats must
// not share a slot with anything:
constexpr bool rtk_cnt_apart(int a, int a_end, int b, int b_end) { return a_end <= b || b_end <= a; }
static_assert(RTK_CNT_EVENTS_END <= RTK_CNT_CYC && RTK_CNT_CYC_END <= RTK_CNT_FINALIZE && RTK_CNT_FINALIZE_END <= RTK_CNT_WALK && RTK_CNT_WALK_END <= RTK_CNT_FINE, "counter map: the event, cycle, finalize and walk ranges overlap");
static_assert(RTK_CNT_FINE_END <= RTK_CNT_HIST && RTK_CNT_HIST_END <= RTK_CNT_PROF && RTK_CNT_PROF_END <= RTK_CNT_WAVE_TRACE && RTK_CNT_WAVE_TRACE_END <= RTK_CNT_LANE_HANDED, "counter map: the trace ranges overlap");
static_assert(RTK_CNT_LANE_END <= RTK_CNT_ROUTES && RTK_CNT_ROUTES_END <= RTK_CNT_LANE_PROF, "counter map: the route counters overlap the lane ranges");
static_assert(RTK_CNT_LANE_END <= RTK_CNT_LANE_PROF && RTK_CNT_LANE_PROF2 - RTK_CNT_LANE_PROF == 24 && RTK_CNT_LANE_PROF_END <= RTK_CNT_PHASE_SKIPPED && RTK_CNT_PHASE_SKIPPED < RTK_CNT_TOTAL, "counter map: the lane ranges overlap");
static_assert(RTK_CNT_PHASE_SKIPPED < RTK_CNT_FA_LINKED && RTK_CNT_FA_LINKED_END <= RTK_CNT_TOTAL, "counter map: the fixAmbiguity counters overlap the phasing slot or leave the block");
static_assert(RTK_CNT_FA_LINKED_END <= RTK_CNT_STRAND2 && RTK_CNT_STRAND2_END <= RTK_CNT_TOTAL, "counter map: the second-strand counters overlap the fixAmbiguity counters or leave the block");
static_assert(RTK_CNT_STRAND2_END <= RTK_CNT_PARK && RTK_CNT_PARK_END <= RTK_CNT_TOTAL, "counter map: the park counters overlap the second-strand counters or leave the block");
static_assert(RTK_CNT_PARK_END <= RTK_CNT_COLOURS && RTK_CNT_COLOURS_END <= RTK_CNT_TOTAL, "counter map: the colour-route counters overlap the park counters or leave the block");
static_assert(rtk_cnt_apart(RTK_CNT_PHASE_TRACE, RTK_CNT_PHASE_TRACE_END, RTK_CNT_FINALIZE_SLOWEST_PHASES, RTK_CNT_FINALIZE_SLOWEST_PHASES_END), "counter map: the two guests of the size-class table overlap");
static_assert(RTK_CNT_HIST <= RTK_CNT_PHASE_TRACE && RTK_CNT_FINALIZE_SLOWEST_PHASES_END <= RTK_CNT_HIST_END, "counter map: the guests of the size-class table left it (update the comment above)");

// indices of RegionScratch::cnt (rtk_region_types.h): a wave's own accumulators, added to the block when its kernel ends
enum RtkRegionCnt { RTK_RC_EXPAND = 0, RTK_RC_COLOUR = 1, RTK_RC_PATHBASE = 2, RTK_RC_ALIGN = 3, RTK_RC_CELLS = 4, // -> RTK_CNT_EXPAND .. RTK_CNT_CELLS
    RTK_RC_CYC_COLOUR = 5, RTK_RC_CYC_PATHS = 6, RTK_RC_CYC_CONSENSUS = 7, RTK_RC_CYC_TOTAL = 8, RTK_RC_CYC_MYERS = 9, RTK_RC_CYC_SETS = 10, // [5, 11) -> RTK_CNT_CYC + 0 .. 5
    RTK_RC_CYC_PATHREC = 11 /* -> RTK_CNT_CYC_SETS as well */, RTK_RC_CYC_TOSTRING = 12, RTK_RC_CYC_PATHQUAL = 13, RTK_RC_CYC_DFS = 14, RTK_RC_CYC_COLOUR_OK = 15,
    // routes of the trims and the consensus (rtk_trim_by_column, rtk_generate_consensus) -> RTK_CNT_ROUTES + 0 .. 4: trims by column with a stored sweep (forward
    // strand of a gap region) / without, trims by the distance call; consensus calls whose forward-string alignment was resumed from the trim's sweep / swept
    RTK_RC_TRIM_STORED = 16, RTK_RC_TRIM_COLUMN = 17, RTK_RC_TRIM_FALLBACK = 18, RTK_RC_CONS_RESUMED = 19, RTK_RC_CONS_SWEPT = 20,
    // linked-allele searches of rtk_fix_ambiguity (rtk_ambiguity.h) -> RTK_CNT_FA_LINKED + 0 .. 2: searches run, searches skipped because no other entry of the
    // safe set was undecided, entries of s_ambiguity the searches produced
    RTK_RC_FA_LINKED_RUN = 21, RTK_RC_FA_LINKED_SKIPPED = 22, RTK_RC_FA_LINKED_ENTRIES = 23,
    // second strand of a gap region (rtk_region_program, rtk_strand2_skippable) -> RTK_CNT_STRAND2 + 0 .. 2: regions that ran it, regions whose forward result
    // decided the bytes alone, and -- RTK_STRAND2_AUDIT=1 -- regions of the second kind whose full route gave other bytes than the forward result
    RTK_RC_STRAND2_RUN = 24, RTK_RC_STRAND2_SKIPPED = 25, RTK_RC_STRAND2_AUDIT_MISMATCH = 26,
    // stored sweeps of the forward trims (rtk_trim_by_column, rtk_park_walk) -> RTK_CNT_PARK + 0 .. 1: those whose path was walked and parked for a consensus, and
    // those nobody walked (the region skipped its second strand, or the sweep could not be parked); the sum is RTK_RC_TRIM_STORED
    RTK_RC_PARK_WALKED = 27, RTK_RC_PARK_DEFERRED = 28,
    // calls of rtk_choose_colors (rtk_colours.h) by the program that answered -> RTK_CNT_COLOURS + 0 .. 5: rtk_choose_colors_small with at most RTK_CS_MAX_IDS ids
    // (repeats counted) / with more ("wide"), rtk_choose_colors_bits, rtk_choose_colors_general; -- RTK_COLOURS_AUDIT=1 -- calls whose first answer differed from the
    // general program's; and calls rtk_choose_colors_small handed on because universe and bit vectors did not fit its LDS buffer (they are answered, and counted, further on)
    RTK_RC_COLOURS_SMALL = 29, RTK_RC_COLOURS_WIDE = 30, RTK_RC_COLOURS_BITS = 31, RTK_RC_COLOURS_GENERAL = 32, RTK_RC_COLOURS_AUDIT_MISMATCH = 33, RTK_RC_COLOURS_DECLINED_FIT = 34,
    // forward trims that kept only the last column of their sweep and whose path was walked after all, from a second, stored sweep (rtk_park_walk) -> RTK_CNT_PARK_RESWEEPS
    RTK_RC_PARK_RESWEEPS = 35, RTK_RC_N = 36 };
static_assert(RTK_CNT_ROUTES_END - RTK_CNT_ROUTES == static_cast<int>(RTK_RC_FA_LINKED_RUN) - static_cast<int>(RTK_RC_TRIM_STORED), "counter map: one slot per route counter");
static_assert(RTK_CNT_FA_LINKED_END - RTK_CNT_FA_LINKED == static_cast<int>(RTK_RC_STRAND2_RUN) - static_cast<int>(RTK_RC_FA_LINKED_RUN), "counter map: one slot per fixAmbiguity counter");
static_assert(RTK_CNT_STRAND2_END - RTK_CNT_STRAND2 == static_cast<int>(RTK_RC_PARK_WALKED) - static_cast<int>(RTK_RC_STRAND2_RUN), "counter map: one slot per second-strand counter");
static_assert(RTK_CNT_PARK_END - RTK_CNT_PARK == static_cast<int>(RTK_RC_COLOURS_SMALL) - static_cast<int>(RTK_RC_PARK_WALKED), "counter map: one slot per park counter");
static_assert(RTK_CNT_COLOURS_END - RTK_CNT_COLOURS == static_cast<int>(RTK_RC_PARK_RESWEEPS) - static_cast<int>(RTK_RC_COLOURS_SMALL), "counter map: one slot per colour-route counter");
// OptsView::colours_mode (rtk_seed_types.h; RTK_COLOURS_ROUTE, RTK_COLOURS_AUDIT, RTK_TEST_COLOURS_FAULT of rtk_knobs.h): route in bits 0 .. 1, the audit and its test hook above
#define RTK_CM_ROUTE 3u
#define RTK_CM_ROUTE_BITS 1u
#define RTK_CM_ROUTE_GENERAL 2u
#define RTK_CM_AUDIT 4u
#define RTK_CM_FAULT 8u
// indices of RegionScratch::fine -> RTK_CNT_FINE + i (their names in the trace: region_trace_report, rtk_pipeline_run.inc)
enum RtkRegionFine { RTK_FINE_COL_GENERAL = 0 /* [7] the laps of rtk_choose_colors_general: 1 .. 4 are ALSO the laps of rtk_fix_ambiguity (trace only) */, RTK_FINE_COL_UNIONS = 0, RTK_FINE_FA_ALIGN = 1, RTK_FINE_FA_WALK = 2, RTK_FINE_FA_LINKED = 3, RTK_FINE_FA_APPLY = 4, RTK_FINE_COL_S_VECTORS = 5, RTK_FINE_COL_S_SELECT = 6,
    RTK_FINE_SIDE_LISTS = 7, RTK_FINE_TRIM = 8, RTK_FINE_FIX_AMBIGUITY = 9, RTK_FINE_FA_CALLS = 10, RTK_FINE_FA_ALL_CONFIDENT = 11, RTK_FINE_COL_S_CYCLES = 12, RTK_FINE_COL_B_CYCLES = 13,
    RTK_FINE_COL_S_CALLS = 14, RTK_FINE_COL_B_CALLS = 15, RTK_FINE_N = 16 };

// Unitig mapping (restates the fields of Bifrost's const_UnitigMap the hot path reads).
struct UMap {
    uint32_t unitig; // RTK_NONE32 == isEmpty
    uint32_t dist;
    uint32_t len;
    uint32_t strand; // 1 = forward
};

RTK_HD UMap rtk_um_empty() { UMap u; u.unitig = RTK_NONE32; u.dist = 0; u.len = 0; u.strand = 1; return u; }
RTK_HD bool rtk_um_is_empty(const UMap& u) { return u.unitig == RTK_NONE32; }
RTK_HD bool rtk_um_eq(const UMap& a, const UMap& b) { return a.unitig == b.unitig && a.dist == b.dist && a.len == b.len && a.strand == b.strand; }

// packed anchor hit: unitig<<33 | dist<<1 | strand ; all ones = no hit
#define RTK_NO_HIT 0xFFFFFFFFFFFFFFFFull
RTK_HD uint64_t rtk_pack_hit(uint32_t unitig, uint32_t dist, uint32_t strand) { return (static_cast<uint64_t>(unitig) << 33) | (static_cast<uint64_t>(dist) << 1) | (strand & 1u); }
RTK_HD UMap rtk_unpack_hit(uint64_t h) { UMap u; u.unitig = static_cast<uint32_t>(h >> 33); u.dist = static_cast<uint32_t>((h >> 1) & 0xFFFFFFFFull); u.len = 1; u.strand = static_cast<uint32_t>(h & 1ull); return u; }

// Exact k-mer lookup (Bifrost find(km,false) [A1]): fw = k-mer code in read orientation. *n_probes = 16-byte table slots visited
// (0 when the pre-filter already answered).
// slot of a hash in a table of `slots` entries: floor(hash * slots / 2^64) -- no power-of-two table sizes needed (a 3 Gb graph: 69 GB at load 0.7
// instead of 137 GB), the high hash bits decide; next slot of the linear probe
RTK_HD uint64_t rtk_ht_slot(uint64_t hh, uint64_t slots) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RTK_SIM)
    return __umul64hi(hh, slots);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(hh) * static_cast<unsigned __int128>(slots)) >> 64);
#endif
}
RTK_HD uint64_t rtk_ht_next(uint64_t i, uint64_t slots) { return i + 1 == slots ? 0 : i + 1; }

RTK_HD uint64_t rtk_find_kmer(const GraphView& g, uint64_t fw, uint32_t* n_probes) {
    const uint64_t rc = rtk_revcomp(fw, g.k);
    const uint64_t can = fw < rc ? fw : rc;
    const uint64_t hh = rtk_hash64(can);
    { // first level: one bit in an array small enough to stay in L2
        const uint64_t b1 = (hh >> 12) & g.bf1_mask;
        if (!((g.bf1[b1 >> 6] >> (b1 & 63ull)) & 1ull)) { if (n_probes) *n_probes = 0; return RTK_NO_HIT; }
    }
    { // pre-filter: absent k-mers (the bulk of the 1-edit variants) stop here after one 8-byte read
        const uint64_t bits = (1ull << (hh & 63)) | (1ull << ((hh >> 6) & 63));
        if ((g.bf[(hh >> 32) & g.bf_mask] & bits) != bits) { if (n_probes) *n_probes = 0; return RTK_NO_HIT; }
    }
    uint64_t i = rtk_ht_slot(hh, g.ht_slots);
    uint32_t np = 0;
    while (true) {
        const uint64_t key = g.ht[2 * i];
        ++np;
        if (key == can) {
            const uint64_t v = g.ht[2 * i + 1];
            const uint32_t stored_is_can = static_cast<uint32_t>(v & 1ull), query_is_can = (fw <= rc) ? 1u : 0u;
            if (n_probes) *n_probes = np;
            return rtk_pack_hit(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>((v & 0xFFFFFFFFull) >> 1), stored_is_can == query_is_can ? 1u : 0u);
        }
        if (key == RTK_EMPTY_KEY) { if (n_probes) *n_probes = np; return RTK_NO_HIT; }
        i = rtk_ht_next(i, g.ht_slots);
    }
}


// ---- k in 33..63 (second pass, k2 = 63): two-word k-mers ------------------------------------------------------------------------
// Code = 2k bits right-aligned in {hi, lo}, first base in the most significant bits (k <= 32: hi = 0 and lo is the one-word code).
// The table keeps its 16-byte slots: the key word is a 64-bit fingerprint of the canonical k-mer and a fingerprint match is
// confirmed against the 2-bit unitig sequence the value word points at, so lookups stay exact.
struct RtkKm { uint64_t hi, lo; };
RTK_HD RtkKm rtk_km_zero() { RtkKm x; x.hi = 0; x.lo = 0; return x; }
RTK_HD bool rtk_km_eq(const RtkKm& a, const RtkKm& b) { return a.hi == b.hi && a.lo == b.lo; }
RTK_HD bool rtk_km_less(const RtkKm& a, const RtkKm& b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }
RTK_HD RtkKm rtk_km_mask(int k) { RtkKm m; m.lo = (k >= 32) ? ~0ull : ((1ull << (2 * k)) - 1ull); m.hi = (k <= 32) ? 0ull : ((1ull << (2 * k - 64)) - 1ull); return m; }
RTK_HD RtkKm rtk_km_push(const RtkKm& x, uint64_t b, int k) { // append base b (0..3) at the end, drop the first
    const RtkKm m = rtk_km_mask(k); RtkKm r; r.hi = ((x.hi << 2) | (x.lo >> 62)) & m.hi; r.lo = ((x.lo << 2) | b) & m.lo; return r;
}
RTK_HD RtkKm rtk_km_revcomp(const RtkKm& x, int k) {
    if (k <= 32) { RtkKm r; r.hi = 0; r.lo = rtk_revcomp(x.lo, k); return r; }
    const uint64_t a = rtk_revcomp(x.lo, 32), b = rtk_revcomp(x.hi, 32); // reverse complement of all 128 bits = {a, b}; the k-mer sits in its top 2k bits
    const int s = 128 - 2 * k; // 2..62
    RtkKm r; r.lo = (b >> s) | (a << (64 - s)); r.hi = a >> s; return r;
}
RTK_HD uint64_t rtk_km_hash(const RtkKm& can) { return rtk_hash64(can.lo ^ rtk_hash64(can.hi ^ 0x9e3779b97f4a7c15ull)); }
RTK_HD uint64_t rtk_km_fingerprint(const RtkKm& can) { const uint64_t f = rtk_hash64(can.lo + 0x9e3779b97f4a7c15ull) ^ rtk_hash64(can.hi ^ 0xd6e8feb86659fd93ull); return f == RTK_EMPTY_KEY ? 0ull : f; }
// reverse complement code of the k-mer starting at base `pos` of the 2-bit unitig pool (base p at bits 2(p & 31) of word p >> 5, i.e.
// last base in the most significant bits: complementing it IS the reverse-complement code). k in 33..63.
RTK_HD RtkKm rtk_km_rc_of_unitig(const GraphView& g, uint64_t pos, int k) {
    const uint64_t w = pos >> 5; const int sh = static_cast<int>(2 * (pos & 31));
    const uint64_t x0 = g.useq[w], x1 = g.useq[w + 1];
    RtkKm l;
    if (sh == 0) { l.lo = x0; l.hi = x1; }
    else { l.lo = (x0 >> sh) | (x1 << (64 - sh)); l.hi = x1 >> sh; if (sh + 2 * k > 128) l.hi |= g.useq[w + 2] << (64 - sh); }
    const RtkKm m = rtk_km_mask(k);
    l.lo = ~l.lo & m.lo; l.hi = ~l.hi & m.hi;
    return l;
}
RTK_HD uint64_t rtk_find_kmer_wide(const GraphView& g, const RtkKm& fw, uint32_t* n_probes) {
    const RtkKm rc = rtk_km_revcomp(fw, g.k);
    const RtkKm can = rtk_km_less(fw, rc) ? fw : rc;
    const uint64_t hh = rtk_km_hash(can);
    { const uint64_t b1 = (hh >> 12) & g.bf1_mask; if (!((g.bf1[b1 >> 6] >> (b1 & 63ull)) & 1ull)) { if (n_probes) *n_probes = 0; return RTK_NO_HIT; } }
    { const uint64_t bits = (1ull << (hh & 63)) | (1ull << ((hh >> 6) & 63)); if ((g.bf[(hh >> 32) & g.bf_mask] & bits) != bits) { if (n_probes) *n_probes = 0; return RTK_NO_HIT; } }
    const uint64_t fp = rtk_km_fingerprint(can);
    uint64_t i = rtk_ht_slot(hh, g.ht_slots);
    uint32_t np = 0;
    while (true) {
        const uint64_t key = g.ht[2 * i];
        ++np;
        if (key == fp) {
            const uint64_t v = g.ht[2 * i + 1];
            const uint32_t u = static_cast<uint32_t>(v >> 32), off = static_cast<uint32_t>((v & 0xFFFFFFFFull) >> 1);
            const RtkKm urc = rtk_km_rc_of_unitig(g, g.uoff[u] + off, g.k);
            if (rtk_km_eq(urc, rc)) { if (n_probes) *n_probes = np; return rtk_pack_hit(u, off, 1u); } // the query reads like the unitig
            if (rtk_km_eq(urc, fw)) { if (n_probes) *n_probes = np; return rtk_pack_hit(u, off, 0u); } // the query is its reverse complement
        }
        if (key == RTK_EMPTY_KEY) { if (n_probes) *n_probes = np; return RTK_NO_HIT; }
        i = rtk_ht_next(i, g.ht_slots);
    }
}
RTK_HD uint64_t rtk_find_km(const GraphView& g, const RtkKm& fw, uint32_t* n_probes) { return g.k <= 31 ? rtk_find_kmer(g, fw.lo, n_probes) : rtk_find_kmer_wide(g, fw, n_probes); }

// Split form of rtk_find_kmer for callers that want several filter reads in flight before any of them is consumed.
RTK_HD void rtk_kmer_prepare(uint64_t fw, int k, uint64_t* can, uint64_t* hh, uint32_t* query_is_can) {
    const uint64_t rc = rtk_revcomp(fw, k);
    *can = fw < rc ? fw : rc; *query_is_can = (fw <= rc) ? 1u : 0u; *hh = rtk_hash64(*can);
}
RTK_HD bool rtk_filter1_pass(uint64_t word1, uint64_t hh, uint64_t bf1_mask) { const uint64_t b1 = (hh >> 12) & bf1_mask; return (word1 >> (b1 & 63ull)) & 1ull; }
RTK_HD bool rtk_filter_pass(uint64_t word, uint64_t hh) { const uint64_t bits = (1ull << (hh & 63)) | (1ull << ((hh >> 6) & 63)); return (word & bits) == bits; }
RTK_HD uint64_t rtk_table_probe_from(const GraphView& g, uint64_t can, uint64_t i, uint32_t query_is_can, uint32_t* n_slots);
RTK_HD uint64_t rtk_table_lookup(const GraphView& g, uint64_t can, uint64_t hh, uint32_t query_is_can, uint32_t* n_slots) { return rtk_table_probe_from(g, can, rtk_ht_slot(hh, g.ht_slots), query_is_can, n_slots); }
// the linear probe from slot i on (a caller that has read the home slot itself continues at rtk_ht_next of it)
RTK_HD uint64_t rtk_table_probe_from(const GraphView& g, uint64_t can, uint64_t i, uint32_t query_is_can, uint32_t* n_slots) {
    uint32_t np = 0;
    while (true) {
        const uint64_t key = g.ht[2 * i]; ++np;
        if (key == can) { const uint64_t v = g.ht[2 * i + 1]; *n_slots = np; return rtk_pack_hit(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>((v & 0xFFFFFFFFull) >> 1), (static_cast<uint32_t>(v & 1ull) == query_is_can) ? 1u : 0u); }
        if (key == RTK_EMPTY_KEY) { *n_slots = np; return RTK_NO_HIT; }
        i = rtk_ht_next(i, g.ht_slots);
    }
}

#endif
