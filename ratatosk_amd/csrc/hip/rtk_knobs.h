// The run-time knobs of the library: every RTK_* environment variable that the code of this directory reads, and the only place that reads them.
// Per knob: type, default, what it does, and WHEN it is read -- on every call (a test may change it inside one process) or once per process (the first call
// fixes it: a test that needs another value starts a fresh process). None of them is part of the interface (include/ratatosk_hip.h); `Ratatosk correct` and
// the Python layer set none by default.
#ifndef RTK_KNOBS_H
#define RTK_KNOBS_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

// ---- how a value is parsed (absent = the default)
inline bool rtk_env_set(const char* name) { return getenv(name) != nullptr; }
inline bool rtk_env_is1(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
inline int rtk_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline int rtk_env_pos_int(const char* name, int dflt) { const int v = rtk_env_int(name, 0); return v > 0 ? v : dflt; } // (0, negative, not a number: the default)
inline uint64_t rtk_env_u64(const char* name, uint64_t dflt) { const char* e = getenv(name); return e ? strtoull(e, nullptr, 10) : dflt; }
inline bool rtk_env_eq(const char* name, const char* value) { const char* e = getenv(name); return e && !strcmp(e, value); }

// ---- trace and developer output: read on every call
inline bool rtk_knob_trace() { return rtk_env_set("RTK_TRACE"); }                 // flag: the [rtk trace] lines on stderr (a stage reads it once and hands it down)
inline int rtk_knob_trace_class(int dflt) { return rtk_env_int("RTK_TRACE_CLASS", dflt); } // int, unset: k_regions runs only the regions of one size class (0 .. 7; the output is NOT valid)
inline bool rtk_knob_lane_cost() { return rtk_env_set("RTK_LANE_COST"); }          // flag, simulator only: one line per region of the lane kernel
inline bool rtk_knob_myers_prof() { return rtk_env_set("RTK_MYERS_PROF"); }        // flag: rtk_myers_batch prints the cycle counters of the Hirschberg drivers
inline bool rtk_knob_myers_time() { return rtk_env_set("RTK_MYERS_TIME"); }        // flag: rtk_myers_batch prints its kernel times
inline bool rtk_knob_index_trace() { return rtk_env_set("RTK_INDEX_TRACE"); }      // flag: progress lines of the index build (rtk_index.hip and its stages rtk_index_*.h)
inline bool rtk_knob_load_trace() { return rtk_env_set("RTK_LOAD_TRACE"); }        // flag: progress lines of the graph upload (rtk_graph_tables.hip)

// ---- seed stage: read on every call
inline uint32_t rtk_knob_mask_seg() { return static_cast<uint32_t>(rtk_env_u64("RTK_MASK_SEG", 8192)); } // u32, 8192: characters of a read per k_mask work item (rounded up to 4096s by mask_seg())
inline int rtk_knob_seed_waves() { return rtk_env_pos_int("RTK_SEED_WAVES", 4096); } // int, 4096: waves of the per-read seed kernels
inline bool rtk_knob_inexact_enum() { return rtk_env_is1("RTK_INEXACT_ENUM"); }    // '1': the enumerating 1-edit search instead of the signature table (A/B, tests)
inline bool rtk_knob_inexact_shared() { return !rtk_env_eq("RTK_INEXACT_SHARED", "0"); } // '0': every window of k_inexact asks the half-k-mer index itself, instead of reading the tile's table of one look-up per read position (same results; A/B, tests)
inline bool rtk_knob_inexact_planes() { return !rtk_env_eq("RTK_INEXACT_PLANES", "0"); } // '0': every lane of k_inexact packs its window's characters from text, instead of taking them from the tile's bit planes (same results; A/B, tests)
inline bool rtk_knob_test_tiny_scratch() { return rtk_env_set("RTK_TEST_TINY_SCRATCH"); } // flag, test hook: attempt 0 of the seed, region and lane work areas is undersized, so that the redo paths run
// the reference's documented ambiguities (rtk_opts_default): which reading the library takes
inline int rtk_knob_a2_exclusive() { return rtk_env_eq("RTK_A2_XOR", "union") ? 0 : (rtk_env_eq("RTK_A2_XOR", "exclusive-ids") ? 2 : 1); } // "union" | "exclusive-ids" | (default) 1
inline int rtk_knob_a3_strand_order() { return rtk_env_eq("RTK_A3_ORDER", "strand") ? 1 : 0; } // "strand": 1
inline int rtk_knob_d1_desc() { return rtk_env_eq("RTK_D1_ORDER", "desc") ? 1 : 0; }         // "desc": 1

// ---- pass-2 phasing step: read on every call
inline bool rtk_knob_phase_align_all() { return rtk_env_is1("RTK_PHASE_ALIGN_ALL"); } // '1': align every read, also those without an unsupported stretch
inline uint32_t rtk_knob_phase_long() { return static_cast<uint32_t>(rtk_env_u64("RTK_PHASE_LONG", 24576)); } // u32, 24576: reads from this length on go to the multi-wave kernel (0: none)
inline int rtk_knob_phase_lwaves() { return std::max(1, std::min(16, rtk_env_int("RTK_PHASE_LWAVES", 4))); } // int 1 .. 16, 4: waves per workgroup of that kernel
inline int rtk_knob_phase_pgrid() { return rtk_env_int("RTK_PHASE_PGRID", 1024); } // int, 1024: waves of the single-wave phasing kernel, first attempt
inline int rtk_knob_phase_lgrid() { return rtk_env_int("RTK_PHASE_LGRID", 192); }  // int, 192: workgroups of the multi-wave kernel, first attempt
inline int rtk_knob_phase_mgrid() { return rtk_env_int("RTK_PHASE_MGRID", 768); }  // int, 768: waves of the middle class, first attempt

// ---- region stage: read on every call
inline bool rtk_knob_lane_max_gap_set() { return rtk_env_set("RTK_LANE_MAX_GAP"); } // (set at all: switches the automatic choice by ticket size off)
inline uint32_t rtk_knob_lane_max_gap() { return static_cast<uint32_t>(rtk_env_u64("RTK_LANE_MAX_GAP", 0)); } // u32, 0 = off: gaps under this many bases go to the lane-per-region kernel
inline int rtk_knob_lane_waves() { return rtk_env_pos_int("RTK_LANE_WAVES", 1024); } // int, 1024: resident waves of the lane kernel
inline bool rtk_knob_lane_serial() { return rtk_env_is1("RTK_LANE_SERIAL"); }      // '1': the lane kernel before the wave kernel on one stream instead of beside it (A/B)
inline int rtk_knob_lane_round() { return rtk_env_int("RTK_LANE_ROUND", 64); }     // int, 64: regions a lane wave takes off its queue at a time
inline bool rtk_knob_compact() { return rtk_env_is1("RTK_COMPACT"); }              // '1': a first attempt with ~1.3 MB work areas (for graphs that leave little HBM)
inline int rtk_knob_region_waves() { return rtk_env_pos_int("RTK_REGION_WAVES", 4096); } // int, 4096: persistent waves of k_regions
inline int rtk_knob_p2_rgrid() { return rtk_env_int("RTK_P2_RGRID", 512); }        // int, 512: cap of the waves of a second-pass ticket's k_regions
inline bool rtk_knob_fa_linked_always() { return rtk_env_is1("RTK_FA_LINKED_ALWAYS"); } // '1': fixAmbiguity runs every linked-allele search, also those that cannot append (same results; parity test, A/B traces)
inline bool rtk_knob_strand2_always() { return rtk_env_is1("RTK_STRAND2_ALWAYS"); } // '1': every gap region that is not corrected by its forward strand alone runs the second strand, as the reference does (same results; parity test, A/B timing)
inline bool rtk_knob_strand2_audit() { return rtk_env_is1("RTK_STRAND2_AUDIT"); }   // '1': where the rule would skip the second strand the full route runs and is emitted, and every difference to the forward result is counted (rtk_stats::n_strand2_audit_mismatch)
inline uint32_t rtk_knob_colours_route() { return rtk_env_eq("RTK_COLOURS_ROUTE", "bits") ? 1u : (rtk_env_eq("RTK_COLOURS_ROUTE", "general") ? 2u : 0u); } // "bits": rtk_choose_colors skips its small program; "general": the general program answers every call (same results; tests/test_colour_routes.py)
inline uint32_t rtk_knob_colours_audit() { return rtk_env_is1("RTK_COLOURS_AUDIT") ? (rtk_env_is1("RTK_TEST_COLOURS_FAULT") ? 3u : 1u) : 0u; } // RTK_COLOURS_AUDIT '1': the general program repeats every selection another program answered, differences are counted (rtk_stats::n_colours_audit_mismatch); with the test hook RTK_TEST_COLOURS_FAULT '1' (3) the first answer loses its largest id before the comparison
inline bool rtk_knob_park_eager() { return rtk_env_is1("RTK_PARK_EAGER"); }         // '1': the forward trim of a gap region walks and parks its alignment right away, also where no consensus will read it (same results; parity test, A/B timing)
inline bool rtk_knob_trim_store() { return rtk_env_is1("RTK_TRIM_STORE"); }         // '1': the forward trim of a gap region stores the whole table of its sweep, instead of keeping the delta vectors of the last column alone (same results; parity test, A/B timing)
inline bool rtk_knob_test_coalesce_fail() { return rtk_env_set("RTK_TEST_COALESCE_FAIL"); } // flag, test hook: a merged batch is reported as failed (its members must come through on their own)

// ---- region stage and rtk_correct_batch: read ONCE per process (the first call fixes the value)
inline uint64_t rtk_knob_lane_auto_bases() { static const uint64_t v = rtk_env_u64("RTK_LANE_AUTO_BASES", 512ull << 20); return v; } // u64, 512 Mi, 0 = never: tickets from this size on take the lane kernel unasked
inline uint64_t rtk_knob_half_slab_bases() { static const uint64_t v = rtk_env_u64("RTK_HALF_SLAB_BASES", 8ull << 20); return v; }   // u64, 8 Mi, 0 = never: tickets up to this size share the work areas two at a time
inline int rtk_knob_half_waves() { static const int v = std::min(rtk_env_pos_int("RTK_HALF_WAVES", 2048), 2048); return v; }          // int <= 2048, 2048: persistent waves on one half of the work areas
inline uint64_t rtk_knob_coalesce_bases() { static const uint64_t v = rtk_env_u64("RTK_COALESCE_BASES", 16ull << 20); return v; }     // u64, 16 Mi, 0 = every call on its own: size up to which concurrent calls are merged
inline long rtk_knob_coalesce_wait_us() { static const long v = [] { const char* e = getenv("RTK_COALESCE_WAIT_US"); return e ? atol(e) : 1500L; }(); return v; } // long, 1500: how long a call waits for company
inline uint32_t rtk_knob_coalesce_split() { static const uint32_t v = static_cast<uint32_t>(rtk_env_pos_int("RTK_COALESCE_SPLIT", 2)); return v; } // u32 >= 1, 2: parts a merged batch is cut into

// ---- index build and graph upload (rtk_index.hip and its stages rtk_index_*.h, rtk_graph_tables.hip): read on every call
inline uint64_t rtk_knob_index_cap(uint64_t dflt) { return rtk_env_u64("RTK_INDEX_CAP", dflt); }         // u64: slots of the k-mer count table (default: from the input size)
inline uint64_t rtk_knob_index_chunk(uint64_t dflt) { const uint64_t v = rtk_env_u64("RTK_INDEX_CHUNK", 0); return v >= 1024 ? v : dflt; } // u64 >= 1024: bytes of input per chunk (tests: small chunks cut long records)
inline int rtk_knob_index_keep_text() { return rtk_env_int("RTK_INDEX_KEEP_TEXT", -1); }                 // 0 | non-zero | unset (-1: decided from the free memory): keep the packed input on the device
inline uint64_t rtk_knob_index_events(uint64_t dflt) { return rtk_env_u64("RTK_INDEX_EVENTS", dflt); }   // u64: capacity of the (unitig, read) event buffer of the colouring
inline uint64_t rtk_knob_index_cover_cap(uint64_t dflt) { return rtk_env_u64("RTK_INDEX_COVER_CAP", dflt); } // u64 >= 1: crossings the buffer of rtk_index_cover_* has room for at first (tests: 1, every chunk with a crossing is mapped a second time)
inline uint64_t rtk_knob_index_snp_mem(uint64_t dflt) { return std::min(dflt, rtk_env_u64("RTK_INDEX_SNP_MEM", dflt)); } // u64 bytes: rtk_index_snp_candidates compares its need with this instead of the free device memory when it is lower (tests: the refusal)
inline uint32_t rtk_knob_index_snp_passes() { return static_cast<uint32_t>(std::min<uint64_t>(rtk_env_u64("RTK_INDEX_SNP_PASSES", 0), 0xFFFFFFFFull)); } // u32, 0 = as few as fit: rtk_index_snp_candidates searches in exactly this many passes over partitions of the key space (clamped to min(256, prefix values); tests: the partitioned path on small inputs)
inline uint64_t rtk_knob_index_pair_mem(uint64_t dflt) { return std::min(dflt, rtk_env_u64("RTK_INDEX_PAIR_MEM", dflt)); } // u64 bytes: rtk_index_pair_ids compares its need with this instead of the free device memory when it is lower (tests: the refusal)
inline uint32_t rtk_knob_index_pair_passes() { return static_cast<uint32_t>(std::min<uint64_t>(rtk_env_u64("RTK_INDEX_PAIR_PASSES", 0), 0xFFFFFFFFull)); } // u32, 0 = as few as fit: rtk_index_pair_ids pairs in exactly this many passes over equal ranges of the hash space (clamped to 256; tests: the partitioned path on small inputs)
inline uint64_t rtk_knob_hx_part_keys(uint64_t dflt) { return rtk_env_u64("RTK_HX_PART_KEYS", dflt); }   // u64: keys per partition when the signature table is built

// ---- identity to the truth (rtk_identity.hip): read when a job begins
inline int rtk_knob_identity_waves() { return std::min(rtk_env_pos_int("RTK_IDENTITY_WAVES", 1024), 16384); } // int <= 16384, 1024: persistent waves of k_identity per chunk in flight (two chunks: twice as many work areas)

// ---- simulator only
inline int rtk_knob_sim_devices() { return std::max(1, rtk_env_int("RTK_SIM_DEVICES", 1)); } // int, 1: pretend GPUs, so that the multi-GPU host plumbing runs on a CPU (every call)

// The knobs of the other binaries and layers are read where they are used; for the sake of one complete list:
//   csrc/common (readers): RTK_ALLOW_TINYBITMAP, RTK_ZLIB_INFLATE
//   csrc/host (graph file -> flat tables, the Ratatosk driver): RTK_BF1_LOG2BITS, RTK_BF1_OFF, RTK_BF_KEYS_PER_WORD, RTK_HT_DENSE_KMERS, RTK_HX_MAX_GB, RTK_INEXACT_ENUM,
//     RTK_LOAD_TRACE, RTK_CLI_STATS, RTK_CLI_TRACE, RTK_SERIAL_READER
//   csrc/tools (rtk_build_index): RTK_FASTA_MEMBER_BYTES, RTK_INDEX_HOST_COLOURS, RTK_INDEX_HOST_UNITIGS, RTK_INDEX_SNPS (device | host: where --gpu --snps finds its candidates),
//     RTK_INDEX_THREADS, RTK_INDEX_TRACE, RTK_INDEX_CHUNK (--gpu --cover-edges-from: characters of cover text per chunk; --pair-by-name --fast: bytes per range of a plain file)
//   csrc/tools (rtk_rescue_reads): RTK_INDEX_CHUNK (characters of -u text per batch), RTK_INDEX_THREADS, RTK_INDEX_TRACE
//   csrc/tools (rtk_qv): RTK_INDEX_CHUNK (characters of -l text per chunk; a longer read is cut into pieces), RTK_INDEX_THREADS, RTK_INDEX_TRACE (--gpu: also the time of k_qv alone)
//   csrc/tools (rtk_identity): RTK_INDEX_CHUNK (characters of -l text per chunk), RTK_INDEX_THREADS, RTK_INDEX_TRACE (--gpu: also the time of k_identity alone and the tail of its launches)
//   ratatosk_amd/api.py: RTK_LIB_OVERRIDE (another build of the library), RTK_HOST_TABLES

#endif
